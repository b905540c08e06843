#!/usr/bin/env python
"""Measure libcolorcc_hip.so on the device: its error against the numpy helper and its time.

    python tools/color_correct_bench.py [--out_dir D] [--skip_error] [--skip_time] [--once]

error -> r11_color_correct_error.json: per case of tests.color_correct_reference.well_conditioned_cases() the worst
|device - helper| in rgb_cc, differing bytes, PSNR difference, and the relative error of colorcc_normal_equations against
float64 numpy sums (relative to the sum of absolute products); the dark frame (render x 0.02) is reported, not gated.
time  -> r11_color_correct_time.json: one 30-frame 375 x 1242 call, median of 20 runs after 3 warm-ups, with torch.cuda.Event
and as a host call with read-back; the numpy helper on one frame of the same host.
--once: a single 30-frame call and nothing else (for a kernel trace).
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def measure_error():
    import torch
    from outdoor_nerf_depth_amd import color_correct as P
    from tests import color_correct_reference as R
    dev = torch.device('cuda', 0)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    cases, worst, worst_ne = [], 0.0, 0.0
    dark = R.gained_pair(375, 1242, 9)
    for label, img, ref in R.well_conditioned_cases() + [('dark (reported only)', (dark[0] * np.float32(0.02)), dark[1])]:
        want, _, counts = R.color_correct(img, ref)
        got, got_u8, psnr, got_counts = P.color_correct(up(img), up(ref), True)
        sums, mag = R.normal_equations(img, ref)
        ne = float((np.abs(P.normal_equations(up(img), up(ref))[0] - sums) / np.maximum(mag, 1e-300)).max())
        err = float(np.abs(got[0] - want).max())
        n_diff, n_bad, n_near = R.byte_rule(got_u8[0], want)
        want_psnr = R.psnr_cc(want, ref, True)
        row = dict(case=label, shape=list(img.shape), rgb_cc_max_abs_err=err, normal_equations_rel_err=ne,
                   bytes_differing=n_diff, bytes_outside_rule=n_bad, helper_values_near_a_byte_edge=n_near,
                   psnr_cc=float(psnr[0]), psnr_cc_helper=want_psnr, mask_counts_equal=bool((got_counts[0] == counts).all()))
        print(json.dumps(row), flush=True)
        cases.append(row)
        if 'reported only' not in label:
            worst, worst_ne = max(worst, err), max(worst_ne, ne)
    return dict(what='libcolorcc_hip.so against tests/color_correct_reference.py (np.linalg.lstsq on the full matrix, float64)',
                device=torch.cuda.get_device_name(0), worst_rgb_cc_abs_err=worst, worst_normal_equations_rel_err=worst_ne,
                gate_rule='tests gate at 10 x worst, and never above 1e-8 (rgb_cc) / 1e-12 (normal equations)', cases=cases)


def split(n_frames=30, H=375, W=1242):
    import torch
    from tests import color_correct_reference as R
    dev = torch.device('cuda', 0)
    pairs = [R.gained_pair(H, W, 100 + (i % 3), noise=0.02) for i in range(3)]
    img = torch.from_numpy(np.stack([pairs[i % 3][0] for i in range(n_frames)])).to(dev)
    ref = torch.from_numpy(np.stack([pairs[i % 3][1] for i in range(n_frames)])).to(dev)
    return img, ref, pairs


def measure_time():
    import torch
    from outdoor_nerf_depth_amd import color_correct as P
    from tests import color_correct_reference as R
    img, ref, pairs = split()
    ev, host = [], []
    for i in range(23):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        pend = P.color_correct_async(img, ref)
        b.record()
        torch.cuda.synchronize()
        if i >= 3:
            ev.append(a.elapsed_time(b) * 1e-3)
        del pend
    for i in range(23):
        torch.cuda.synchronize()
        t = time.perf_counter()
        P.color_correct(img, ref)
        if i >= 3:
            host.append(time.perf_counter() - t)
    t = time.perf_counter()
    R.color_correct(*pairs[0])
    helper = time.perf_counter() - t
    n_bytes = 30 * 375 * 1242 * (5 * 3 * 13 + 15 + 27)       # 5 x 3 channel passes of 12 + 1 B, apply: 15 B read, 24 + 3 B written
    return dict(what='colorcc_correct, one call for 30 frames of 375 x 1242', device=torch.cuda.get_device_name(0),
                event_seconds_median_of_20=float(np.median(ev)), event_seconds_min=float(np.min(ev)),
                host_call_with_readback_seconds_median_of_20=float(np.median(host)),
                numpy_helper_seconds_per_frame=helper, numpy_helper_host_cpus=len(os.sched_getaffinity(0)),
                bytes_moved_per_call=n_bytes, effective_GB_per_s=float(n_bytes / np.median(ev) / 1e9))


def main(argv=None):
    p = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    p.add_argument('--out_dir', default=os.path.join(ROOT, 'profiles'))
    p.add_argument('--skip_error', action='store_true')
    p.add_argument('--skip_time', action='store_true')
    p.add_argument('--once', action='store_true')
    args = p.parse_args(argv)
    if args.once:
        import torch
        from outdoor_nerf_depth_amd import color_correct as P
        img, ref, _ = split()
        print('psnr_cc', P.color_correct(img, ref)[2])
        return
    os.makedirs(args.out_dir, exist_ok=True)
    for skip, fn, name in ((args.skip_error, measure_error, 'r11_color_correct_error.json'),
                           (args.skip_time, measure_time, 'r11_color_correct_time.json')):
        if not skip:
            res = fn()
            with open(os.path.join(args.out_dir, name), 'w') as f:
                json.dump(res, f, indent=1)
                f.write('\n')
            print(json.dumps({k: v for k, v in res.items() if k != 'cases'}))


if __name__ == '__main__':
    main()

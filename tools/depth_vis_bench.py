#!/usr/bin/env python
"""Measure libdepthvis_hip.so on the device: its percentile error against the numpy helper and its time.

    python tools/depth_vis_bench.py [--out_dir D] [--skip_error] [--skip_time] [--once]

error -> depth_vis_error.json: weighted percentiles (0.5, 99.5) of frames with weights uniform in (0, 1] against
tests.depth_vis_reference.weighted_percentile: |device - helper|, relative, next to the bound of another summation order.
time  -> depth_vis_time.json: the five pictures of a 30-frame 375 x 1242 split (depth_vis.mip360_suite_async) and the two of a
NeRF++ split (minmax_colorize_async on 60 frames), median of 10 runs after 2 warm-ups, with torch.cuda.Event and as a host
call with read-back.
--once: a single suite call and nothing else (for a kernel trace).
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
    from outdoor_nerf_depth_amd import depth_vis as P
    from tests import depth_vis_reference as R
    dev = torch.device('cuda', 0)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    u = 2.0 ** -53
    cases = []
    for n in (4097, 96 * 129, 375 * 1242, 3 * 375 * 1242):
        rs = np.random.RandomState(n % 9973)
        v = rs.uniform(0.1, 30.0, (1, n)).astype(np.float32)
        w = (1.0 - rs.rand(1, n)).astype(np.float32)
        got = P.weighted_percentiles(up(v), up(w), R.SUITE_PS)[0]
        ref, j, wj, xs, cw = R.weighted_percentile(v[0], w[0], R.SUITE_PS)
        gate = [2 * n * u * cw[-1] / wj[k] * (xs[j[k] + 1] - xs[j[k]]) + 4 * u * abs(ref[k]) for k in range(2)]
        row = dict(n=n, device=[float(x) for x in got], helper=[float(x) for x in ref],
                   rel_err=[float(abs(got[k] - ref[k]) / abs(ref[k])) for k in range(2)], order_bound=[float(g) for g in gate],
                   abs_err=[float(abs(got[k] - ref[k])) for k in range(2)])
        print(json.dumps(row), flush=True)
        cases.append(row)
    return dict(what='depthvis_percentiles against tests/depth_vis_reference.py (stable argsort, cumsum, np.interp in float64)',
                device=torch.cuda.get_device_name(0), worst_rel_err=max(max(c['rel_err']) for c in cases), cases=cases)


def split(n_frames=30, H=375, W=1242):
    import torch
    dev = torch.device('cuda', 0)
    rs = np.random.RandomState(0)
    f = lambda lo, hi, *c: torch.from_numpy(rs.uniform(lo, hi, (3, H, W) + c).astype(np.float32)).to(dev).repeat(
        (n_frames // 3,) + (1,) * (2 + len(c)))
    med = f(0.5, 60.0)
    return dict(rgb=f(0, 1, 3), acc=f(0, 1), distance_mean=f(0.5, 60.0), distance_median=med, distance_p5=med * 0.8,
                distance_p95=med * 1.3, origins=f(-1, 1, 3), directions=f(-1, 1, 3))


def _timed(fn, runs=10, warm=2):
    import torch
    ev, host = [], []
    for i in range(runs + warm):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        pend = fn()
        b.record()
        torch.cuda.synchronize()
        if i >= warm:
            ev.append(a.elapsed_time(b) * 1e-3)
        del pend
    for i in range(runs + warm):
        torch.cuda.synchronize()
        t = time.perf_counter()
        fn().get()
        if i >= warm:
            host.append(time.perf_counter() - t)
    return dict(event_seconds_median=float(np.median(ev)), event_seconds_min=float(np.min(ev)),
                host_call_with_readback_seconds_median=float(np.median(host)))


def measure_time():
    import torch
    from outdoor_nerf_depth_amd import depth_vis as P
    s = split()
    suite = _timed(lambda: P.mip360_suite_async(**s))
    depth = torch.cat([s['distance_mean'], s['distance_median']])
    nerfpp = _timed(lambda: P.minmax_colorize_async(depth))
    return dict(what='one call per split of 30 frames of 375 x 1242: the five MipNeRF-360 pictures; fg and bg depth of NeRF++',
                device=torch.cuda.get_device_name(0), mip360_suite=suite, nerfpp_minmax_60_frames=nerfpp,
                bar_seconds='0.29 (rendering one frame of the split, DESIGN.md 9.5)')


def main(argv=None):
    p = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    p.add_argument('--out_dir', default=os.path.join(ROOT, 'profiles'))
    p.add_argument('--skip_error', action='store_true')
    p.add_argument('--skip_time', action='store_true')
    p.add_argument('--once', action='store_true')
    args = p.parse_args(argv)
    if args.once:
        from outdoor_nerf_depth_amd import depth_vis as P
        print('lohi_mean', P.mip360_suite_async(**split()).get()['lohi_mean'][:3])
        return
    os.makedirs(args.out_dir, exist_ok=True)
    for skip, fn, name in ((args.skip_error, measure_error, 'depth_vis_error.json'),
                           (args.skip_time, measure_time, 'depth_vis_time.json')):
        if not skip:
            res = fn()
            with open(os.path.join(args.out_dir, name), 'w') as f:
                json.dump(res, f, indent=1)
                f.write('\n')
            print(json.dumps({k: v for k, v in res.items() if k != 'cases'}))


if __name__ == '__main__':
    main()

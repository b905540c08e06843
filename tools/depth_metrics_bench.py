#!/usr/bin/env python
"""Measure libdepthmetrics_hip.so on the device: the time of a split's depth columns next to the host path.

    python tools/depth_metrics_bench.py [--out_dir D] [--once]

-> depth_metrics_time.json: the nine metrics of a 30-frame 375 x 1242 split (depth_metrics.depth_metrics_async), with and without
the error map, median of 10 runs after 2 warm-ups, with torch.cuda.Event and as a host call with read-back; the bytes the call
moves (8 B per pixel read, 4 B written with the map) over the event time; and, in the same run, the present host path: the two
numpy functions of the evaluators over the same frames, their device-to-host copy included.  The device's numbers are also checked
against tests/depth_metrics_reference.py on the split's first frame.
--once: a single call and nothing else (for a kernel trace).
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SCALE = 0.0137
HBM_BYTES_PER_SECOND = 6.3e12     # the streaming-read rate the floor below is quoted against


def split(n_frames=30, H=375, W=1242):
    """(pred, gt) device float32 [F, H, W]: the seeded frames of the tests at the split's size, three distinct frames repeated"""
    import torch
    from tests import depth_metrics_reference as R
    pred, gt = R.seeded_frames((H, W), SCALE, seed=0, n_frames=3)
    dev = torch.device('cuda', 0)
    up = lambda a: torch.from_numpy(a).to(dev).repeat(n_frames // 3, 1, 1).contiguous()
    return up(pred), up(gt)


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


def _host_path(pred, gt, runs=10, warm=2):
    """today's host path over the same frames: copy every rendered frame back, then the evaluators' numpy function"""
    import torch
    from outdoor_nerf_depth_amd import eval_outputs
    gt_host = gt.cpu().numpy()
    times = []
    for i in range(runs + warm):
        torch.cuda.synchronize()
        t = time.perf_counter()
        for f in range(pred.shape[0]):
            eval_outputs.depth_errors(pred[f].cpu().numpy(), gt_host[f], SCALE)
        if i >= warm:
            times.append(time.perf_counter() - t)
    return {'eval_outputs.depth_errors': dict(seconds_median=float(np.median(times)), seconds_min=float(np.min(times)))}


def measure_time():
    import torch
    from outdoor_nerf_depth_amd import depth_metrics as P
    from tests import depth_metrics_reference as R
    pred, gt = split()
    F, H, W = pred.shape
    got = P.depth_metrics(pred[:1], gt[:1], SCALE, err_map=True)
    ref, err_map, _ = R.split_metrics(pred[:1].cpu().numpy(), gt[:1].cpu().numpy(), SCALE)
    R.assert_rows_close(got, ref, 'first frame')
    np.testing.assert_array_equal(got['err_map'], err_map)
    plain = _timed(lambda: P.depth_metrics_async(pred, gt, SCALE))
    with_map = _timed(lambda: P.depth_metrics_async(pred, gt, SCALE, err_map=True))
    for res, per_pixel in ((plain, 8), (with_map, 12)):
        res['bytes'] = per_pixel * F * H * W
        res['hbm_floor_seconds'] = res['bytes'] / HBM_BYTES_PER_SECOND
        res['bytes_per_second'] = res['bytes'] / res['event_seconds_median']
    host = _host_path(pred, gt)
    slowest = max(v['seconds_median'] for v in host.values())
    return dict(what='the nine depth metrics of one split of %d frames of %d x %d in one call; bytes = 8 per pixel read (+ 4 written '
                     'with the error map)' % (F, H, W),
                device=torch.cuda.get_device_name(0), metrics=plain, metrics_and_err_map=with_map, host_path=host,
                host_over_device_call_with_readback=slowest / plain['host_call_with_readback_seconds_median'],
                bar_seconds='0.29 MipNeRF-360, 0.20 NeRF++ (rendering one frame of the split, DESIGN.md 9.5)')


def main(argv=None):
    p = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    p.add_argument('--out_dir', default=os.path.join(ROOT, 'profiles'))
    p.add_argument('--once', action='store_true')
    args = p.parse_args(argv)
    if args.once:
        from outdoor_nerf_depth_amd import depth_metrics as P
        pred, gt = split()
        print('rmse', P.depth_metrics_async(pred, gt, SCALE, err_map=True).get()['rmse'][:3])
        return
    os.makedirs(args.out_dir, exist_ok=True)
    res = measure_time()
    with open(os.path.join(args.out_dir, 'depth_metrics_time.json'), 'w') as f:
        json.dump(res, f, indent=1)
        f.write('\n')
    print(json.dumps(res))


if __name__ == '__main__':
    main()

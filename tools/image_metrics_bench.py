#!/usr/bin/env python
"""Time one image_metrics call on a KITTI-sized test split (30 frames of 375 x 1242) and set it beside the numpy statement
of the same metric (tests/ssim_reference.py) on the same frames and host.

    python tools/image_metrics_bench.py [--frames 30] [--hw 375,1242] [--out profiles/image_metrics_time.json]

Device time: torch.cuda.Event around the call's two kernels (inputs already on the device), median of --runs runs after
--warmup warm-ups.  The call with its read-back (what a CLI pays) is timed with a host clock around image_metrics().
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def main(argv=None):
    p = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    p.add_argument('--frames', type=int, default=30)
    p.add_argument('--hw', type=str, default='375,1242')
    p.add_argument('--runs', type=int, default=20)
    p.add_argument('--warmup', type=int, default=3)
    p.add_argument('--out', type=str, default=None)
    args = p.parse_args(argv)
    import torch
    from outdoor_nerf_depth_amd.image_metrics import image_metrics, image_metrics_async
    from tests import ssim_reference as R
    if not torch.cuda.is_available():
        raise SystemExit('image_metrics_bench needs a GPU')
    H, W = (int(v) for v in args.hw.split(','))
    rs = np.random.RandomState(0)
    gt = rs.randint(0, 256, (args.frames, H, W, 3)).astype(np.uint8)
    pred = np.clip(np.rint(gt + rs.normal(0, 12.0, gt.shape)), 0, 255).astype(np.uint8)
    dev = torch.device('cuda:0')
    g, q = torch.from_numpy(gt).to(dev), torch.from_numpy(pred).to(dev)
    for _ in range(args.warmup):
        image_metrics(g, q)
    dev_ms, call_ms = [], []
    for _ in range(args.runs):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        pending = image_metrics_async(g, q)
        e1.record()
        e1.synchronize()
        dev_ms.append(e0.elapsed_time(e1))
        pending.get()
    for _ in range(args.runs):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ssim, psnr8 = image_metrics(g, q)
        call_ms.append(1e3 * (time.perf_counter() - t0))
    t0 = time.perf_counter()
    want_s, want_p = R.image_metrics(gt, pred)
    numpy_s = time.perf_counter() - t0
    res = {
        'what': 'one image_metrics call (nerfpp_image_metrics_u8: SSIM + 8-bit PSNR) on %d frames of %d x %d x 3 uint8' % (args.frames, H, W),
        'device': torch.cuda.get_device_name(0),
        'timer': 'torch.cuda.Event around the call, median of %d runs after %d warm-ups' % (args.runs, args.warmup),
        'device_ms_median': float(np.median(dev_ms)), 'device_ms_min': float(np.min(dev_ms)), 'device_ms_max': float(np.max(dev_ms)),
        'call_with_readback_ms_median': float(np.median(call_ms)),
        'numpy_helper_s': numpy_s, 'numpy_helper_s_per_frame': numpy_s / args.frames,
        'bytes_read': int(2 * gt.size),
        'max_abs_ssim_diff_vs_helper': float(np.abs(ssim - want_s).max()),
        'max_rel_psnr8_diff_vs_helper': float(np.abs(psnr8 / want_p - 1).max()),
    }
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, 'w') as f:
            f.write(json.dumps(res, indent=1) + '\n')


if __name__ == '__main__':
    main()

#!/usr/bin/env python
"""Time one lpips_u8 call (liblpips_hip.so) on a KITTI-sized test split (30 pairs of 375 x 1242) and set it beside the
float32 torch-CPU statement of the metric (tests/lpips_reference.py: what the reference's utils/eval.py pays) on the same host.

    python tools/lpips_bench.py [--pairs 30] [--hw 375,1242] [--cpu_pairs 2] [--out profiles/lpips_time.json]

Device time: torch.cuda.Event around the call (inputs, packed weights and workspace already on the device), median of --runs
runs after --warmup warm-ups.  The CPU statement is timed on --cpu_pairs pairs and scaled to --pairs (it is linear in them).
Weights are random (tests/lpips_reference.random_weights): the time does not depend on their values.
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

PEAK_F32_MFMA_TFLOPS = 157.3          # v_mfma_f32_32x32x2_f32 on MI355X: 64 FLOP / clk / SIMD


def conv_flop(H, W):
    """multiply-adds x 2 of the 13 convolutions on one H x W image"""
    from tests.lpips_reference import CONV_SHAPES, TAP_AFTER
    total, h, w = 0, H, W
    for i, (cin, cout) in enumerate(CONV_SHAPES):
        total += 2 * 9 * cin * cout * h * w
        if i in TAP_AFTER[:-1]:
            h, w = h // 2, w // 2
    return total


def main(argv=None):
    p = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    p.add_argument('--pairs', type=int, default=30)
    p.add_argument('--hw', type=str, default='375,1242')
    p.add_argument('--runs', type=int, default=20)
    p.add_argument('--warmup', type=int, default=3)
    p.add_argument('--cpu_pairs', type=int, default=2)
    p.add_argument('--out', type=str, default=None)
    args = p.parse_args(argv)
    import torch
    from outdoor_nerf_depth_amd import lpips as P
    from tests import lpips_reference as R
    if not torch.cuda.is_available():
        raise SystemExit('lpips_bench needs a GPU')
    H, W = (int(v) for v in args.hw.split(','))
    rs = np.random.RandomState(0)
    gt = rs.randint(0, 256, (args.pairs, H, W, 3)).astype(np.uint8)
    pred = np.clip(np.rint(gt + rs.normal(0, 12.0, gt.shape)), 0, 255).astype(np.uint8)
    dev = torch.device('cuda:0')
    ref_w = R.random_weights(R.WEIGHT_SEED, R.LIN_SCALE)
    weights = P.Weights(ref_w)
    g, q = torch.from_numpy(gt).to(dev), torch.from_numpy(pred).to(dev)
    packed = weights.packed(dev)
    ws = torch.empty(P.workspace_bytes(args.pairs, H, W) // 8, dtype=torch.float64, device=dev)
    out = torch.empty((args.pairs, 6), dtype=torch.float64, device=dev)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    call = lambda: P.check(P.lib().lpips_u8(stream, args.pairs, H, W, g.data_ptr(), q.data_ptr(), packed.data_ptr(), ws.data_ptr(),
                                            out.data_ptr()), 'lpips_u8')
    for _ in range(args.warmup):
        call()
    torch.cuda.synchronize()
    dev_ms = []
    for _ in range(args.runs):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        call()
        e1.record()
        e1.synchronize()
        dev_ms.append(e0.elapsed_time(e1))
    got = out.cpu().numpy()
    n_cpu = max(1, min(args.cpu_pairs, args.pairs))
    t0 = time.perf_counter()
    cpu_t, _ = R.lpips(gt[:n_cpu], pred[:n_cpu], ref_w, torch.float32)
    cpu_s = time.perf_counter() - t0
    flop = 2 * args.pairs * conv_flop(H, W)
    med = float(np.median(dev_ms))
    res = {
        'what': 'one lpips_u8 call (LPIPS v0.1, VGG-16, float32 MFMA) on %d pairs of %d x %d x 3 uint8' % (args.pairs, H, W),
        'device': torch.cuda.get_device_name(0),
        'timer': 'torch.cuda.Event around the call, median of %d runs after %d warm-ups' % (args.runs, args.warmup),
        'device_ms_median': med, 'device_ms_min': float(np.min(dev_ms)), 'device_ms_max': float(np.max(dev_ms)),
        'device_ms_per_pair': med / args.pairs,
        'convolution_tflop': flop / 1e12,
        'achieved_tflops': flop / 1e12 / (med / 1e3),
        'fraction_of_f32_mfma_peak': flop / 1e12 / (med / 1e3) / PEAK_F32_MFMA_TFLOPS,
        'f32_mfma_peak_tflops': PEAK_F32_MFMA_TFLOPS,
        'workspace_bytes': int(ws.numel() * 8),
        'cpu_float32_reference_s_measured': cpu_s, 'cpu_float32_reference_pairs_measured': n_cpu,
        'cpu_float32_reference_s_per_pair': cpu_s / n_cpu,
        'cpu_float32_reference_s_scaled_to_all_pairs': cpu_s / n_cpu * args.pairs,
        'cpu_threads': torch.get_num_threads(),
        'max_abs_total_diff_vs_cpu_float32': float(np.abs(got[:n_cpu, 5] - cpu_t).max()),
    }
    print(json.dumps(res))
    if args.out:
        with open(args.out, 'w') as f:
            f.write(json.dumps(res, indent=1) + '\n')


if __name__ == '__main__':
    main()

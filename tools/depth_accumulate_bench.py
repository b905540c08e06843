"""Time one accumulation of depth priors from neighbouring frames (depthacc_accumulate) at the size of the 295-frame KITTI sequence on
one GPU, and the 'mse' training step of both paths against another checkout of this package (the parent commit, built in its own
tree).

    python tools/depth_accumulate_bench.py [--parent /path/to/parent/checkout] [--rounds 3] [--calls 20] [--out profiles/depth_accumulate_time.json]
    python tools/depth_accumulate_bench.py --worker call       # the timed calls in this process

The call: 295 frames of 375 x 1242, V = 4 nearest frames, origin and rows asked for, on the analytic plane scene of
tools/depth_consistency_bench.py, once with a 5 % prior (a LiDAR sweep's coverage; a seeded uniform mask) and once with the dense one.
Warm-up calls, then `calls` timed ones, each between two device events; the median, the extremes and every time are reported.  Two
windows: the library call by itself (cameras and neighbour lists uploaded before, outputs reused: the fill, the scatter, the resolve
and the row sum, nothing of the host) and the binding's accumulate_async as a trainer calls it (host validation of the cameras and
lists, two small uploads, allocation, the launches).  The call is once per run: the times are reported, not gated.  Next to them the
compulsory traffic -- every source frame read once per view (4 V bytes per pixel), the z-buffer written once and read once (8 + 8),
the frame's own depth read by the resolve pass (4) and depth_out and origin written (4 + 1) -- and the ratio of the launches' time
to that traffic at the HBM rate this project uses as achievable, 6.2 TB/s.  The atomic traffic: at most one 8-byte
global_atomic_umin_x2 per valid source pixel and view (fewer: a projection that leaves the target, or lands on a pixel with a
measurement of its own, issues none), set against the chip-wide rate of float atomics as 8-byte requests.  A dense prior issues no atomic at
all: every target pixel has its own measurement and the scatter drops the projection after one 4-byte gather of the target's depth.

The training steps: tools/depth_gnll_bench.py's workers ('mse' only), this checkout and --parent in alternating fresh processes (the
one that goes first alternates from round to round); the parent's runs against each other are the A/A spread of the box.  Without
the load-time flags a step makes exactly the calls it made, so 'mse' of this code belongs inside that spread.  Prints one JSON line
(and writes it to --out).
"""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from depth_consistency_bench import F, H, W, K, FOCAL, HBM_ACHIEVABLE, plane_scene, timed      # noqa: E402

ATOMIC_RATE = 1.3e12 / 4 * 8      # bytes / s: the 334 G float atomic adds per second this project measured, as 8-byte requests


def worker_call(calls, warmup):
    import torch
    from outdoor_nerf_depth_amd import depth_accumulate as DA
    dev = torch.device('cuda:0')
    dense, cams, nbr = plane_scene(dev)
    gen = torch.Generator(device=dev)
    gen.manual_seed(2)
    sparse = torch.where(torch.rand(dense.shape, generator=gen, device=dev) < 0.05, dense, torch.zeros_like(dense))
    cams_d, nbr_d, n_views = DA.upload(cams, nbr, dev)
    prm = DA.check_params()
    res = {}
    for name, depth in (('sparse_5_percent', sparse), ('dense', dense)):
        # the launches by themselves: cameras and lists on the device already, the outputs of the first call written again
        first = DA.enqueue(depth, cams_d, nbr_d, n_views, prm, origin=True, src=False, rows=True)
        launches, last = timed(lambda: DA.enqueue(depth, cams_d, nbr_d, n_views, prm, origin=True, src=False, rows=True, out=first.tensors),
                               calls, warmup)
        out = torch.empty_like(depth)
        binding, _ = timed(lambda: DA.accumulate_async(depth, cams, nbr, origin=True, src=False, rows=True, depth_out=out), calls, warmup)
        rows = last.tensors['rows'].sum(0).cpu().numpy()
        res[name] = {'launches_ms': launches, 'binding_ms': binding, 'totals': dict(zip(DA.ROW_NAMES, (int(v) for v in rows)))}
        del first, last, out
    print(json.dumps(res))


def main():
    p = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    p.add_argument('--worker', default=None, help="'call': the timed calls in this process")
    p.add_argument('--parent', default=None, help='another checkout (built) whose mse training steps alternate with this one\'s')
    p.add_argument('--rounds', type=int, default=3)
    p.add_argument('--calls', type=int, default=20)
    p.add_argument('--warmup', type=int, default=3)
    p.add_argument('--steps', type=int, default=60)
    p.add_argument('--timeout', type=int, default=300, help='seconds per worker process')
    p.add_argument('--out', default=None, help='also write the JSON result to this file')
    args = p.parse_args()
    sys.path.insert(0, os.path.dirname(HERE))
    if args.worker == 'call':
        return worker_call(args.calls, args.warmup)

    def child(cmd):
        out = subprocess.run([sys.executable] + cmd, capture_output=True, text=True, timeout=args.timeout)
        if out.returncode != 0:                               # (nothing more is started on the GPU after a failed run)
            sys.stderr.write(out.stdout[-2000:] + out.stderr[-2000:])
            sys.exit(out.returncode)
        return json.loads(out.stdout.strip().splitlines()[-1])

    got = child([os.path.abspath(__file__), '--worker', 'call', '--calls', str(args.calls), '--warmup', str(args.warmup)])
    pixels = F * H * W
    per_pixel = {'read': 4 * K + 4 + 8, 'written': 8 + 4 + 1}
    traffic = (per_pixel['read'] + per_pixel['written']) * pixels
    floor_ms = 1e3 * traffic / HBM_ACHIEVABLE
    res = {'call': {'frames': F, 'height': H, 'width': W, 'views': K, 'focal': FOCAL, 'calls': args.calls, 'warmup': args.warmup,
                    'what': 'launches_ms: the library call alone (cameras and lists on the device, outputs reused); binding_ms: '
                            'depth_accumulate.accumulate_async with its host validation, uploads and allocation',
                    'compulsory_bytes': traffic, 'compulsory_bytes_per_pixel': per_pixel,
                    'hbm_achievable_bytes_per_s': HBM_ACHIEVABLE, 'ms_of_the_compulsory_traffic_at_that_rate': floor_ms, 'priors': {}}}
    for name, g in got.items():
        ms, whole = g['launches_ms'], g['binding_ms']
        med = float(np.median(ms))
        own = g['totals']['n_own']
        atomics_at_most = 0 if own == pixels else own * K      # a dense prior: every projection meets a measured pixel and is dropped
        res['call']['priors'][name] = {
            'ms_median': med, 'ms_min': min(ms), 'ms_max': max(ms), 'ms': ms, 'binding_ms_median': float(np.median(whole)),
            'binding_ms_min': min(whole), 'binding_ms_max': max(whole), 'binding_ms': whole, 'totals': g['totals'],
            'time_over_the_compulsory_traffic': med / floor_ms,
            'atomics_at_most': atomics_at_most, 'ms_of_those_atomics_at_the_float_atomic_rate': 1e3 * atomics_at_most * 8 / ATOMIC_RATE,
            'gathered_target_depths_at_most': own * K}
    if args.parent:
        res['mse_step'] = {'steps': args.steps, 'rounds': args.rounds, 'paths': {}}
        for path in ('mip360', 'nerfpp'):
            runs = {'parent_mse': [], 'mse': []}
            for r in range(args.rounds):                      # (who goes first alternates: a process inherits the clocks the last one left)
                for name, root in (('parent_mse', args.parent), ('mse', os.path.dirname(HERE)))[::1 if r % 2 == 0 else -1]:
                    runs[name].append(child([os.path.join(HERE, 'depth_gnll_bench.py'), '--worker', path + ':mse', '--root', root,
                                             '--steps', str(args.steps), '--warmup', '5'])['ms_per_step'])
            med = {k: float(np.median(v)) for k, v in runs.items()}
            res['mse_step']['paths'][path] = {
                'ms_per_step_runs': runs, 'ms_per_step_median': med, 'mse_minus_parent_mse_ms': med['mse'] - med['parent_mse'],
                'parent_A_A_spread_ms': max(runs['parent_mse']) - min(runs['parent_mse']),
                'mse_inside_parent_spread': bool(min(runs['parent_mse']) <= med['mse'] <= max(runs['parent_mse']))}
    print(json.dumps(res))
    if args.out:
        with open(args.out, 'w') as f:
            f.write(json.dumps(res, indent=1) + '\n')
    return 0


if __name__ == '__main__':
    sys.exit(main())

"""Time the 4096-ray MipNeRF-360 training step with the per-ray depth losses ('kl_ray', 'urf_ray') against 'mse' on one GPU, and
'mse' against another checkout of this package (the parent commit, built in its own tree) in alternating fresh processes.

    python tools/mip360_depth_rays_bench.py [--parent /path/to/parent/checkout] [--rounds 3] [--steps 30] [--warmup 5] [--out x.json]
    python tools/mip360_depth_rays_bench.py --worker kl_ray        # one timing in this process

The workload is mip360.benchmark_step's: configs/360.gin shape (64 / 64 / 32 samples), synthetic rays, he_uniform weights, half of
the rays supervised, every step joined.  Each configuration runs `rounds` times, interleaved (parent mse, mse, kl_ray, urf_ray,
parent mse, ...), one process each; the parent's runs against each other are the A/A spread of the box.  Prints one JSON line (and
writes it to --out): ms per step of every run, medians, spreads, and the bytes the two launches of mip360_depth_loss_rays move
per step (weights + both tdist edges read, gradients read and written, for the three levels).
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))


def worker(kind, n_rays, steps, warmup, root):
    sys.path.insert(0, root)
    import torch
    from outdoor_nerf_depth_amd import mip360 as M
    d = torch.device('cuda:0')
    rs_p = np.random.RandomState(0)
    he = lambda shapes: [(rs_p.uniform(-np.sqrt(6.0 / i), np.sqrt(6.0 / i), (i, o)).astype(np.float32), np.zeros(o, np.float32))
                         for i, o in shapes]
    prop, nerf = he(M.mlp_shapes(M.PROP_CFG)), he(M.mlp_shapes(M.NERF_CFG))
    rs = np.random.RandomState(0)
    n = n_rays
    dirs = rs.randn(n, 3).astype(np.float32)
    dirs /= np.linalg.norm(dirs, axis=-1, keepdims=True)
    T = lambda x: torch.from_numpy(x).to(d)
    rays = dict(origins=T((rs.randn(n, 3) * 0.3).astype(np.float32)), directions=T(dirs), viewdirs=T(dirs.copy()),
                radii=T(np.full((n, 1), 2e-3, np.float32)), near=T(np.full((n, 1), 0.2, np.float32)),
                far=T(np.full((n, 1), 1e6, np.float32)))
    gt = T(rs.rand(n, 3).astype(np.float32))
    sup = T(np.where(rs.rand(n) < .5, rs.uniform(1, 6, n), 0).astype(np.float32))
    tr = M.Mip360Trainer(prop, nerf, d, depth_loss_type=kind, depth_sigma=0.3)
    for _ in range(warmup):
        tr.train_step(rays, gt, sup)
    tr.flush()
    torch.cuda.synchronize(d)
    t0 = time.perf_counter()
    for _ in range(steps):
        sc = tr.train_step(rays, gt, sup)
    tr.flush()
    torch.cuda.synchronize(d)
    ms = 1e3 * (time.perf_counter() - t0) / steps
    print(json.dumps({'depth_loss_type': kind, 'ms_per_step': ms, 'steps': steps, 'scalars': [float(v) for v in sc.cpu()]}))


def main():
    p = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    p.add_argument('--worker', default=None, help='time one configuration in this process: mse, kl_ray or urf_ray')
    p.add_argument('--root', default=os.path.dirname(HERE), help='checkout whose package the worker imports')
    p.add_argument('--parent', default=None, help='another checkout (built) to alternate with')
    p.add_argument('--n_rays', type=int, default=4096)
    p.add_argument('--rounds', type=int, default=3)
    p.add_argument('--steps', type=int, default=30)
    p.add_argument('--warmup', type=int, default=5)
    p.add_argument('--timeout', type=int, default=180, help='seconds per worker process')
    p.add_argument('--out', default=None, help='also write the JSON result to this file')
    args = p.parse_args()
    if args.worker is not None:
        return worker(args.worker, args.n_rays, args.steps, args.warmup, args.root)
    configs = [('mse', 'mse', args.root), ('kl_ray', 'kl_ray', args.root), ('urf_ray', 'urf_ray', args.root)]
    if args.parent:
        configs = [('parent_mse', 'mse', args.parent)] + configs
    runs = {name: [] for name, _, _ in configs}
    for _ in range(args.rounds):
        for name, kind, root in configs:
            cmd = [sys.executable, os.path.abspath(__file__), '--worker', kind, '--root', root, '--n_rays', str(args.n_rays),
                   '--steps', str(args.steps), '--warmup', str(args.warmup)]
            out = subprocess.run(cmd, capture_output=True, text=True, timeout=args.timeout)
            if out.returncode != 0:                        # (nothing more is started on the GPU after a failed run)
                sys.stderr.write(out.stdout[-2000:] + out.stderr[-2000:])
                return out.returncode
            runs[name].append(json.loads(out.stdout.strip().splitlines()[-1])['ms_per_step'])
    med = {k: float(np.median(v)) for k, v in runs.items()}
    n, samples = args.n_rays, (64, 64, 32)
    res = {'workload': 'MipNeRF-360 configs/360.gin train step, %d rays, synthetic, half of the rays supervised, joined updates' % n,
           'steps': args.steps, 'ms_per_step_runs': runs, 'ms_per_step_median': med,
           'spread_ms': {k: float(max(v) - min(v)) for k, v in runs.items()},
           'kl_ray_minus_mse_ms': med['kl_ray'] - med['mse'], 'urf_ray_minus_mse_ms': med['urf_ray'] - med['mse'],
           # per (ray, level): S weights + (S + 1) edges read, S gradients read + written, one workspace float written + read
           'depth_loss_rays_bytes_per_step': int(sum(n * 4 * (4 * S + 3) for S in samples))}
    if args.parent:
        res['mse_minus_parent_mse_ms'] = med['mse'] - med['parent_mse']
        res['parent_A_A_spread_ms'] = res['spread_ms']['parent_mse']
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, 'w') as f:
            f.write(json.dumps(res, indent=1) + '\n')
    return 0


if __name__ == '__main__':
    sys.exit(main())

"""Time the 4096-ray MipNeRF-360 training step with and without per-image appearance embeddings (GLO) on one GPU, and
against another checkout of this package (the parent commit, built in its own tree) in alternating fresh processes.

    python tools/mip360_glo_bench.py [--parent /path/to/parent/checkout] [--rounds 3] [--steps 30] [--warmup 5]
    python tools/mip360_glo_bench.py --worker 4          # one timing in this process: G = 4 (or 0; -1: no GLO arguments at all)

The workload is mip360.benchmark_step's: configs/360.gin shape, synthetic rays, he_uniform weights, every step joined.  With
G > 0 every ray carries a frame index in [0, 100) and the table has 1000 rows (upstream's default).  Each configuration runs
`rounds` times, interleaved (parent, G=0, G=4, parent, ...), one process each; the parent's runs against each other are the
A/A spread of the box.  Prints one JSON line: ms per step of every run, medians, and the stage-1 traffic of
mip360_glo_backward (n_rays x 32 samples x 128 bf16) for turning a profiled kernel time into bytes/s.
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))


def worker(G, n_rays, steps, warmup, root):
    sys.path.insert(0, root)
    import torch
    from outdoor_nerf_depth_amd import mip360 as M
    d = torch.device('cuda:0')
    rs_p = np.random.RandomState(0)
    he = lambda shapes: [(rs_p.uniform(-np.sqrt(6.0 / i), np.sqrt(6.0 / i), (i, o)).astype(np.float32), np.zeros(o, np.float32))
                         for i, o in shapes]
    prop = he(M.mlp_shapes(M.PROP_CFG))
    nerf = he(M.mlp_shapes(M.NERF_CFG, G) if G > 0 else M.mlp_shapes(M.NERF_CFG))
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
    kw, step_kw = {}, {}
    if G >= 0:
        kw = dict(num_glo_features=G, num_glo_embeddings=1000)
    if G > 0:
        step_kw = dict(cam_idx=T(rs.randint(0, 100, n).astype(np.int32)))
    tr = M.Mip360Trainer(prop, nerf, d, **kw)
    for _ in range(warmup):
        tr.train_step(rays, gt, sup, **step_kw)
    tr.flush()
    torch.cuda.synchronize(d)
    t0 = time.perf_counter()
    for _ in range(steps):
        tr.train_step(rays, gt, sup, **step_kw)
    tr.flush()
    torch.cuda.synchronize(d)
    print(json.dumps({'G': G, 'ms_per_step': 1e3 * (time.perf_counter() - t0) / steps, 'steps': steps}))


def main():
    p = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    p.add_argument('--worker', type=int, default=None, help='time one configuration in this process: G = 0..4, or -1 for a trainer built without GLO arguments')
    p.add_argument('--root', default=os.path.dirname(HERE), help='checkout whose package the worker imports')
    p.add_argument('--parent', default=None, help='another checkout (built) to alternate with')
    p.add_argument('--n_rays', type=int, default=4096)
    p.add_argument('--rounds', type=int, default=3)
    p.add_argument('--steps', type=int, default=30)
    p.add_argument('--warmup', type=int, default=5)
    p.add_argument('--timeout', type=int, default=180, help='seconds per worker process')
    args = p.parse_args()
    if args.worker is not None:
        return worker(args.worker, args.n_rays, args.steps, args.warmup, args.root)
    configs = [('G0', 0, args.root), ('G4', 4, args.root)]
    if args.parent:
        configs = [('parent', -1, args.parent)] + configs
    runs = {name: [] for name, _, _ in configs}
    for _ in range(args.rounds):
        for name, G, root in configs:
            cmd = [sys.executable, os.path.abspath(__file__), '--worker', str(G), '--root', root, '--n_rays', str(args.n_rays),
                   '--steps', str(args.steps), '--warmup', str(args.warmup)]
            out = subprocess.run(cmd, capture_output=True, text=True, timeout=args.timeout)
            if out.returncode != 0:                        # (nothing more is started on the GPU after a failed run)
                sys.stderr.write(out.stdout[-2000:] + out.stderr[-2000:])
                return out.returncode
            runs[name].append(json.loads(out.stdout.strip().splitlines()[-1])['ms_per_step'])
    med = {k: float(np.median(v)) for k, v in runs.items()}
    res = {'workload': 'MipNeRF-360 configs/360.gin train step, %d rays, synthetic, joined updates' % args.n_rays, 'steps': args.steps,
           'ms_per_step_runs': runs, 'ms_per_step_median': med,
           'spread_ms': {k: float(max(v) - min(v)) for k, v in runs.items()},
           'G4_over_G0': med['G4'] / med['G0'],
           'glo_backward_stage1_bytes': args.n_rays * 32 * 128 * 2}
    if args.parent:
        res['G0_over_parent'] = med['G0'] / med['parent']
    print(json.dumps(res))
    return 0


if __name__ == '__main__':
    sys.exit(main())

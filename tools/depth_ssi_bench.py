"""Time the two training steps with the scale-and-shift-invariant depth loss ('ssi') against 'mse' on one GPU, and 'mse' against
another checkout of this package (the parent commit, built in its own tree) in alternating fresh processes.

    python tools/depth_ssi_bench.py [--parent /path/to/parent/checkout] [--rounds 3] [--steps 30] [--warmup 5] [--out profiles/depth_ssi_time.json]
    python tools/depth_ssi_bench.py --worker mip360:ssi          # one timing in this process (mip360 | nerfpp : mse | ssi)

Workloads: the MipNeRF-360 step of configs/360.gin (4096 rays, 64 / 64 / 32 samples, synthetic rays over 280 frames, he_uniform
weights, half of the rays supervised, every step joined) and the NeRF++ step (1024 rays of one synthetic frame, 64 + 128 samples,
bf16).  Each configuration runs `rounds` times, interleaved (parent mse, mse, ssi, parent mse, ...), one process each; the parent's
runs against each other are the A/A spread of the box.  The only gate: 'mse' of this code stays inside that spread (the step makes
no call the parent does not make); the exit code is 2 when it does not.  Prints one JSON line (and writes it to --out): ms per
step of every run, medians, spreads, and the bytes the first launch of depthssi_levels reads per step (every group's workgroup
reads the whole batch: G * n * 12 bytes per level, from L2).
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
MIP360_FRAMES = 280
WORKLOADS = {'mip360': 4096, 'nerfpp': 1024}


def mip360_step(kind, n, root):
    import torch
    from outdoor_nerf_depth_amd import mip360 as M
    d = torch.device('cuda:0')
    rs_p = np.random.RandomState(0)
    he = lambda shapes: [(rs_p.uniform(-np.sqrt(6.0 / i), np.sqrt(6.0 / i), (i, o)).astype(np.float32), np.zeros(o, np.float32))
                         for i, o in shapes]
    prop, nerf = he(M.mlp_shapes(M.PROP_CFG)), he(M.mlp_shapes(M.NERF_CFG))
    rs = np.random.RandomState(0)
    dirs = rs.randn(n, 3).astype(np.float32)
    dirs /= np.linalg.norm(dirs, axis=-1, keepdims=True)
    T = lambda x: torch.from_numpy(x).to(d)
    rays = dict(origins=T((rs.randn(n, 3) * 0.3).astype(np.float32)), directions=T(dirs), viewdirs=T(dirs.copy()),
                radii=T(np.full((n, 1), 2e-3, np.float32)), near=T(np.full((n, 1), 0.2, np.float32)),
                far=T(np.full((n, 1), 1e6, np.float32)))
    gt = T(rs.rand(n, 3).astype(np.float32))
    sup = T(np.where(rs.rand(n) < .5, rs.uniform(1, 6, n), 0).astype(np.float32))
    kw, step_kw = {}, {}
    if kind == 'ssi':
        kw = dict(depth_ssi_groups=MIP360_FRAMES)
        step_kw = dict(cam_idx=T(rs.randint(0, MIP360_FRAMES, n).astype(np.int32)))
    tr = M.Mip360Trainer(prop, nerf, d, depth_loss_type=kind, **kw)
    return lambda: tr.train_step(rays, gt, sup, **step_kw), tr.flush


def nerfpp_step(kind, n, root):
    import torch
    from outdoor_nerf_depth_amd import _lib as L
    from outdoor_nerf_depth_amd.synthetic import SyntheticKitti
    from outdoor_nerf_depth_amd.trainer import NerfppTrainer, batch_to_device
    d = torch.device('cuda:0')
    batch = batch_to_device(SyntheticKitti().random_batch(n, np.random.RandomState(0)), d)
    tr = NerfppTrainer(d, precision=L.PREC_BF16, use_depth=True, depth_loss_type=kind, lambda_depth=0.1)
    return lambda: tr.train_step(batch)[-1], tr.flush


def worker(what, steps, warmup, root):
    sys.path.insert(0, root)
    import torch
    path, kind = what.split(':')
    step, flush = {'mip360': mip360_step, 'nerfpp': nerfpp_step}[path](kind, WORKLOADS[path], root)
    for _ in range(warmup):
        step()
    flush()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        sc = step()
    flush()
    torch.cuda.synchronize()
    ms = 1e3 * (time.perf_counter() - t0) / steps
    print(json.dumps({'workload': what, 'ms_per_step': ms, 'steps': steps, 'scalars': [float(v) for v in sc.cpu()]}))


def main():
    p = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    p.add_argument('--worker', default=None, help='time one configuration in this process: mip360:mse, mip360:ssi, nerfpp:mse or nerfpp:ssi')
    p.add_argument('--root', default=os.path.dirname(HERE), help='checkout whose package the worker imports')
    p.add_argument('--parent', default=None, help='another checkout (built) to alternate with')
    p.add_argument('--rounds', type=int, default=3)
    p.add_argument('--steps', type=int, default=30)
    p.add_argument('--warmup', type=int, default=5)
    p.add_argument('--timeout', type=int, default=180, help='seconds per worker process')
    p.add_argument('--out', default=None, help='also write the JSON result to this file')
    args = p.parse_args()
    if args.worker is not None:
        return worker(args.worker, args.steps, args.warmup, args.root)
    res = {'steps': args.steps, 'rounds': args.rounds, 'paths': {}}
    outside = False
    for path, n in WORKLOADS.items():
        configs = [('mse', path + ':mse', args.root), ('ssi', path + ':ssi', args.root)]
        if args.parent:
            configs = [('parent_mse', path + ':mse', args.parent)] + configs
        runs = {name: [] for name, _, _ in configs}
        for _ in range(args.rounds):
            for name, what, root in configs:
                cmd = [sys.executable, os.path.abspath(__file__), '--worker', what, '--root', root, '--steps', str(args.steps), '--warmup',
                       str(args.warmup)]
                out = subprocess.run(cmd, capture_output=True, text=True, timeout=args.timeout)
                if out.returncode != 0:                    # (nothing more is started on the GPU after a failed run)
                    sys.stderr.write(out.stdout[-2000:] + out.stderr[-2000:])
                    return out.returncode
                runs[name].append(json.loads(out.stdout.strip().splitlines()[-1])['ms_per_step'])
        med = {k: float(np.median(v)) for k, v in runs.items()}
        levels, groups = (3, MIP360_FRAMES) if path == 'mip360' else (1, 1)      # (nerfpp: one call per cascade level, two per step)
        calls = 1 if path == 'mip360' else 2
        entry = {'rays': n, 'ms_per_step_runs': runs, 'ms_per_step_median': med,
                 'spread_ms': {k: float(max(v) - min(v)) for k, v in runs.items()}, 'ssi_minus_mse_ms': med['ssi'] - med['mse'],
                 'depthssi_first_launch_bytes_read_per_step': int(calls * levels * groups * n * 12)}
        if args.parent:
            lo, hi = min(runs['parent_mse']), max(runs['parent_mse'])
            entry['mse_minus_parent_mse_ms'] = med['mse'] - med['parent_mse']
            entry['parent_A_A_spread_ms'] = entry['spread_ms']['parent_mse']
            entry['mse_inside_parent_spread'] = bool(lo <= med['mse'] <= hi)
            outside = outside or not entry['mse_inside_parent_spread']
        res['paths'][path] = entry
    print(json.dumps(res))
    if args.out:
        with open(args.out, 'w') as f:
            f.write(json.dumps(res, indent=1) + '\n')
    return 2 if outside else 0


if __name__ == '__main__':
    sys.exit(main())

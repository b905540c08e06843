"""Time the NeRF++ training step with the line-of-sight term (ray_los.py) off and on, on one GPU, the step with it off
against another checkout of this package (the parent commit, built in its own tree) in alternating fresh processes, and the
library's two launches alone.

    python tools/ray_los_bench.py [--parent /path/to/parent/checkout] [--rounds 5] [--steps 30] [--warmup 5] [--out profiles/ray_los_time.json]
    python tools/ray_los_bench.py --worker off          # one timing in this process (off | on | launches)

Workload: the NeRF++ step of bench.py's shape (1024 rays of one synthetic frame, 64 + 128 samples, bf16) with the mse depth loss on
the scene's gt prior.  Each configuration runs `rounds` times, interleaved (parent off, off, on, parent off, ...), one process each;
the parent's runs against each other are the A/A spread of the box.  The only gate: the median of 'off' of this code lies inside the
[min, max] of the parent's own runs (the step makes no call the parent does not make); the exit code is 2 when it does not.
'launches' times raylos_level by itself at both levels' shapes, (1024, 64) and (1024, 192), on buffers that stay put, every ray
supervised.  Prints one JSON line (and writes it to --out): ms per step of every run, medians, spreads, microseconds per call of the
two launches, and the bytes their first launch moves per step (a supervised ray's rows of weights and positions are read once, the
entries of its row of the weight gradient that take a term are read and written: at most 16 bytes per sample, plus 32 per ray).
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
RAYS, LEVELS = 1024, (64, 192)
LAMBDA, SIGMA_M = 100.0, 4.0


def step_worker(kind, steps, warmup):
    import torch
    from outdoor_nerf_depth_amd import _lib as L
    from outdoor_nerf_depth_amd.synthetic import SyntheticKitti
    from outdoor_nerf_depth_amd.trainer import NerfppTrainer, batch_to_device
    d = torch.device('cuda:0')
    scene = SyntheticKitti()
    batch = batch_to_device(scene.random_batch(RAYS, np.random.RandomState(0)), d)
    kw = dict(lambda_los=LAMBDA, los_sigma=SIGMA_M) if kind == 'on' else {}
    tr = NerfppTrainer(d, precision=L.PREC_BF16, use_depth=True, depth_loss_type='mse', lambda_depth=0.1,
                       depth_scale=float(scene.depth_scale), **kw)
    for _ in range(warmup):
        tr.train_step(batch)
    tr.flush()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        sc = tr.train_step(batch)[-1]
    tr.flush()
    torch.cuda.synchronize()
    ms = 1e3 * (time.perf_counter() - t0) / steps
    return {'workload': kind, 'ms_per_step': ms, 'steps': steps, 'scalars': [float(v) for v in sc.cpu()]}


def launches_worker(steps, warmup):
    """raylos_level alone at each level's shape: HIP events around `steps` back-to-back calls"""
    import torch
    from outdoor_nerf_depth_amd import ray_los
    d = torch.device('cuda:0')
    rs = np.random.RandomState(0)
    out = {'workload': 'launches', 'steps': steps, 'us_per_call': {}}
    for S in LEVELS:
        z = torch.from_numpy(np.sort(rs.uniform(0.0, 1.0, (RAYS, S)), -1).astype(np.float32)).to(d)
        w = torch.from_numpy((rs.dirichlet(np.ones(S), RAYS) * 0.9).astype(np.float32)).to(d)
        hi = torch.full((RAYS,), 1.5, device=d)
        p = torch.from_numpy(rs.uniform(0.1, 0.9, RAYS).astype(np.float32)).to(d)
        sigma = torch.full((RAYS,), 2.0 / S, device=d)
        g, fold = torch.zeros(RAYS, S, device=d), torch.zeros(1, device=d)
        call = lambda: ray_los.ray_los(w, z, hi, p, sigma, LAMBDA, g, fold)
        for _ in range(warmup):
            call()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        for _ in range(steps):
            call()
        b.record()
        torch.cuda.synchronize()
        out['us_per_call']['%dx%d' % (RAYS, S)] = 1e3 * a.elapsed_time(b) / steps
    return out


def worker(what, steps, warmup, root):
    sys.path.insert(0, root)
    res = launches_worker(steps, warmup) if what == 'launches' else step_worker(what, steps, warmup)
    print(json.dumps(res))


def main():
    p = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    p.add_argument('--worker', default=None, help='time one configuration in this process: off, on or launches')
    p.add_argument('--root', default=os.path.dirname(HERE), help='checkout whose package the worker imports')
    p.add_argument('--parent', default=None, help='another checkout (built) to alternate with')
    p.add_argument('--rounds', type=int, default=5)
    p.add_argument('--steps', type=int, default=30)
    p.add_argument('--warmup', type=int, default=5)
    p.add_argument('--timeout', type=int, default=180, help='seconds per worker process')
    p.add_argument('--out', default=None, help='also write the JSON result to this file')
    args = p.parse_args()
    if args.worker is not None:
        return worker(args.worker, args.steps, args.warmup, args.root)

    def run(what, root):
        cmd = [sys.executable, os.path.abspath(__file__), '--worker', what, '--root', root, '--steps', str(args.steps), '--warmup',
               str(args.warmup)]
        out = subprocess.run(cmd, capture_output=True, text=True, timeout=args.timeout)
        if out.returncode != 0:                            # (nothing more is started on the GPU after a failed run)
            sys.stderr.write(out.stdout[-2000:] + out.stderr[-2000:])
            sys.exit(out.returncode)
        return json.loads(out.stdout.strip().splitlines()[-1])

    configs = [('off', 'off', args.root), ('on', 'on', args.root)]
    if args.parent:
        configs = [('parent_off', 'off', args.parent)] + configs
    runs = {name: [] for name, _, _ in configs}
    for _ in range(args.rounds):
        for name, what, root in configs:
            runs[name].append(run(what, root)['ms_per_step'])
    med = {k: float(np.median(v)) for k, v in runs.items()}
    res = {'steps': args.steps, 'rounds': args.rounds, 'rays': RAYS, 'samples': list(LEVELS), 'depth_loss_type': 'mse',
           'lambda_los': LAMBDA, 'los_sigma_m': SIGMA_M,
           'ms_per_step_runs': runs, 'ms_per_step_median': med, 'spread_ms': {k: float(max(v) - min(v)) for k, v in runs.items()},
           'on_minus_off_ms': med['on'] - med['off'], 'launches_us_per_call': run('launches', args.root)['us_per_call'],
           'raylos_first_launch_bytes_per_step_at_most': int(RAYS * (16 * sum(LEVELS) + 32 * len(LEVELS)))}
    outside = False
    if args.parent:
        lo, hi = min(runs['parent_off']), max(runs['parent_off'])
        res['off_minus_parent_off_ms'] = med['off'] - med['parent_off']
        res['parent_A_A_spread_ms'] = res['spread_ms']['parent_off']
        res['off_inside_parent_spread'] = outside_ok = bool(lo <= med['off'] <= hi)
        outside = not outside_ok
    print(json.dumps(res))
    if args.out:
        with open(args.out, 'w') as f:
            f.write(json.dumps(res, indent=1) + '\n')
    return 2 if outside else 0


if __name__ == '__main__':
    sys.exit(main())

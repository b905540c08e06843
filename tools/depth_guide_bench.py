"""Time the NeRF++ training step with depth-guided fine sampling (depth_guide.py) off and on, on one GPU, the step with it
off against another checkout of this package (the parent commit, built in its own tree) in alternating fresh processes, and the
library's one launch alone.

    python tools/depth_guide_bench.py [--parent /path/to/parent/checkout] [--rounds 5] [--steps 30] [--warmup 5] [--out profiles/depth_guide_time.json]
    python tools/depth_guide_bench.py --worker off          # one timing in this process (off | on | launch)

Workload: the NeRF++ step of bench.py's shape (1024 rays of one synthetic frame, 64 + 128 samples, bf16) with the mse depth loss on
the sparse synthetic prior and its own standard deviation; 'on' guides 64 of the 128 new foreground samples.  Each configuration runs
`rounds` times, interleaved (parent off, off, on, parent off, ...), one process each; the parent's runs against each other are the
A/A spread of the box.  The only gate: 'off' of this code stays inside that spread (the step makes no call the parent does not
make); the exit code is 2 when it does not.  What 'on' costs is reported: the new launch plus two single-volume fine calls and two
uniform fills in place of the one pair call.  'launch' times depthguide_merge by itself at (1024 rays, S_prev 64, S_in 64 + 64, G 64)
on buffers that stay put, uniforms drawn in the kernel.  Prints one JSON line (and writes it to --out).
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
RAYS, CASCADE, GUIDE = 1024, (64, 128), 64
LAUNCH = (64, 64 + 64, 64)                                # S_prev, S_in, G


def step_worker(kind, steps, warmup):
    import torch
    from outdoor_nerf_depth_amd import _lib as L
    from outdoor_nerf_depth_amd.synthetic import SyntheticKitti
    from outdoor_nerf_depth_amd.trainer import NerfppTrainer, batch_to_device
    d = torch.device('cuda:0')
    scene = SyntheticKitti()
    b = scene.random_batch(RAYS, np.random.RandomState(0))
    b['depth_std'] = scene.depth_std(b['frame'], np.zeros(RAYS, np.int64), b['depth_sup'])      # (the sparse prior's: 1 % everywhere)
    batch = batch_to_device(b, d)
    kw = dict(depth_guide_samples=GUIDE) if kind == 'on' else {}
    tr = NerfppTrainer(d, precision=L.PREC_BF16, cascade_samples=CASCADE, use_depth=True, depth_loss_type='mse', **kw)
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
    out = {'workload': kind, 'ms_per_step': ms, 'steps': steps, 'scalars': [float(v) for v in sc.cpu()]}
    if kind == 'on':
        out['guided_share'] = float((tr.last_depth_guide[1] == 0).float().mean())
    return out


def launch_worker(steps, warmup):
    """depthguide_merge alone: HIP events around `steps` back-to-back calls"""
    import torch
    from outdoor_nerf_depth_amd import depth_guide
    d = torch.device('cuda:0')
    rs = np.random.RandomState(0)
    S_prev, S_in, G = LAUNCH
    U = lambda S: torch.from_numpy(np.sort(rs.uniform(0.05, 1.4, (RAYS, S)), -1).astype(np.float32)).to(d)
    zp, zin = U(S_prev), U(S_in)
    wp = torch.from_numpy((rs.dirichlet(np.ones(S_prev), RAYS) * 0.9).astype(np.float32)).to(d)
    lo, hi = torch.full((RAYS,), 0.01, device=d), torch.full((RAYS,), 1.5, device=d)
    p = torch.from_numpy(np.where(rs.rand(RAYS) < 0.5, rs.uniform(0.1, 1.2, RAYS), 0).astype(np.float32)).to(d)
    s = (0.05 * p).contiguous()
    step = [0]

    def call():
        step[0] += 1
        return depth_guide.depth_guide(zp, wp, zin, lo, hi, G, prior=p, prior_std=s, rng=(777, step[0]))
    for _ in range(warmup):
        call()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(steps):
        call()
    b.record()
    torch.cuda.synchronize()
    return {'workload': 'launch', 'steps': steps, 'us_per_call': {'%dx(%d,%d,%d)' % ((RAYS,) + LAUNCH): 1e3 * a.elapsed_time(b) / steps}}


def worker(what, steps, warmup, root):
    sys.path.insert(0, root)
    res = launch_worker(steps, warmup) if what == 'launch' else step_worker(what, steps, warmup)
    print(json.dumps(res))


def main():
    p = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    p.add_argument('--worker', default=None, help='time one configuration in this process: off, on or launch')
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
    share = None
    for _ in range(args.rounds):
        for name, what, root in configs:
            r = run(what, root)
            runs[name].append(r['ms_per_step'])
            share = r.get('guided_share', share)
    med = {k: float(np.median(v)) for k, v in runs.items()}
    res = {'steps': args.steps, 'rounds': args.rounds, 'rays': RAYS, 'cascade': list(CASCADE), 'guide_samples': GUIDE, 'loss': 'mse',
           'precision': 'bf16', 'guided_share': share, 'ms_per_step_runs': runs, 'ms_per_step_median': med,
           'spread_ms': {k: float(max(v) - min(v)) for k, v in runs.items()}, 'on_minus_off_ms': med['on'] - med['off'],
           'launch_us_per_call': run('launch', args.root)['us_per_call']}
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

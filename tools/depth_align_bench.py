"""Time one alignment of relative depth priors to metric anchors (depthalign_fit_apply) at the size of the 295-frame KITTI sequence on
one GPU, the 'mse' training step of both paths against another checkout of this package (the parent commit, built in its own tree),
and the effect on training of the test scene whose priors are distorted per frame.

    python tools/depth_align_bench.py [--parent /path/to/parent/checkout] [--rounds 3] [--calls 20] [--train] [--out profiles/depth_align_time.json]
    python tools/depth_align_bench.py --worker call       # the timed calls in this process
    python tools/depth_align_bench.py --worker train      # the training runs in this process

The call: 295 frames of 375 x 1242 in disparity space with the defaults (10 reweighted solves), std_out asked for.  The prior is a
seeded random depth map per frame distorted by a scale and a shift of its own with 0.2 % noise; the anchor is that depth with 0.2 %
noise and a tenth of its pixels multiplied by 1.3 .. 2.5, once at 5 % of the pixels (a LiDAR sweep's coverage; a seeded uniform mask)
and once at every pixel.  Warm-up calls, then `calls` timed ones, each between two device events; the median, the extremes and every
time are reported.  Two windows: the library call by itself (outputs reused: the five kinds of launches, nothing of the host) and the
binding's align_async as a trainer calls it (host checks, allocation, the launches).  The call is once per run: the times are
reported, not gated.  Next to them the compulsory traffic -- prior and anchor read once, depth_out and std_out written once, 16
bytes per pixel -- and the ratio of the launches' time to that traffic at the HBM rate this project uses as achievable, 6.2 TB/s.

The training steps: tools/depth_gnll_bench.py's workers ('mse' only), this checkout and --parent in alternating fresh processes (the
one that goes first alternates from round to round); the parent's runs against each other are the A/A spread of the box.  Without
the load-time flags a step makes exactly the calls it made, so 'mse' of this code belongs inside that spread.

The training effect (--train): tests/test_gpu_depth_ssi.py's 12-frame scene whose depths_mono_crop are a_f * depth + b_f per frame,
with a tenth of the true depth's pixels as depths_lidar.  400 steps from seeds 0, 1, 2 (sampler and initial parameters) of `mse` on the
prior aligned at load time (Config.depth_align_anchor = 'lidar'), `mse` and `ssi` on the raw prior, and rgb-only; the figure is the
mean |rendered distance_mean - true depth| over the rays with a true depth, averaged over the last 50 batches (`runs`) and, because
one ray that ends at the far plane moves a mean by orders of magnitude, also the median of those 50 batch figures
(`runs_median_batch`).  Once at 1024 rays a batch (93 a frame)
and once at 64 (6 a frame: under ssi's min_rays, the thin groups of DESIGN 9.8's known limit).  Prints one JSON line (and writes it
to --out).
"""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from depth_consistency_bench import F, H, W, HBM_ACHIEVABLE, timed      # noqa: E402

KINDS = ('mse_aligned', 'mse', 'ssi', 'rgb_only')


def bench_inputs(dev):
    """(prior, sparse anchor, dense anchor) float32 [F, H, W] on the device"""
    import torch
    gen = torch.Generator(device=dev)
    gen.manual_seed(3)
    U = lambda *shape: torch.rand(shape, generator=gen, device=dev)
    G = lambda *shape: torch.randn(shape, generator=gen, device=dev)
    z = 2.0 + 78.0 * U(F, H, W)
    alpha, beta = 0.5 + 2.5 * U(F, 1, 1), 0.005 * U(F, 1, 1)
    prior = ((1.0 / z) * (1 + 0.002 * G(F, H, W)) + beta) / alpha
    dense = z * (1 + 0.002 * G(F, H, W))
    dense = torch.where(U(F, H, W) < 0.1, dense * (1.3 + 1.2 * U(F, H, W)), dense)
    sparse = torch.where(U(F, H, W) < 0.05, dense, torch.zeros_like(dense))
    return prior.contiguous(), sparse.contiguous(), dense.contiguous()


def worker_call(calls, warmup):
    import torch
    from outdoor_nerf_depth_amd import depth_align as DAL
    dev = torch.device('cuda:0')
    prior, sparse, dense = bench_inputs(dev)
    prm = DAL.check_params(space='disparity')
    res = {}
    for name, anchor in (('sparse_5_percent', sparse), ('dense', dense)):
        first = DAL.enqueue(prior, anchor, prm, std=True)
        launches, last = timed(lambda: DAL.enqueue(prior, anchor, prm, std=True, out=first.tensors), calls, warmup)
        binding, _ = timed(lambda: DAL.align_async(prior, anchor, std=True, space='disparity'), calls, warmup)
        rows = last.tensors['rows'].cpu().numpy()
        res[name] = {'launches_ms': launches, 'binding_ms': binding, 'totals': DAL.totals_line(rows),
                     'pairs': int(rows[:, 3].sum()), 'fitted': int((rows[:, 5] == 0).sum()), 'solves': int(rows[:, 6].sum())}
        del first, last
    print(json.dumps(res))


def _write_scene(root):
    """the scene of tests/test_gpu_depth_ssi.py's distorted_scene, plus depths_lidar: a tenth of the true depth's pixels"""
    from PIL import Image
    sys.path.insert(0, os.path.dirname(HERE))
    from tests.test_mip360_scene import write_scene
    write_scene(root, n_frames=12, H=32, W=40)
    rs = np.random.RandomState(7)
    os.makedirs(os.path.join(root, 'depths_lidar'))
    for name in sorted(os.listdir(os.path.join(root, 'depths_mono_crop'))):
        a, b = rs.uniform(0.5, 2.0), rs.uniform(-1.0, 1.0)
        f = os.path.join(root, 'depths_mono_crop', name)
        sup = np.asarray(Image.open(f)).astype(np.float64)
        Image.fromarray(np.where(sup > 0, np.clip(np.round(a * sup + b * 256.0), 1, 65535), 0).astype(np.uint16)).save(f)
    rs = np.random.RandomState(8)
    for name in sorted(os.listdir(os.path.join(root, 'depths_gt'))):
        gt = np.asarray(Image.open(os.path.join(root, 'depths_gt', name)))
        Image.fromarray(np.where(rs.rand(*gt.shape) < 0.1, gt, 0).astype(np.uint16)).save(os.path.join(root, 'depths_lidar', name))


def _train(data, kind, seed, batch, steps=400, last=50):
    import torch
    from outdoor_nerf_depth_amd import mip360 as M
    from outdoor_nerf_depth_amd import mip360_data as D
    from outdoor_nerf_depth_amd import mip360_train as TR
    dev = torch.device('cuda:0')
    b = ["Config.data_dir = '%s'" % data, 'Config.max_steps = %d' % steps, 'Config.batch_size = %d' % batch, 'Config.lr_delay_steps = 0',
         "Config.depth_sup_type = 'mono_crop'", 'Config.sample_every = 1', 'Config.compute_disp_metrics = %s' % (kind != 'rgb_only'),
         "Config.depth_loss_type = '%s'" % ('ssi' if kind == 'ssi' else 'mse')]
    if kind == 'mse_aligned':
        b.append("Config.depth_align_anchor = 'lidar'")
    cfg = D.parse_gin(bindings=b)
    scene = D.Scene(cfg)
    train = scene.device_frames('train', dev)
    tr = TR.make_trainer(cfg, dev, init_seed=seed, n_train_frames=train['cams'].shape[0])
    err = []
    for step in range(steps):
        bt = M.sample_batch(train['cams'], train['rgb_u8'], train['depth_sup'], seed, step, batch, scene.near, scene.far, depth_gt=train['depth_gt'])
        tr.train_step(bt['rays'], bt['rgb'], bt['depth_sup'], jitter01=list(bt['jitter01']), cam_idx=bt['pix'] if kind == 'ssi' else None)
        if step >= steps - last:
            m = bt['depth_gt'] > 0
            err.append(float(((tr.last_distance_mean.reshape(-1) - bt['depth_gt']).abs() * m).sum() / m.sum().clamp(min=1)))
    tr.flush()
    torch.cuda.synchronize()
    return float(np.mean(err)), float(np.median(err))


def worker_train(seeds=(0, 1, 2), batches=(1024, 64)):
    import tempfile
    res = {}
    with tempfile.TemporaryDirectory() as root:
        data = os.path.join(root, 'scene')
        _write_scene(data)
        for batch in batches:
            for kind in KINDS:
                both = [_train(data, kind, seed, batch) for seed in seeds]
                runs, med = [m for m, _ in both], [m for _, m in both]
                res['%s@%d' % (kind, batch)] = {'runs': runs, 'mean': float(np.mean(runs)), 'spread': float(max(runs) - min(runs)),
                                                'runs_median_batch': med, 'mean_of_median_batch': float(np.mean(med)),
                                                'spread_of_median_batch': float(max(med) - min(med))}
                sys.stderr.write('%s@%d %s\n' % (kind, batch, runs))
    print(json.dumps(res))


def main():
    p = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    p.add_argument('--worker', default=None, help="'call': the timed calls in this process; 'train': the training runs")
    p.add_argument('--parent', default=None, help='another checkout (built) whose mse training steps alternate with this one\'s')
    p.add_argument('--train', action='store_true', help='also run the training-effect comparison (24 runs of 400 steps)')
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
    if args.worker == 'train':
        return worker_train()

    def child(cmd, timeout=args.timeout):
        out = subprocess.run([sys.executable] + cmd, capture_output=True, text=True, timeout=timeout)
        if out.returncode != 0:                               # (nothing more is started on the GPU after a failed run)
            sys.stderr.write(out.stdout[-2000:] + out.stderr[-2000:])
            sys.exit(out.returncode)
        return json.loads(out.stdout.strip().splitlines()[-1])

    got = child([os.path.abspath(__file__), '--worker', 'call', '--calls', str(args.calls), '--warmup', str(args.warmup)])
    pixels = F * H * W
    per_pixel = {'read': 4 + 4, 'written': 4 + 4}
    traffic = 16 * pixels
    floor_ms = 1e3 * traffic / HBM_ACHIEVABLE
    res = {'call': {'frames': F, 'height': H, 'width': W, 'space': 'disparity', 'iters': 10, 'calls': args.calls, 'warmup': args.warmup,
                    'what': 'launches_ms: the library call alone (outputs reused); binding_ms: depth_align.align_async with its host '
                            'checks and allocation',
                    'compulsory_bytes': traffic, 'compulsory_bytes_per_pixel': per_pixel,
                    'hbm_achievable_bytes_per_s': HBM_ACHIEVABLE, 'ms_of_the_compulsory_traffic_at_that_rate': floor_ms, 'anchors': {}}}
    for name, g in got.items():
        ms, whole = g['launches_ms'], g['binding_ms']
        med = float(np.median(ms))
        res['call']['anchors'][name] = {
            'ms_median': med, 'ms_min': min(ms), 'ms_max': max(ms), 'ms': ms, 'binding_ms_median': float(np.median(whole)),
            'binding_ms_min': min(whole), 'binding_ms_max': max(whole), 'binding_ms': whole, 'totals': g['totals'], 'pairs': g['pairs'],
            'fitted': g['fitted'], 'solves': g['solves'], 'time_over_the_compulsory_traffic': med / floor_ms}
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
    if args.train:
        res['training_effect'] = child([os.path.abspath(__file__), '--worker', 'train'], timeout=1000)
    print(json.dumps(res))
    if args.out:
        with open(args.out, 'w') as f:
            f.write(json.dumps(res, indent=1) + '\n')
    return 0


if __name__ == '__main__':
    sys.exit(main())

"""Time one splat of a reconstruction's 3D points into depth priors (depthpoints_splat) at the size of the 295-frame KITTI sequence
on one GPU, the 'mse' training step of both paths against another checkout of this package (the parent commit, built in its own
tree), and the training effect of the points as the anchor of an alignment.

    python tools/depth_points_bench.py [--parent /path/to/parent/checkout] [--rounds 3] [--calls 20] [--train] [--out profiles/depth_points_time.json]
    python tools/depth_points_bench.py --worker call       # the timed calls in this process
    python tools/depth_points_bench.py --worker train      # the training runs in this process

The call: 295 frames of 375 x 1242 with the cameras of tools/depth_consistency_bench.py and a synthetic cloud of 200 000 points on
that scene's plane, each observed by 6 consecutive frames (1.2 M observations).  Nobody has counted the points of the KITTI
sequences' reconstructions here: the size is ASSUMED, a COLMAP model of a few hundred frames at this resolution being of that order.
Both modes, `track` (the observations) and `all` (every point into every frame, occl_radius 4), every output asked for.  Warm-up
calls, then `calls` timed ones, each between two device events; the median, the extremes and every time are reported.  Two windows:
the library call by itself (tables on the device, outputs reused: the fills, the scatter, the resolve and the row sum, nothing of
the host) and the binding's splat_async as a trainer calls it (host validation, three uploads, allocation, the launches).  The call
is once per run: the times are reported, not gated.  Next to them the compulsory traffic -- the z-buffer written once by the fill
and read once by the resolve (8 + 8 bytes per pixel), depth, std, point and origin written (4 + 4 + 4 + 1), the points read once
(32 bytes each) and, in the `track` mode, the observations (8 bytes each) -- and the ratio of the launches' time to that traffic at
the HBM rate this project uses as achievable, 6.2 TB/s.  The atomic traffic: one 8-byte integer minimum per projected observation.

The training steps: tools/depth_gnll_bench.py's workers ('mse' only), this checkout and --parent in alternating fresh processes (the
one that goes first alternates from round to round); the parent's runs against each other are the A/A spread of the box.  Without
the load-time flags a step makes exactly the calls it made, so 'mse' of this code belongs inside that spread.

The training effect (--train): the per-frame distorted scene of tools/depth_align_bench.py (12 frames of 32 x 40, every frame's
`mono_crop` prior distorted by a scale and a shift of its own) with a cloud of that scene's own surface points, tracks being the
frames that see a point at its depth.  MipNeRF-360, 400 steps at 1024 rays, three seeds each: `mse` on the prior aligned to the
points (Config.depth_align_anchor = 'points', Config.depth_points_vis = 'track'), `mse` on the raw prior, and rgb only; the figure
is the mean |rendered - true depth| over the last 50 batches.  The anchors per frame (depth_points_rows) are reported with it.
Prints one JSON line (and writes it to --out).
"""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from depth_consistency_bench import F, H, W, FOCAL, HBM_ACHIEVABLE, timed      # noqa: E402

N_POINTS, TRACK = 200000, 6
KINDS = ('mse_points_anchor', 'mse', 'rgb_only')


def bench_cloud():
    """(cams float64 [F, 16], points float64 [N_POINTS, 4], obs int32 [N_POINTS * TRACK, 2] sorted by (frame, point)): points on
    the plane z = 6 + 0.1 x + 0.05 y under random pixels of random frames of tools/depth_consistency_bench.py's cameras"""
    from outdoor_nerf_depth_amd import depth_consistency as DC
    rs = np.random.RandomState(0)
    c2w = np.zeros((F, 3, 4))
    for i in range(F):                                        # (plane_scene's cameras, without its depth maps)
        c2w[i, :, 3] = (0.3 * i, 0.05 * rs.randn(), 0.02 * i)
        a = rs.randn(3)
        a /= np.linalg.norm(a)
        th = rs.uniform(0.01, 0.06) if i % 3 else 0.0
        Kx = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
        c2w[i, :, :3] = np.eye(3) + np.sin(th) * Kx + (1 - np.cos(th)) * (Kx @ Kx)
    cams = DC.pack_cams(np.array([[FOCAL, 0, W / 2.0], [0, FOCAL, H / 2.0], [0, 0, 1.0]]), c2w)
    rs = np.random.RandomState(1)
    f, x, y = rs.randint(0, F, N_POINTS), rs.uniform(0, W, N_POINTS), rs.uniform(0, H, N_POINTS)
    d = np.einsum('nij,nj->ni', c2w[f, :, :3], np.stack([(x - W / 2.0) / FOCAL, (y - H / 2.0) / FOCAL, np.ones(N_POINTS)], 1))
    n, c = np.array([-0.1, -0.05, 1.0]), c2w[f, :, 3]
    t = (6.0 - c @ n) / (d @ n)
    points = np.concatenate([c + t[:, None] * d, rs.uniform(0.001, 0.01, (N_POINTS, 1))], 1)
    first = np.clip(f - TRACK // 2, 0, F - TRACK)
    obs = np.stack([np.repeat(np.arange(N_POINTS), TRACK), (first[:, None] + np.arange(TRACK)).reshape(-1)], 1)
    return cams, points, obs[np.lexsort((obs[:, 0], obs[:, 1]))].astype(np.int32)


def worker_call(calls, warmup):
    import torch
    from outdoor_nerf_depth_amd import depth_points as DP
    dev = torch.device('cuda:0')
    cams, points, obs = bench_cloud()
    res = {}
    for vis in DP.MODES:
        o = obs if vis == 'track' else None
        prm = DP.check_params(vis)
        tables = DP.upload(*DP._host_inputs(cams, points, o, (F, H, W))[:3], dev)
        # the launches by themselves: the tables on the device already, the outputs of the first call written again
        first = DP.enqueue(*tables, (F, H, W), prm)
        launches, last = timed(lambda: DP.enqueue(*tables, (F, H, W), prm, out=first.tensors), calls, warmup)
        binding, _ = timed(lambda: DP.splat_async(cams, points, o, (F, H, W), dev), calls, warmup)
        rows = last.tensors['rows'].sum(0).cpu().numpy()
        res[vis] = {'launches_ms': launches, 'binding_ms': binding, 'totals': dict(zip(DP.ROW_NAMES, (int(v) for v in rows)))}
        del first, last
    print(json.dumps(res))


# ------------------------------------------------------------------------------------------------------- the training effect
def _write_points(root, n=2000, seed=9):
    """points3D.txt for the scene of depth_align_bench._write_scene: the surface points under n random pixels of random frames, taken
    from depths_gt/ through the model's own cameras; a point's track is the images that see it at its depth within 1 %"""
    from PIL import Image
    from outdoor_nerf_depth_amd import mip360_data as D
    from tests.test_depth_points import write_points3d_txt
    sparse = os.path.join(root, 'sparse', '0')
    cams, images = D.read_model(sparse)
    fx, fy, cx, cy, _ = D.camera_intrinsics(cams[1][0], cams[1][3])
    gt_of = dict(zip(sorted(os.listdir(os.path.join(root, 'images'))), sorted(os.listdir(os.path.join(root, 'depths_gt')))))
    ids = list(images)
    Rt = {i: (D.qvec_to_rotmat(images[i][0]), images[i][1]) for i in ids}
    depth = {i: np.asarray(Image.open(os.path.join(root, 'depths_gt', gt_of[images[i][3]]))).astype(np.float64) / 256.0 for i in ids}
    Hh, Ww = depth[ids[0]].shape
    rs = np.random.RandomState(seed)
    xyz, tracks = [], []
    for _ in range(n):
        i = ids[rs.randint(len(ids))]
        x, y = rs.randint(Ww), rs.randint(Hh)
        d = depth[i][y, x]
        if not d > 0:
            continue
        R, t = Rt[i]
        w = R.T @ (np.array([(x + 0.5 - cx) / fx * d, (y + 0.5 - cy) / fy * d, d]) - t)
        seen = []
        for j in ids:
            p = Rt[j][0] @ w + Rt[j][1]
            if p[2] <= 0:
                continue
            u, v = int(np.floor(fx * p[0] / p[2] + cx)), int(np.floor(fy * p[1] / p[2] + cy))
            if 0 <= u < Ww and 0 <= v < Hh and abs(depth[j][v, u] - p[2]) <= 0.01 * p[2]:
                seen.append(j)
        xyz.append(w)
        tracks.append(seen)
    write_points3d_txt(os.path.join(sparse, 'points3D.txt'), xyz, rs.uniform(0.3, 1.5, len(xyz)), tracks)


def _train(data, kind, seed, batch=1024, steps=400, last=50):
    import torch
    from outdoor_nerf_depth_amd import mip360 as M
    from outdoor_nerf_depth_amd import mip360_data as D
    from outdoor_nerf_depth_amd import mip360_train as TR
    dev = torch.device('cuda:0')
    b = ["Config.data_dir = '%s'" % data, 'Config.max_steps = %d' % steps, 'Config.batch_size = %d' % batch, 'Config.lr_delay_steps = 0',
         "Config.depth_sup_type = 'mono_crop'", 'Config.sample_every = 1', 'Config.compute_disp_metrics = %s' % (kind != 'rgb_only'),
         "Config.depth_loss_type = 'mse'"]
    if kind == 'mse_points_anchor':
        b += ["Config.depth_align_anchor = 'points'", "Config.depth_points_vis = 'track'", 'Config.depth_points_min_track = 2']
    cfg = D.parse_gin(bindings=b)
    scene = D.Scene(cfg)
    train = scene.device_frames('train', dev)
    tr = TR.make_trainer(cfg, dev, init_seed=seed, n_train_frames=train['cams'].shape[0])
    err = []
    for step in range(steps):
        bt = M.sample_batch(train['cams'], train['rgb_u8'], train['depth_sup'], seed, step, batch, scene.near, scene.far, depth_gt=train['depth_gt'])
        tr.train_step(bt['rays'], bt['rgb'], bt['depth_sup'], jitter01=list(bt['jitter01']))
        if step >= steps - last:
            m = bt['depth_gt'] > 0
            err.append(float(((tr.last_distance_mean.reshape(-1) - bt['depth_gt']).abs() * m).sum() / m.sum().clamp(min=1)))
    tr.flush()
    torch.cuda.synchronize()
    info = {}
    if 'depth_points_rows' in train:
        info = {'anchors_per_frame': train['depth_points_rows'][:, 2].cpu().tolist(),
                'alignment_status_per_frame': train['depth_align_rows'][:, 5].cpu().tolist()}
    return float(np.mean(err)), info


def worker_train(seeds=(0, 1, 2)):
    import tempfile
    from depth_align_bench import _write_scene
    res = {}
    with tempfile.TemporaryDirectory() as root:
        data = os.path.join(root, 'scene')
        _write_scene(data)
        _write_points(data)
        for kind in KINDS:
            both = [_train(data, kind, seed) for seed in seeds]
            runs = [m for m, _ in both]
            res[kind] = dict({'runs': runs, 'mean': float(np.mean(runs)), 'spread': float(max(runs) - min(runs))}, **both[0][1])
            sys.stderr.write('%s %s\n' % (kind, runs))
    print(json.dumps(res))


def main():
    p = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    p.add_argument('--worker', default=None, help="'call': the timed calls in this process; 'train': the training runs")
    p.add_argument('--parent', default=None, help='another checkout (built) whose mse training steps alternate with this one\'s')
    p.add_argument('--train', action='store_true', help='also run the training-effect comparison (9 runs of 400 steps)')
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

    def child(cmd):
        out = subprocess.run([sys.executable] + cmd, capture_output=True, text=True, timeout=args.timeout)
        if out.returncode != 0:                               # (nothing more is started on the GPU after a failed run)
            sys.stderr.write(out.stdout[-2000:] + out.stderr[-2000:])
            sys.exit(out.returncode)
        return json.loads(out.stdout.strip().splitlines()[-1])

    got = child([os.path.abspath(__file__), '--worker', 'call', '--calls', str(args.calls), '--warmup', str(args.warmup)])
    pixels = F * H * W
    per_pixel = {'read': 8, 'written': 8 + 4 + 4 + 4 + 1}
    res = {'call': {'frames': F, 'height': H, 'width': W, 'points': N_POINTS, 'track': TRACK, 'focal': FOCAL, 'calls': args.calls,
                    'warmup': args.warmup, 'the_cloud_size_is': 'assumed: nobody has counted the points of the KITTI reconstructions here',
                    'what': 'launches_ms: the library call alone (tables on the device, outputs reused); binding_ms: '
                            'depth_points.splat_async with its host validation, uploads and allocation',
                    'compulsory_bytes_per_pixel': per_pixel, 'hbm_achievable_bytes_per_s': HBM_ACHIEVABLE, 'modes': {}}}
    for vis, g in got.items():
        traffic = (per_pixel['read'] + per_pixel['written']) * pixels + 32 * N_POINTS + (8 * N_POINTS * TRACK if vis == 'track' else 0)
        floor_ms = 1e3 * traffic / HBM_ACHIEVABLE
        ms, whole = g['launches_ms'], g['binding_ms']
        med = float(np.median(ms))
        res['call']['modes'][vis] = {
            'ms_median': med, 'ms_min': min(ms), 'ms_max': max(ms), 'ms': ms, 'binding_ms_median': float(np.median(whole)),
            'binding_ms_min': min(whole), 'binding_ms_max': max(whole), 'binding_ms': whole, 'totals': g['totals'],
            'compulsory_bytes': traffic, 'ms_of_the_compulsory_traffic_at_that_rate': floor_ms, 'time_over_the_compulsory_traffic': med / floor_ms,
            'integer_atomics': g['totals']['n_projected']}
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
        res['training_effect'] = child([os.path.abspath(__file__), '--worker', 'train'])
    print(json.dumps(res))
    if args.out:
        with open(args.out, 'w') as f:
            f.write(json.dumps(res, indent=1) + '\n')
    return 0


if __name__ == '__main__':
    sys.exit(main())

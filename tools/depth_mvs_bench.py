"""Time one plane sweep (depthmvs_sweep) at the size of the 295-frame KITTI sequence on one GPU, the 'mse' training step of both
paths against another checkout of this package (the parent commit, built in its own tree), and the effect of the prior on training.

    python tools/depth_mvs_bench.py [--parent /path/to/parent/checkout] [--rounds 3] [--calls 10] [--train] [--out profiles/depth_mvs_time.json]
    python tools/depth_mvs_bench.py --worker call       # the timed calls in this process
    python tools/depth_mvs_bench.py --worker train      # the training-effect runs in this process
    python tools/depth_mvs_bench.py --smooth_paths 4 8 [--train] [--out profiles/depth_mvs_smooth_time.json]
    python tools/depth_mvs_bench.py --worker smooth --smooth_paths 4 8      # the plain and the smoothed calls in this process

The call: 295 frames of 375 x 1242 of the analytic plane scene of tools/depth_consistency_bench.py, painted with a texture fixed in
the world (every pixel's world point quantised to a 2 cm lattice and hashed to a grey level), 4 views, 64 planes uniform in inverse
depth between 100 m and 2 m, the defaults otherwise, every output but the census asked for.  Warm-up calls, then `calls` timed ones,
each between two device events; the median, the extremes and every time are reported.  Two windows: the library call by itself
(cameras, lists and planes uploaded before, outputs reused: the census, the sweep and the row sum, nothing of the host) and the
binding's sweep_async as a trainer calls it (host checks, three small uploads, allocation, the launches).  The call is once per run:
the times are reported, not gated.  Next to them
  - the compulsory traffic: rgb read (3 bytes per pixel), the census written and read once (4 + 4), the outputs written (depth, std 8;
    status, plane 2; cost, second 4); the neighbours' census words a gather reads are counted as work, not as compulsory traffic.
    The ratio of the launches' time to that traffic at the HBM rate this project uses as achievable, 6.2 TB/s;
  - the work of the sweep, from its loop bounds: a step is one (cell of tile and halo, view, plane); it is 14 written float64
    operations (6 adds, 2 divisions, 2 multiplications, 2 adds, 2 floors), six 8-byte and three broadcast LDS reads, and, where the
    view is in bounds, one gather of 4 bytes.  Frame edges are not subtracted.
The per-launch split is taken from a kernel trace of the same worker, not from this script.

The training steps: tools/depth_gnll_bench.py's workers ('mse' only), this checkout and --parent in alternating fresh processes (the
one that goes first alternates from round to round); the parent's runs against each other are the A/A spread of the box.  Without
the load-time flag a step makes exactly the calls it made, so 'mse' of this code belongs inside that spread.

The training effect (--train): the tests' textured box scene as a COLMAP scene, 12 frames of 32 x 40; 400 steps of 1024 rays of the
MipNeRF-360 trainer, three seeds each of `mse` on the `mvs` prior (Config.depth_mvs_views = 4, 12 planes from 12 m to 2 m), the same
with Config.depth_cons_views = 4, the same with Config.depth_comp_iters = 3, `gnll` with the sweep's standard deviation (floored at
0.02 m), and rgb-only.  The metric: mean |rendered distance_mean - true depth| over the rays of a batch, over the last 50 batches;
per seed and pooled, each with its standard error.  Prints one JSON line (and writes it to --out).

--smooth_paths: the same call with semi-global smoothing, for 0 paths (the plain call) and every listed number of paths
in one process, the library call alone between device events: the median of `calls` after `warmup`, the totals, the workspace and
the frames the slabs hold under the binding's default budget.  Next to them the slab traffic from the loop bounds: entries (frames x
pixels x planes rounded up to 8) x (2 bytes written by the slab launch, 2 + 4 + 4 read and written per path but the first, which
reads no S, and 4 + 2 / planes read by the select).  With --train the training effect is `mse` on the `mvs` prior with and without
Config.depth_mvs_smooth_paths = 8 on the box scene whose band of lattice cells q_x in [-4, 4) is painted grey 128.
"""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from depth_consistency_bench import F, H, W, FOCAL, HBM_ACHIEVABLE, plane_scene, timed      # noqa: E402

VIEWS, PLANES, NEAR, FAR, RADIUS, LATTICE = 4, 64, 2.0, 100.0, 2, 0.02
TILE_W, TILE_H = 32, 16
OPS_STEP, LDS_BYTES_STEP = 14, 6 * 8 + 3 * 8
BYTES_PIXEL = 3 + 4 + 4 + 8 + 2 + 4


def texture(depth, cams):
    """uint8 [F, H, W, 3] on depth's device: every pixel's world point quantised to LATTICE metres and hashed to a grey level"""
    import torch
    dev = depth.device
    yy, xx = torch.meshgrid(torch.arange(H, device=dev, dtype=torch.float64), torch.arange(W, device=dev, dtype=torch.float64), indexing='ij')
    dc = torch.stack([(xx + 0.5 - W / 2.0) / FOCAL, (yy + 0.5 - H / 2.0) / FOCAL, torch.ones_like(xx)], -1)
    out = torch.empty(depth.shape + (3,), dtype=torch.uint8, device=dev)
    for f in range(depth.shape[0]):                                # frame by frame: the float64 temporaries stay small
        pose = torch.from_numpy(cams[f, 4:].reshape(3, 4)).to(dev)
        q = torch.floor((pose[:, 3] + depth[f].double()[..., None] * (dc @ pose[:, :3].T)) / LATTICE).long()
        h = (q[..., 0] * 73856093) ^ (q[..., 1] * 19349663) ^ (q[..., 2] * 83492791)
        h = (h ^ (h >> 13)) * 1274126177
        out[f] = ((h >> 16) & 255).to(torch.uint8)[..., None]
    return out


def worker_call(calls, warmup):
    import torch
    from outdoor_nerf_depth_amd import depth_mvs as DM
    dev = torch.device('cuda:0')
    depth, cams, nbr = plane_scene(dev)
    rgb = texture(depth, cams)
    prm = DM.check_params(VIEWS, PLANES, NEAR, FAR, agg_radius=RADIUS)
    table = DM.check_table(DM.planes_table(NEAR, FAR, PLANES))
    cams_d, nbr_d, inv_d = torch.from_numpy(cams).to(dev), torch.from_numpy(np.ascontiguousarray(nbr, np.int32)).to(dev), torch.from_numpy(table).to(dev)
    first = DM.enqueue(rgb, cams_d, nbr_d, inv_d, prm)
    launches, last = timed(lambda: DM.enqueue(rgb, cams_d, nbr_d, inv_d, prm, out=first.tensors), calls, warmup)
    binding, _ = timed(lambda: DM.sweep_async(rgb, cams, nbr, near=NEAR, far=FAR, planes=PLANES, agg_radius=RADIUS), calls, warmup)
    t = last.tensors
    acc = t['status'] == DM.ACCEPTED
    step = float(table[1] - table[0])
    err = (1.0 / t['depth'][acc].double() - 1.0 / depth[acc].double()).abs()
    print(json.dumps({'launches_ms': launches, 'binding_ms': binding, 'totals': dict(zip(DM.ROW_NAMES, (int(v) for v in t['rows'].sum(0).cpu()))),
                      'accepted_within_two_plane_steps': float((err <= 2 * step).double().mean()),
                      'absrel_of_the_accepted': float(((t['depth'][acc].double() - depth[acc].double()).abs() / depth[acc].double()).mean()),
                      'workspace_bytes': DM.workspace_bytes(F, H, W)}))


def worker_smooth(calls, warmup, paths):
    import torch
    from outdoor_nerf_depth_amd import depth_mvs as DM
    dev = torch.device('cuda:0')
    depth, cams, nbr = plane_scene(dev)
    rgb = texture(depth, cams)
    table = DM.check_table(DM.planes_table(NEAR, FAR, PLANES))
    cams_d, nbr_d, inv_d = torch.from_numpy(cams).to(dev), torch.from_numpy(np.ascontiguousarray(nbr, np.int32)).to(dev), torch.from_numpy(table).to(dev)
    step = float(table[1] - table[0])
    res = {}
    for n in [0] + list(paths):
        prm = DM.check_params(VIEWS, PLANES, NEAR, FAR, agg_radius=RADIUS, smooth_paths=n)
        first = DM.enqueue(rgb, cams_d, nbr_d, inv_d, prm)
        ms, last = timed(lambda: DM.enqueue(rgb, cams_d, nbr_d, inv_d, prm, out=first.tensors), calls, warmup)
        t = last.tensors
        acc = t['status'] == DM.ACCEPTED
        err = (1.0 / t['depth'][acc].double() - 1.0 / depth[acc].double()).abs()
        res[str(n)] = {'launches_ms': ms, 'ms_median': float(np.median(ms)), 'ms_min': min(ms), 'ms_max': max(ms),
                       'totals': dict(zip(DM.ROW_NAMES, (int(v) for v in t['rows'].sum(0).cpu()))),
                       'accepted_within_two_plane_steps_of_the_accepted': float((err <= 2 * step).double().mean()),
                       'workspace_bytes': DM.workspace_bytes(F, H, W)}
        if n:
            from outdoor_nerf_depth_amd import depth_mvs_smooth as MS
            slab = MS.slab_frames_of(F, H, W, PLANES)
            res[str(n)].update(slab_frames=slab, workspace_bytes=MS.workspace_bytes(F, H, W, PLANES, slab), penalties=DM.smooth_penalties(prm))
        del first, last, t
        torch.cuda.empty_cache()
    print(json.dumps(res))


KINDS = ('mse_mvs', 'mse_mvs_cons', 'mse_mvs_comp', 'gnll_mvs', 'rgb_only')
MVS = ["Config.depth_sup_type = 'mvs'", 'Config.depth_mvs_views = 4', 'Config.depth_mvs_planes = 12', 'Config.depth_mvs_near = 2.0',
       'Config.depth_mvs_far = 12.0']


def _write_scene(root, band=False):
    """tests/test_depth_consistency.py's analytic box scene as a COLMAP scene (12 frames of 32 x 40), its images repainted with the
    tests' texture fixed in the world; band: the lattice cells with q_x in [-4, 4) painted grey 128"""
    from PIL import Image
    sys.path.insert(0, os.path.dirname(HERE))
    from tests.test_depth_consistency import write_colmap_scene, analytic_cameras, analytic_depth
    from tests.test_depth_mvs import textured_images
    names, _ = write_colmap_scene(root, box=True)
    K, c2w = analytic_cameras(12, 32, 40)
    depth = analytic_depth(K, c2w, 32, 40, box=True)
    rgb = textured_images(K, c2w, depth)
    if band:
        from tests.test_depth_mvs import world_points, LATTICE as TEST_LATTICE
        q = np.floor(world_points(K, c2w, depth) / TEST_LATTICE).astype(np.int64)
        rgb = rgb.copy()
        rgb[(q[..., 0] >= -4) & (q[..., 0] < 4)] = 128
    for i, name in enumerate(names):
        Image.fromarray(rgb[i]).save(os.path.join(root, 'images', name))


def _train(data, kind, seed, batch=1024, steps=400, last=50):
    """|rendered distance_mean - true depth| averaged over the rays of each of the last batches: the list of those means"""
    import torch
    from outdoor_nerf_depth_amd import mip360 as M
    from outdoor_nerf_depth_amd import mip360_data as D
    from outdoor_nerf_depth_amd import mip360_train as TR
    dev = torch.device('cuda:0')
    b = ["Config.data_dir = '%s'" % data, 'Config.max_steps = %d' % steps, 'Config.batch_size = %d' % batch, 'Config.lr_delay_steps = 0',
         'Config.sample_every = 1', "Config.depth_loss_type = '%s'" % ('gnll' if kind == 'gnll_mvs' else 'mse')]
    b += ["Config.depth_sup_type = 'gt'", 'Config.compute_disp_metrics = False'] if kind == 'rgb_only' else MVS
    b += {'mse_mvs_cons': ['Config.depth_cons_views = 4'], 'mse_mvs_comp': ['Config.depth_comp_iters = 3'],
          'gnll_mvs': ['Config.depth_mvs_std_floor = 0.02'], 'mse_mvs_smooth': ['Config.depth_mvs_smooth_paths = 8']}.get(kind, [])
    cfg = D.parse_gin(bindings=b)
    scene = D.Scene(cfg)
    train = scene.device_frames('train', dev)
    tr = TR.make_trainer(cfg, dev, init_seed=seed, n_train_frames=train['cams'].shape[0])
    err = []
    for step in range(steps):
        bt = M.sample_batch(train['cams'], train['rgb_u8'], train['depth_sup'], seed, step, batch, scene.near, scene.far, depth_gt=train['depth_gt'])
        kw = dict(depth_std=TR.batch_depth_std(train['depth_std'], bt['pix'])) if 'depth_std' in train else {}
        tr.train_step(bt['rays'], bt['rgb'], bt['depth_sup'], jitter01=list(bt['jitter01']), **kw)
        if step >= steps - last:
            m = bt['depth_gt'] > 0
            err.append(float(((tr.last_distance_mean.reshape(-1) - bt['depth_gt']).abs() * m).sum() / m.sum().clamp(min=1)))
    tr.flush()
    torch.cuda.synchronize()
    return err, float((train['depth_sup'] > 0).float().mean())


def worker_train(seeds=(0, 1, 2), kinds=KINDS, band=False):
    import tempfile
    res = {}
    with tempfile.TemporaryDirectory() as root:
        data = os.path.join(root, 'scene')
        _write_scene(data, band)
        for kind in kinds:
            runs = [_train(data, kind, seed) for seed in seeds]
            every = np.concatenate([e for e, _ in runs])
            res[kind] = {'seeds': list(seeds), 'mean_per_seed': [float(np.mean(e)) for e, _ in runs],
                         'standard_error_per_seed': [float(np.std(e, ddof=1) / np.sqrt(len(e))) for e, _ in runs],
                         'mean': float(every.mean()), 'standard_error': float(np.std(every, ddof=1) / np.sqrt(len(every))),
                         'prior_coverage': runs[0][1]}
            sys.stderr.write('%s %s\n' % (kind, res[kind]['mean_per_seed']))
    print(json.dumps(res))


def main():
    p = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    p.add_argument('--worker', default=None, help="'call': the timed calls in this process; 'train': the training runs; 'smooth': the plain "
                   "and the smoothed calls; 'train_smooth': mse on the mvs prior with and without smoothing on the band scene")
    p.add_argument('--smooth_paths', type=int, nargs='+', default=None, help='time the call with 0 paths and with each of these (4, 8) '
                   'instead of the plain call alone; with --train the training effect of 8 paths on the band scene')
    p.add_argument('--train', action='store_true', help='also run the training-effect comparison (15 runs of 400 steps)')
    p.add_argument('--parent', default=None, help='another checkout (built) whose mse training steps alternate with this one\'s')
    p.add_argument('--rounds', type=int, default=3)
    p.add_argument('--calls', type=int, default=10)
    p.add_argument('--warmup', type=int, default=2)
    p.add_argument('--steps', type=int, default=60)
    p.add_argument('--timeout', type=int, default=400, help='seconds per worker process')
    p.add_argument('--out', default=None, help='also write the JSON result to this file')
    args = p.parse_args()
    sys.path.insert(0, os.path.dirname(HERE))
    if args.worker == 'call':
        return worker_call(args.calls, args.warmup)
    if args.worker == 'train':
        return worker_train()
    if args.worker == 'smooth':
        return worker_smooth(args.calls, args.warmup, args.smooth_paths or [4, 8])
    if args.worker == 'train_smooth':
        return worker_train(kinds=('mse_mvs', 'mse_mvs_smooth'), band=True)

    def child(cmd, timeout=None):
        out = subprocess.run([sys.executable] + cmd, capture_output=True, text=True, timeout=timeout or args.timeout)
        if out.returncode != 0:                               # (nothing more is started on the GPU after a failed run)
            sys.stderr.write(out.stdout[-2000:] + out.stderr[-2000:])
            sys.exit(out.returncode)
        return json.loads(out.stdout.strip().splitlines()[-1])

    if args.smooth_paths:
        g = child([os.path.abspath(__file__), '--worker', 'smooth', '--calls', str(args.calls), '--warmup', str(args.warmup), '--smooth_paths']
                  + [str(n) for n in args.smooth_paths])
        entries = F * H * W * ((PLANES + 7) // 8 * 8)
        for n, r in g.items():
            n = int(n)
            if n:
                r['slab_entries'] = entries
                r['slab_bytes_moved'] = entries * 2 + entries * (2 + 4) + (n - 1) * entries * (2 + 4 + 4) + entries * 4 + F * H * W * 2
                r['ms_of_the_slab_traffic_at_the_hbm_rate'] = 1e3 * r['slab_bytes_moved'] / HBM_ACHIEVABLE
                r['ms_over_the_plain_call'] = r['ms_median'] - g['0']['ms_median']
        res = {'call': {'frames': F, 'height': H, 'width': W, 'views': VIEWS, 'planes': PLANES, 'near': NEAR, 'far': FAR, 'agg_radius': RADIUS,
                        'calls': args.calls, 'warmup': args.warmup, 'hbm_achievable_bytes_per_s': HBM_ACHIEVABLE,
                        'what': 'the library call alone (cameras, lists and planes on the device, outputs reused), by smooth_paths',
                        'smooth_paths': g}}
        if args.train:
            res['training_effect_band_scene'] = child([os.path.abspath(__file__), '--worker', 'train_smooth'], timeout=900)
        print(json.dumps(res))
        if args.out:
            with open(args.out, 'w') as f:
                f.write(json.dumps(res, indent=1) + '\n')
        return 0
    g = child([os.path.abspath(__file__), '--worker', 'call', '--calls', str(args.calls), '--warmup', str(args.warmup)])
    pixels = F * H * W
    tiles = ((W + TILE_W - 1) // TILE_W) * ((H + TILE_H - 1) // TILE_H)
    steps = F * tiles * (TILE_W + 2 * RADIUS) * (TILE_H + 2 * RADIUS) * VIEWS * PLANES
    traffic = BYTES_PIXEL * pixels
    floor_ms = 1e3 * traffic / HBM_ACHIEVABLE
    ms, whole = g['launches_ms'], g['binding_ms']
    med = float(np.median(ms))
    res = {'call': {
        'frames': F, 'height': H, 'width': W, 'focal': FOCAL, 'views': VIEWS, 'planes': PLANES, 'near': NEAR, 'far': FAR, 'agg_radius': RADIUS,
        'calls': args.calls, 'warmup': args.warmup,
        'what': 'launches_ms: the library call alone (cameras, lists and planes on the device, outputs reused); binding_ms: '
                'depth_mvs.sweep_async with its host checks, uploads and allocation',
        'hbm_achievable_bytes_per_s': HBM_ACHIEVABLE, 'ms_median': med, 'ms_min': min(ms), 'ms_max': max(ms), 'ms': ms,
        'binding_ms_median': float(np.median(whole)), 'binding_ms_min': min(whole), 'binding_ms_max': max(whole), 'binding_ms': whole,
        'totals': g['totals'], 'accepted_within_two_plane_steps': g['accepted_within_two_plane_steps'],
        'absrel_of_the_accepted': g['absrel_of_the_accepted'], 'workspace_bytes': g['workspace_bytes'],
        'compulsory_bytes': traffic, 'ms_of_the_compulsory_traffic_at_that_rate': floor_ms, 'time_over_the_compulsory_traffic': med / floor_ms,
        'steps_cell_view_plane': steps, 'written_float64_operations': OPS_STEP * steps, 'float64_divisions': 2 * steps, 'gathers_at_most': steps,
        'lds_bytes_read': LDS_BYTES_STEP * steps, 'float64_operations_per_s': OPS_STEP * steps / (med * 1e-3),
        'steps_per_s': steps / (med * 1e-3), 'lds_bytes_per_s': LDS_BYTES_STEP * steps / (med * 1e-3)}}
    if args.parent:
        res['mse_step'] = {'steps': args.steps, 'rounds': args.rounds, 'paths': {}}
        for path in ('mip360', 'nerfpp'):
            runs = {'parent_mse': [], 'mse': []}
            for r in range(args.rounds):                      # (who goes first alternates: a process inherits the clocks the last one left)
                for name, root in (('parent_mse', args.parent), ('mse', os.path.dirname(HERE)))[::1 if r % 2 == 0 else -1]:
                    runs[name].append(child([os.path.join(HERE, 'depth_gnll_bench.py'), '--worker', path + ':mse', '--root', root,
                                             '--steps', str(args.steps), '--warmup', '5'])['ms_per_step'])
            med_ = {k: float(np.median(v)) for k, v in runs.items()}
            res['mse_step']['paths'][path] = {
                'ms_per_step_runs': runs, 'ms_per_step_median': med_, 'mse_minus_parent_mse_ms': med_['mse'] - med_['parent_mse'],
                'parent_A_A_spread_ms': max(runs['parent_mse']) - min(runs['parent_mse']),
                'mse_inside_parent_spread': bool(min(runs['parent_mse']) <= med_['mse'] <= max(runs['parent_mse']))}
    if args.train:
        res['training_effect'] = child([os.path.abspath(__file__), '--worker', 'train'], timeout=900)
    print(json.dumps(res))
    if args.out:
        with open(args.out, 'w') as f:
            f.write(json.dumps(res, indent=1) + '\n')
    return 0


if __name__ == '__main__':
    sys.exit(main())

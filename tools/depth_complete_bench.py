"""Time one completion of depth priors by image-guided filtering (depthcomp_complete) at the size of the 295-frame KITTI sequence on
one GPU, and the 'mse' training step of both paths against another checkout of this package (the parent commit, built in its own
tree).

    python tools/depth_complete_bench.py [--parent /path/to/parent/checkout] [--rounds 3] [--calls 20] [--train] [--out profiles/depth_complete_time.json]
    python tools/depth_complete_bench.py --worker call       # the timed calls in this process
    python tools/depth_complete_bench.py --worker train      # the training-effect runs in this process

The call: 295 frames of 375 x 1242 of the analytic plane scene of tools/depth_consistency_bench.py under a guide image that follows
its depth (a colour per half metre, plus a few levels of noise), conf, pass and rows asked for, once with a 5 % prior (a LiDAR
sweep's coverage; a seeded uniform mask) and once with the dense one, at the defaults (radius 4, 3 passes) and at radius 8.  Warm-up
calls, then `calls` timed ones, each between two device events; the median, the extremes and every time are reported.  Two windows:
the library call by itself (tables uploaded before, outputs reused: the passes and the row sum, nothing of the host) and the
binding's complete_async as a trainer calls it (the tables built and uploaded, allocation, the launches).  The call is once per run:
the times are reported, not gated.  Next to them
  - the compulsory traffic: depth read (4 bytes per pixel) and, where a pixel is empty, its colour (3); depth_out, std_out, conf
    written (12) and origin, pass (2); between two passes the state written and read (13 + 13).  A dense prior reads depth and
    writes the outputs and the state, and nothing else.  The ratio of the launches' time to that traffic at the HBM rate this
    project uses as achievable, 6.2 TB/s;
  - the work of the window walk, from the counts of the passes (the rows of calls with 1, 2, ... passes give the empty pixels every
    pass starts with): per tap of an empty pixel 2 written float64 operations (g, G += g) and 24 bytes of LDS reads (colour, both
    weights, confidence); per tap that carries depth 8 more operations and 8 more bytes.  Frame edges are not subtracted.
The per-launch split is taken from a kernel trace of the same worker, not from this script.

The training steps: tools/depth_gnll_bench.py's workers ('mse' only), this checkout and --parent in alternating fresh processes (the
one that goes first alternates from round to round); the parent's runs against each other are the A/A spread of the box.  Without
the load-time flags a step makes exactly the calls it made, so 'mse' of this code belongs inside that spread.

The training effect (--train): the tests' analytic box scene as a COLMAP scene, 12 frames of 32 x 40 under a guide image that follows
its surfaces, with a 5 % prior; 400 steps of 1024 rays of the MipNeRF-360 trainer, three seeds each of `mse` with
Config.depth_comp_iters = 3, the same after Config.depth_acc_views = 4, plain `mse`, rgb-only, and `gnll` with the completion's standard
deviation (floored at 0.02 m).  The metric: mean |rendered distance_mean - true depth| over the rays of a batch, over the last 50
batches; per seed and pooled, each with its standard error.  Prints one JSON line (and writes it to --out).
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

CONFIGS = {'defaults': dict(radius=4, iters=3), 'radius_8': dict(radius=8, iters=3)}


def guide(depth):
    """uint8 [F, H, W, 3] on depth's device: a colour per half metre of depth, plus noise of a few levels"""
    import torch
    gen = torch.Generator(device=depth.device)
    gen.manual_seed(3)
    palette = torch.randint(0, 256, (256, 3), generator=gen, device=depth.device, dtype=torch.int16)
    out = torch.empty(depth.shape + (3,), dtype=torch.uint8, device=depth.device)
    for f in range(depth.shape[0]):                                # frame by frame: the int16 temporaries stay small
        layer = (depth[f] * 2.0).floor().clamp_(0, 255).long()
        noise = torch.randint(-3, 4, layer.shape + (3,), generator=gen, device=depth.device, dtype=torch.int16)
        out[f] = (palette[layer] + noise).clamp_(0, 255).to(torch.uint8)
    return out


def worker_call(calls, warmup):
    import torch
    from outdoor_nerf_depth_amd import depth_complete as DCP
    dev = torch.device('cuda:0')
    dense, _, _ = plane_scene(dev)
    rgb = guide(dense)
    gen = torch.Generator(device=dev)
    gen.manual_seed(2)
    sparse = torch.where(torch.rand(dense.shape, generator=gen, device=dev) < 0.05, dense, torch.zeros_like(dense))
    res = {}
    for cname, cfg in CONFIGS.items():
        prm = DCP.check_params(**cfg)
        ws_h, wc_h = DCP.tables(prm['radius'], prm['sigma_space'], prm['sigma_colour'])
        ws_d, wc_d = torch.from_numpy(ws_h).to(dev), torch.from_numpy(wc_h).to(dev)
        for name, depth in (('sparse_5_percent', sparse), ('dense', dense)):
            first = DCP.enqueue(depth, rgb, None, ws_d, wc_d, prm)
            launches, last = timed(lambda: DCP.enqueue(depth, rgb, None, ws_d, wc_d, prm, out=first.tensors), calls, warmup)
            out = torch.empty_like(depth)
            binding, _ = timed(lambda: DCP.complete_async(depth, rgb, depth_out=out, **cfg), calls, warmup)
            rows = last.tensors['rows'].sum(0).cpu().numpy()
            true = dense[last.tensors['origin'] == DCP.ORIGIN_FILLED].double()
            got = last.tensors['depth'][last.tensors['origin'] == DCP.ORIGIN_FILLED].double()
            absrel = float(((got - true).abs() / true).mean()) if true.numel() else None
            after = []                                             # own + filled after 1, 2, ... passes: what the next pass starts with
            for k in range(1, prm['iters']):
                r = DCP.enqueue(depth, rgb, None, ws_d, wc_d, dict(prm, iters=k), out=first.tensors).tensors['rows'].sum(0).cpu().numpy()
                after.append(int(r[0] + r[1]))
            res['%s/%s' % (cname, name)] = {'launches_ms': launches, 'binding_ms': binding, 'absrel_of_the_filled': absrel,
                                            'totals': dict(zip(DCP.ROW_NAMES, (int(v) for v in rows))), 'valid_after_pass': after}
            del first, last, out
    print(json.dumps(res))


KINDS = ('mse_comp', 'mse_acc_comp', 'mse', 'rgb_only', 'gnll_comp')


def _write_scene(root):
    """tests/test_depth_consistency.py's analytic box scene as a COLMAP scene (12 frames of 32 x 40), its images repainted with a
    guide that follows the surfaces, plus depths_lidar: a seeded 5 % of the true depth's pixels"""
    from PIL import Image
    sys.path.insert(0, os.path.dirname(HERE))
    from tests.test_depth_consistency import write_colmap_scene
    from tests.depth_complete_reference import guide
    write_colmap_scene(root, box=True)
    rs = np.random.RandomState(7)
    os.makedirs(os.path.join(root, 'depths_lidar'))
    for name in sorted(os.listdir(os.path.join(root, 'depths_gt'))):
        gt = np.asarray(Image.open(os.path.join(root, 'depths_gt', name)))
        Image.fromarray(guide(gt.astype(np.float64) / 256.0, seed=3)).save(os.path.join(root, 'images', name))
        Image.fromarray(np.where(rs.rand(*gt.shape) < 0.05, gt, 0).astype(np.uint16)).save(os.path.join(root, 'depths_lidar', name))


def _train(data, kind, seed, batch=1024, steps=400, last=50):
    """|rendered distance_mean - true depth| averaged over the rays of each of the last batches: the list of those means"""
    import torch
    from outdoor_nerf_depth_amd import mip360 as M
    from outdoor_nerf_depth_amd import mip360_data as D
    from outdoor_nerf_depth_amd import mip360_train as TR
    dev = torch.device('cuda:0')
    b = ["Config.data_dir = '%s'" % data, 'Config.max_steps = %d' % steps, 'Config.batch_size = %d' % batch, 'Config.lr_delay_steps = 0',
         "Config.depth_sup_type = 'lidar'", 'Config.sample_every = 1', 'Config.compute_disp_metrics = %s' % (kind != 'rgb_only'),
         "Config.depth_loss_type = '%s'" % ('gnll' if kind == 'gnll_comp' else 'mse')]
    if kind.endswith('_comp'):
        b.append('Config.depth_comp_iters = 3')
    if kind == 'mse_acc_comp':
        b.append('Config.depth_acc_views = 4')
    if kind == 'gnll_comp':
        b.append('Config.depth_comp_std_floor = 0.02')
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
    coverage = float((train['depth_sup'] > 0).float().mean())
    return err, coverage


def worker_train(seeds=(0, 1, 2)):
    import tempfile
    res = {}
    with tempfile.TemporaryDirectory() as root:
        data = os.path.join(root, 'scene')
        _write_scene(data)
        for kind in KINDS:
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
    p.add_argument('--worker', default=None, help="'call': the timed calls in this process; 'train': the training runs")
    p.add_argument('--train', action='store_true', help='also run the training-effect comparison (15 runs of 400 steps)')
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
    if args.worker == 'train':
        return worker_train()

    def child(cmd, timeout=None):
        out = subprocess.run([sys.executable] + cmd, capture_output=True, text=True, timeout=timeout or args.timeout)
        if out.returncode != 0:                               # (nothing more is started on the GPU after a failed run)
            sys.stderr.write(out.stdout[-2000:] + out.stderr[-2000:])
            sys.exit(out.returncode)
        return json.loads(out.stdout.strip().splitlines()[-1])

    got = child([os.path.abspath(__file__), '--worker', 'call', '--calls', str(args.calls), '--warmup', str(args.warmup)])
    pixels = F * H * W
    res = {'call': {'frames': F, 'height': H, 'width': W, 'focal': FOCAL, 'calls': args.calls, 'warmup': args.warmup,
                    'what': 'launches_ms: the library call alone (tables on the device, outputs reused); binding_ms: '
                            'depth_complete.complete_async with its tables, uploads and allocation',
                    'hbm_achievable_bytes_per_s': HBM_ACHIEVABLE, 'runs': {}}}
    for name, g in got.items():
        cfg = CONFIGS[name.split('/')[0]]
        taps_per_pixel = (2 * cfg['radius'] + 1) ** 2
        own = g['totals']['n_own']
        valid = [own] + g['valid_after_pass']                  # valid pixels every pass starts with
        walk_taps = sum((pixels - v) * taps_per_pixel for v in valid)
        carrying = sum((pixels - v) * taps_per_pixel * (v / pixels) for v in valid)
        traffic = (4 + 14) * pixels + 3 * (pixels - own) + (cfg['iters'] - 1) * 26 * pixels
        floor_ms = 1e3 * traffic / HBM_ACHIEVABLE
        ms, whole = g['launches_ms'], g['binding_ms']
        med = float(np.median(ms))
        res['call']['runs'][name] = {
            'radius': cfg['radius'], 'iters': cfg['iters'], 'ms_median': med, 'ms_min': min(ms), 'ms_max': max(ms), 'ms': ms,
            'binding_ms_median': float(np.median(whole)), 'binding_ms_min': min(whole), 'binding_ms_max': max(whole), 'binding_ms': whole,
            'totals': g['totals'], 'valid_at_the_start_of_every_pass': valid, 'absrel_of_the_filled': g['absrel_of_the_filled'],
            'compulsory_bytes': traffic, 'ms_of_the_compulsory_traffic_at_that_rate': floor_ms, 'time_over_the_compulsory_traffic': med / floor_ms,
            'window_taps': walk_taps, 'window_taps_that_carry_depth_estimate': carrying,
            'written_float64_operations': 2 * walk_taps + 8 * carrying, 'lds_bytes_read': 24 * walk_taps + 8 * carrying,
            'float64_operations_per_s': (2 * walk_taps + 8 * carrying) / (med * 1e-3), 'lds_bytes_per_s': (24 * walk_taps + 8 * carrying) / (med * 1e-3)}
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
        res['training_effect'] = child([os.path.abspath(__file__), '--worker', 'train'], timeout=900)
    print(json.dumps(res))
    if args.out:
        with open(args.out, 'w') as f:
            f.write(json.dumps(res, indent=1) + '\n')
    return 0


if __name__ == '__main__':
    sys.exit(main())

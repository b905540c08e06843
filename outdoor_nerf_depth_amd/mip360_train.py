"""MipNeRF-360 training CLI on the HIP kernels: the counterpart of nerf-methods/mipnerf360/train.py for configs/360.gin
(scripts/train_kitti.sh).

    python -m outdoor_nerf_depth_amd.mip360_train --gin_configs=configs/360.gin \\
        --gin_bindings="Config.data_dir = '/data/kitti/DTU_format'" --gin_bindings="Config.checkpoint_dir = '/runs/x'" ...

Per step a batch of Config.batch_size rays (split over --world_size ranks) is drawn on the device by mip360.sample_batch
from the train frames, with the per-level jitter of the same counter-keyed generator, and fed to Mip360Trainer.train_step.
Every print_every steps: losses, PSNR, rays/s.  Checkpoints `{checkpoint_dir}/checkpoint_{step}` at step 1 and every
checkpoint_every steps (trainer state + sampler seed / counter; a run resumes from the newest one, bit-identically), and
at every checkpoint_every the test split is rendered into `test_preds_{step}/` with its metric files (train.py:304-388).
Config.depth_loss_type: 'mse' / 'l1' / 'kl' / 'urf' as upstream ('kl' / 'urf' with its reduction, which needs batches of as many
rays as a level has samples), or 'kl_ray' / 'urf_ray': the same two losses reduced per ray, for any batch size.
With --depth_metrics every such render also gets metric_depth_{name}_{step}.txt: the whole KITTI depth-metric set of the rendered
depth (n_valid, rmse, absrel, sqrel, absdiff, rmse_log, a1, a2, a3), in one device call for the split (depth_metrics.py).
"""
import argparse
import glob
import os
import re
import time

import numpy as np
import torch

from . import mip360 as M
from . import mip360_data as D
from .depth_metrics import DEPTH_METRICS_HELP as DEPTH_METRICS_HELP_FORMAT

CAP = 80.0             # depth metrics: the 80 m cap of train.py / eval.py
IMAGE_METRICS_HELP = ("also score the written color_*.png like the reference's utils/eval.py: SSIM (scikit-image defaults) and PSNR "
                      'on the 8-bit images, on the device -> metric_ssim_{step}.txt, metric_psnr8_{step}.txt')
COLOR_CORRECT_HELP = ("also colour-correct every test render against its ground-truth frame on the device, as upstream's eval.py does "
                      '(image.color_correct) -> color_cc_{idx:03d}.png, metric_cc_psnr_{step}.txt (per image, space-separated); with '
                      '--image_metrics / --lpips_weights also metric_cc_ssim / metric_cc_psnr8 / metric_cc_lpips of the corrected bytes')
DEPTH_VIS_HELP = ("also write the pictures upstream's eval.py draws of every test frame (vis.visualize_suite), coloured on the device: "
                  'vis_depth_mean_{idx:03d}.png and vis_depth_median_{idx:03d}.png (turbo over -log distance, clipped at the acc-weighted '
                  '0.5 / 99.5 percentiles of the frame, matted over a checkerboard by acc), vis_depth_triplet_, vis_color_matte_ and '
                  'vis_coords_mod_{idx:03d}.png')
DEPTH_METRICS_HELP = DEPTH_METRICS_HELP_FORMAT % 'metric_depth_{name}_{step}.txt for the nine names'
LPIPS_WEIGHTS_HELP = ("also score the written color_*.png with LPIPS (v0.1, VGG-16) on the device, as the reference's utils/eval.py "
                      'does on the CPU: A[,B] = one or two files (.npz or torch state dicts) that together hold '
                      "torchvision's VGG-16 `features.*` tensors and the lpips package's `lin{0..4}.model.1.weight`; this package "
                      'ships no weights.  Adds %s')


def he_uniform_params(shapes, rs):
    """flax nn.Dense with he_uniform kernels and zero biases (the MLPs' initialisers)"""
    return [(rs.uniform(-np.sqrt(6.0 / i), np.sqrt(6.0 / i), (i, o)).astype(np.float32), np.zeros(o, np.float32)) for i, o in shapes]


def make_trainer(cfg, device, world_size=1, init_seed=0, n_train_frames=None):
    """Mip360Trainer for the Config.  Config.compute_disp_metrics = False trains rgb-only: upstream adds the depth terms to the
    loss only under that flag (train_utils.py:108-150), so the trainer gets no depth loss then.  Model.num_glo_features = G > 0
    adds the per-image embeddings: the view layer is initialised with fan-in 283 + G, the table as flax's nn.Embed does
    (mip360.init_glo_embed), drawn after the MLPs so that G = 0 draws what it always drew.  n_train_frames (training only) is
    checked against Model.num_glo_embeddings before anything touches the device."""
    if int(cfg['max_steps']) < 2:
        raise D.ConfigError('Config.max_steps = %r: at least 2 (train_frac = (step - 1) / (max_steps - 1))' % cfg['max_steps'])
    G, E = int(cfg.get('num_glo_features', 0)), int(cfg.get('num_glo_embeddings', 1000))
    if n_train_frames is not None:
        D.check_glo_frames(cfg, n_train_frames)
    rs = np.random.RandomState(init_seed)                # identical initial parameters on every rank
    prop, nerf = he_uniform_params(M.mlp_shapes(M.PROP_CFG), rs), he_uniform_params(M.mlp_shapes(M.NERF_CFG, G), rs)
    depth_loss_type = cfg['depth_loss_type'] if cfg['compute_disp_metrics'] else None
    glo_kw = dict(num_glo_features=G, num_glo_embeddings=E, glo_embed=M.init_glo_embed(E, G, rs)) if G > 0 else {}
    tr = M.Mip360Trainer(prop, nerf, device, max_steps=int(cfg['max_steps']), lambda_depth=float(cfg['lambda_depth']),
                         depth_loss_type=depth_loss_type, world_size=world_size, depth_sigma=float(cfg['depth_sigma']), **glo_kw)
    tr.lr_kw = dict(lr_init=float(cfg['lr_init']), lr_final=float(cfg['lr_final']), lr_delay_steps=int(cfg['lr_delay_steps']),
                    lr_delay_mult=float(cfg['lr_delay_mult']))
    return tr


def mse_to_psnr(mse):
    """image.mse_to_psnr (internal/image.py)"""
    return -10. / np.log(10.) * np.log(mse)


def checkpoints(ckpt_dir):
    """[(step, path)] of the checkpoint_{step} files, oldest first"""
    out = []
    for p in glob.glob(os.path.join(ckpt_dir, 'checkpoint_*')):
        m = re.fullmatch(r'checkpoint_(\d+)', os.path.basename(p))
        if m and os.path.isfile(p):
            out.append((int(m.group(1)), p))
    return sorted(out)


def save_checkpoint(path, tr, seed, counter):
    state = tr.state_dict()
    cpu = {'step': state['step'], **{k: {kk: vv.cpu() for kk, vv in state[k].items()} for k in ('prop', 'nerf')}}
    if 'glo' in state:                                   # Model.num_glo_features > 0: the table, its moments, G and E
        cpu['glo'] = {kk: (vv.cpu() if torch.is_tensor(vv) else vv) for kk, vv in state['glo'].items()}
    tmp = path + '.tmp'
    torch.save({'trainer': cpu, 'seed': int(seed), 'counter': int(counter)}, tmp)
    os.replace(tmp, path)


def load_checkpoint(path, tr):
    ck = torch.load(path, map_location='cpu')
    tr.load_state_dict(ck['trainer'])
    return ck


def to_u8(img):
    """the bytes of utils.save_img_u8: clip to [0, 1], x 255, truncate"""
    return (np.clip(np.nan_to_num(img), 0., 1.) * 255.).astype(np.uint8)


def save_u8(img, path):
    """utils.save_img_u8"""
    from PIL import Image
    Image.fromarray(to_u8(img)).save(path)


def save_f32(img, path):
    """utils.save_img_f32: float32 TIFF"""
    from PIL import Image
    Image.fromarray(np.nan_to_num(img).astype(np.float32)).save(path, 'TIFF')


def depth_metrics(pred, gt, scale):
    """train.py:322-352 / eval.py: (rmse, absrel, absrel map) over 1e-3 < gt < 80 in metres, predictions clipped to
    [1e-3, 80]; pred / gt in scene units (divided by depth_scale here)."""
    g, p = gt / scale, pred / scale
    valid = (g < CAP) & (g > 1e-3)
    vg, vp = g[valid].clip(1e-3, CAP), p[valid].clip(1e-3, CAP)
    absrel_map = np.zeros_like(p)
    absrel_map[valid] = np.abs(vg - vp)
    with np.errstate(invalid='ignore', divide='ignore'):
        return float(np.sqrt(np.mean((vg - vp) ** 2))), float(np.mean(np.abs(vg - vp) / vg)), absrel_map


def save_depth_png(pred, scale, path):
    from PIL import Image
    Image.fromarray((np.asarray(pred / scale).clip(1e-3, CAP) * 256.0).astype(np.uint16)).save(path)


def write_metric(path, values):
    vals = list(values) + [np.mean(values)]
    with open(path, 'w') as f:
        f.write('\n'.join(str(v) for v in vals))


def render_split(model, scene, frames, cfg, train_frac, device_rgb=None, device_render=None, device_depth=None):
    """Yield (index, numpy rendering) for every frame of the test split (models.render_image per frame).  device_rgb: a list
    that receives each frame's float32 [H, W, 3] colour as a device tensor (what --color_correct keeps on the device).
    device_render: a list that receives each frame's whole rendering (M.RENDER_KEYS) plus the rays' 'origins' and 'directions'
    [H, W, 3] as float32 device tensors (what --depth_vis keeps on the device).  device_depth: a list that receives each frame's
    float32 [H, W] depth as a device tensor (what --depth_metrics keeps on the device)."""
    for j in range(frames['cams'].shape[0]):
        r = M.render_image(model, frames['cams'], j, scene.height, scene.width, scene.near, scene.far, train_frac,
                           int(cfg['render_chunk_size']))
        if device_rgb is not None:
            device_rgb.append(r['rgb'].float())
        if device_depth is not None:
            device_depth.append(r['depth'].float())
        if device_render is not None:
            rays = M.frame_rays(frames['cams'], j, scene.width, 0, scene.height * scene.width, scene.near, scene.far)
            device_render.append({**{k: v.float() for k, v in r.items()},
                                  **{k: rays[k].reshape(scene.height, scene.width, 3) for k in ('origins', 'directions')}})
        yield j, {k: v.float().cpu().numpy() for k, v in r.items()}


def write_image_metrics(out_dir, step, gt_u8, pred_bytes):
    """--image_metrics: SSIM and 8-bit PSNR of the written color_*.png bytes against the ground-truth bytes, as the reference's
    utils/eval.py scores a prediction folder (image_metrics.py: one device call for the split) -> metric_ssim_{step}.txt,
    metric_psnr8_{step}.txt.  gt_u8: device uint8 [F, H, W, 3] (Scene.device_frames); pred_bytes: list of F uint8 [H, W, 3] arrays."""
    from .image_metrics import image_metrics
    pred = torch.from_numpy(np.stack(pred_bytes)).to(gt_u8.device)
    ssim, psnr8 = image_metrics(gt_u8, pred)
    write_metric(os.path.join(out_dir, 'metric_ssim_%d.txt' % step), [float(v) for v in ssim])
    write_metric(os.path.join(out_dir, 'metric_psnr8_%d.txt' % step), [float(v) for v in psnr8])


def write_lpips(out_dir, step, gt_u8, pred_bytes, weights):
    """--lpips_weights: LPIPS (lpips.py, one device call for the split) of the same byte pairs -> metric_lpips_{step}.txt"""
    from .lpips import lpips_u8
    pred = torch.from_numpy(np.stack(pred_bytes)).to(gt_u8.device)
    write_metric(os.path.join(out_dir, 'metric_lpips_%d.txt' % step), [float(v) for v in lpips_u8(gt_u8, pred, weights)[0]])


def write_color_corrected(out_dir, step, gt_u8, rgb_f32, quantize, image_metrics=False, lpips_weights=None):
    """--color_correct: upstream's eval.py:152-180, 287-289 for the split in one device call (color_correct.py) ->
    color_cc_{idx:03d}.png and metric_cc_psnr_{step}.txt (per image, joined by single spaces, no mean: upstream's format of that
    file).  The corrected bytes stay on the device for their SSIM / 8-bit PSNR / LPIPS (metric_cc_ssim, metric_cc_psnr8,
    metric_cc_lpips, in the format of their plain twins).  gt_u8: device uint8 [F, H, W, 3]; rgb_f32: device float32 [F, H, W, 3]."""
    from PIL import Image
    from .color_correct import color_correct_async
    pend = color_correct_async(rgb_f32, gt_u8, quantize)
    scores = None
    if image_metrics:
        from .image_metrics import image_metrics_async
        scores = image_metrics_async(gt_u8, pend.cc_u8)
    _, cc_u8, psnr_cc, _ = pend.get()
    for idx in range(cc_u8.shape[0]):
        Image.fromarray(cc_u8[idx]).save(os.path.join(out_dir, 'color_cc_%03d.png' % idx))
    with open(os.path.join(out_dir, 'metric_cc_psnr_%d.txt' % step), 'w') as f:
        f.write(' '.join(str(float(v)) for v in psnr_cc))
    if scores is not None:
        ssim, psnr8 = scores.get()
        write_metric(os.path.join(out_dir, 'metric_cc_ssim_%d.txt' % step), [float(v) for v in ssim])
        write_metric(os.path.join(out_dir, 'metric_cc_psnr8_%d.txt' % step), [float(v) for v in psnr8])
    if lpips_weights is not None:
        from .lpips import lpips_u8
        write_metric(os.path.join(out_dir, 'metric_cc_lpips_%d.txt' % step),
                     [float(v) for v in lpips_u8(gt_u8, pend.cc_u8, lpips_weights)[0]])
    return psnr_cc


def write_depth_vis(out_dir, device_render):
    """--depth_vis: upstream's vis.visualize_suite for the split in one device call (depth_vis.py) -> vis_depth_mean_,
    vis_depth_median_, vis_depth_triplet_, vis_color_matte_ and vis_coords_mod_{idx:03d}.png.  device_render: render_split's list."""
    from .depth_vis import mip360_suite_async, save_pngs, SUITE_KEYS
    st = lambda k: torch.stack([r[k] for r in device_render])
    host = mip360_suite_async(st('rgb'), st('acc'), st('distance_mean'), st('distance_median'), st('distance_percentile_5'),
                              st('distance_percentile_95'), st('origins'), st('directions')).get()
    for k in SUITE_KEYS:
        save_pngs(host[k], os.path.join(out_dir, 'vis_' + k + '_%03d.png'))


def write_depth_metrics(out_dir, step, device_depth, depth_gt, scale):
    """--depth_metrics: the nine depth-error metrics of the split in one device call (depth_metrics.py) ->
    metric_depth_{name}_{step}.txt, per image, then the mean.  device_depth: render_split's list of float32 [H, W] device tensors;
    depth_gt: the split's device float32 [F, H, W] (Scene.device_frames); both in scene units, scale = Scene.scale."""
    from .depth_metrics import depth_metrics_async, METRIC_NAMES
    host = depth_metrics_async(torch.stack(device_depth), depth_gt, scale).get()
    for name in METRIC_NAMES:
        write_metric(os.path.join(out_dir, 'metric_depth_%s_%d.txt' % (name, step)), [float(v) for v in host[name]])


def load_lpips_weights(paths):
    """lpips.Weights of --lpips_weights A[,B], or None without the flag"""
    if not paths:
        return None
    from .lpips import load_weights
    return load_weights(paths)


def test_render(tr, scene, frames, cfg, step, out_dir, train_frac, image_metrics=False, lpips_weights=None, depth_metrics_flag=False):
    """The in-loop test render of train.py:304-388: color / depth PNGs, absrel maps, per-image PSNR / RMSE / AbsRel + mean.
    depth_metrics_flag (--depth_metrics): also metric_depth_{name}_{step}.txt of the whole depth-metric set (write_depth_metrics)."""
    os.makedirs(out_dir, exist_ok=True)
    model = M.Mip360Model.from_trainer(tr)
    gt_all = frames['depth_gt'].cpu().numpy()
    rgb_gt_all = frames['rgb_u8'].cpu().numpy()
    psnrs, rmses, absrels, pred_bytes = [], [], [], []
    device_depth = [] if depth_metrics_flag else None
    for idx, r in render_split(model, scene, frames, cfg, train_frac, device_depth=device_depth):
        rmse, absrel, absrel_map = depth_metrics(r['depth'], gt_all[idx], scene.scale)
        np.save(os.path.join(out_dir, 'absrel_%03d.npy' % idx), absrel_map)
        save_depth_png(r['depth'], scene.scale, os.path.join(out_dir, 'depth_%03d.png' % idx))
        rmses.append(rmse)
        absrels.append(absrel)
        gt = rgb_gt_all[idx].astype(np.float64) / 255.
        psnrs.append(float(mse_to_psnr(((r['rgb'].astype(np.float64) - gt) ** 2).mean())))
        save_u8(r['rgb'], os.path.join(out_dir, 'color_%03d.png' % idx))
        if image_metrics or lpips_weights is not None:
            pred_bytes.append(to_u8(r['rgb']))
    if image_metrics:
        write_image_metrics(out_dir, step, frames['rgb_u8'], pred_bytes)
    if lpips_weights is not None:
        write_lpips(out_dir, step, frames['rgb_u8'], pred_bytes, lpips_weights)
    if depth_metrics_flag:
        write_depth_metrics(out_dir, step, device_depth, frames['depth_gt'], scene.scale)
    write_metric(os.path.join(out_dir, 'metric_psnr_%d.txt' % step), psnrs)
    write_metric(os.path.join(out_dir, 'metric_rmse_%d.txt' % step), rmses)
    write_metric(os.path.join(out_dir, 'metric_absrel_%d.txt' % step), absrels)
    return np.mean(psnrs)


def train_worker(rank, cfg, world_size, port, seed, image_metrics=False, lpips_paths=None, depth_metrics_flag=False):
    device = torch.device('cuda', rank)
    lpips_weights = load_lpips_weights(lpips_paths) if rank == 0 else None
    torch.cuda.set_device(device)
    if world_size > 1:
        import torch.distributed as dist
        from . import dist_utils
        os.environ.setdefault('MASTER_ADDR', '127.0.0.1')
        os.environ['MASTER_PORT'] = str(port)
        dist_utils.apply_rccl_env_defaults(world_size)
        dist.init_process_group('nccl', rank=rank, world_size=world_size, device_id=device)
    ckpt_dir = cfg['checkpoint_dir']
    if not ckpt_dir:
        raise D.ConfigError('Config.checkpoint_dir is not set')
    os.makedirs(ckpt_dir, exist_ok=True)
    scene = D.Scene(cfg)
    D.check_glo_frames(cfg, len(scene.indices('train')))    # (before any device work, train.py:82-84)
    train = scene.device_frames('train', device)
    max_steps, every = int(cfg['max_steps']), int(cfg['checkpoint_every'])
    if every < 1:
        raise D.ConfigError('Config.checkpoint_every = %r: at least 1' % cfg['checkpoint_every'])
    # (an empty test split raises here when the run will render it, instead of writing NaN metrics later)
    test = scene.device_frames('test', device) if rank == 0 and every <= max_steps else None
    tr = make_trainer(cfg, device, world_size)
    rank_seed = seed + rank                             # one generator per rank (ddp_train_nerf: seed per rank)
    counter = 0
    found = checkpoints(ckpt_dir)
    if found:
        ck = load_checkpoint(found[-1][1], tr)
        counter = int(ck['counter'])
        if int(ck['seed']) != seed:
            raise D.ConfigError('%s was written with --seed %d' % (found[-1][1], ck['seed']))
        if rank == 0:
            print('Resuming from %s (step %d)' % (found[-1][1], tr.step), flush=True)
    n = int(cfg['batch_size']) // world_size
    t0, rays_done = time.time(), 0
    while tr.step < max_steps:
        b = M.sample_batch(train['cams'], train['rgb_u8'], train['depth_sup'], rank_seed, counter, n, scene.near, scene.far,
                           num_levels=tr.cfg['num_levels'])
        counter += 1
        # (the batch's frame column indexes the train split's frames 0..F-1: the rows of the embedding table)
        sc = tr.train_step(b['rays'], b['rgb'], b['depth_sup'], jitter01=list(b['jitter01']),
                           cam_idx=b['pix'] if tr.glo is not None else None)
        step = tr.step
        rays_done += n * world_size
        if rank == 0 and (step % int(cfg['print_every']) == 0 or step == 1):
            s = sc.cpu().numpy()
            mse = float(((tr.last_rgb - b['rgb']) ** 2).mean())
            dt = time.time() - t0
            print('step %d/%d: loss=%.5f data=%.5f depth=%.5f interlevel=%.5f distortion=%.5f psnr=%.2f lr=%.3e rays/s=%.0f'
                  % (step, max_steps, s[0], s[1], s[2], s[3], s[4], mse_to_psnr(mse),
                     M.learning_rate(step - 1, max_steps=max_steps, **tr.lr_kw), rays_done / max(dt, 1e-9)), flush=True)
            t0, rays_done = time.time(), 0
        if rank == 0 and (step == 1 or step % every == 0):
            save_checkpoint(os.path.join(ckpt_dir, 'checkpoint_%d' % step), tr, seed, counter)
        if rank == 0 and step % every == 0:
            train_frac = float(np.clip((step - 1) / (max_steps - 1), 0, 1))
            psnr = test_render(tr, scene, test, cfg, step, os.path.join(ckpt_dir, 'test_preds_%d' % step), train_frac,
                               image_metrics, lpips_weights, depth_metrics_flag)
            print('step %d: test psnr=%.3f' % (step, psnr), flush=True)
    if rank == 0 and max_steps % every != 0 and not os.path.exists(os.path.join(ckpt_dir, 'checkpoint_%d' % max_steps)):
        save_checkpoint(os.path.join(ckpt_dir, 'checkpoint_%d' % max_steps), tr, seed, counter)
    if world_size > 1:
        import torch.distributed as dist
        dist.barrier()
        dist.destroy_process_group()


def make_parser():
    p = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    D.add_gin_flags(p)
    p.add_argument('--world_size', type=int, default=1, help='data-parallel ranks (one process per GPU)')
    p.add_argument('--seed', type=int, default=0, help='sampler seed (rank r draws with seed + r)')
    p.add_argument('--port', type=int, default=12356)
    p.add_argument('--image_metrics', action='store_true', help=IMAGE_METRICS_HELP)
    p.add_argument('--lpips_weights', type=str, default=None, help=LPIPS_WEIGHTS_HELP % 'metric_lpips_{step}.txt')
    p.add_argument('--depth_metrics', action='store_true', help=DEPTH_METRICS_HELP)
    return p


def main(argv=None):
    args = make_parser().parse_args(argv)
    cfg = D.parse_gin(args.gin_configs, args.gin_bindings)
    if args.world_size > 1:
        if int(cfg['batch_size']) % args.world_size:
            raise D.ConfigError('Config.batch_size %d is not divisible by --world_size %d' % (cfg['batch_size'], args.world_size))
        torch.multiprocessing.spawn(train_worker, args=(cfg, args.world_size, args.port, args.seed, args.image_metrics, args.lpips_weights, args.depth_metrics), nprocs=args.world_size, join=True)
    else:
        train_worker(0, cfg, 1, args.port, args.seed, args.image_metrics, args.lpips_weights, args.depth_metrics)


if __name__ == '__main__':
    main()

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
rays as a level has samples), or one of the after-calls of depth_losses.LOSSES: 'kl_ray' / 'urf_ray', the same two
losses reduced per ray, for any batch size (9.7); 'ssi', scale and shift fitted per training frame, for relative-depth priors
(9.8; Config.depth_ssi_min_rays; log lines end with ssi_fit = the share of supervised rays in fitted frames); 'gnll', the Gaussian
negative log-likelihood for priors with a per-pixel standard deviation (9.9; depths{sfx}_{type}_std/ or Config.depth_gnll_std
metres everywhere; log lines end with gnll_gated = the share of supervised rays the gate let through).
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

from . import depth_losses as DL
from . import depth_prior_stages as PS
from . import eval_outputs as EO
from . import mip360 as M
from . import mip360_data as D
from .depth_metrics import DEPTH_METRICS_HELP as DEPTH_METRICS_HELP_FORMAT
from .eval_outputs import load_lpips_weights, mse_to_psnr

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
    checked against Model.num_glo_embeddings before anything touches the device; it is also the number of groups of the 'ssi'
    depth loss (one scale and shift per training frame)."""
    if int(cfg['max_steps']) < 2:
        raise D.ConfigError('Config.max_steps = %r: at least 2 (train_frac = (step - 1) / (max_steps - 1))' % cfg['max_steps'])
    G, E = int(cfg.get('num_glo_features', 0)), int(cfg.get('num_glo_embeddings', 1000))
    if n_train_frames is not None:
        D.check_glo_frames(cfg, n_train_frames)
    rs = np.random.RandomState(init_seed)                # identical initial parameters on every rank
    prop, nerf = he_uniform_params(M.mlp_shapes(M.PROP_CFG), rs), he_uniform_params(M.mlp_shapes(M.NERF_CFG, G), rs)
    depth_loss_type = cfg['depth_loss_type'] if cfg['compute_disp_metrics'] else None
    glo_kw = dict(num_glo_features=G, num_glo_embeddings=E, glo_embed=M.init_glo_embed(E, G, rs)) if G > 0 else {}
    ssi_kw = {}
    if DL.needs(depth_loss_type, 'cam_idx'):             # (without n_train_frames -- the evaluator -- the trainer cannot step)
        ssi_kw = dict(depth_ssi_groups=n_train_frames, depth_ssi_min_rays=int(cfg['depth_ssi_min_rays']))
    tr = M.Mip360Trainer(prop, nerf, device, max_steps=int(cfg['max_steps']), lambda_depth=float(cfg['lambda_depth']),
                         depth_loss_type=depth_loss_type, world_size=world_size, depth_sigma=float(cfg['depth_sigma']), **glo_kw,
                         **ssi_kw)
    tr.lr_kw = dict(lr_init=float(cfg['lr_init']), lr_final=float(cfg['lr_final']), lr_delay_steps=int(cfg['lr_delay_steps']),
                    lr_delay_mult=float(cfg['lr_delay_mult']))
    return tr


def batch_depth_std(depth_std, pix):
    """The resident frames' standard deviation [F, H, W] at a batch's pixels: pix [n, 3] = (frame, x, y) as sample_batch returns it"""
    f, x, y = pix.long().unbind(1)
    return depth_std[f, y, x].contiguous()


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


def save_depth_png(pred, scale, path):
    from PIL import Image
    Image.fromarray(EO.depth_u16(pred, scale)).save(path)


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


def write_metric_files(out_dir, step, scores, prefix=''):
    """metric_{prefix}{name}_{step}.txt of {name: per-image values}: per image, then the mean"""
    for name, vals in scores.items():
        EO.write_scores(os.path.join(out_dir, 'metric_%s%s_%d.txt' % (prefix, name, step)), vals)


def write_color_corrected(out_dir, step, gt_u8, rgb_f32, quantize, image_metrics=False, lpips_weights=None):
    """--color_correct: upstream's eval.py:152-180, 287-289 for the split in one device call (color_correct.py) ->
    color_cc_{idx:03d}.png and metric_cc_psnr_{step}.txt (per image, joined by single spaces, no mean: upstream's format of that
    file).  The corrected bytes stay on the device for their SSIM / 8-bit PSNR / LPIPS (metric_cc_ssim, metric_cc_psnr8,
    metric_cc_lpips, in the format of their plain twins).  gt_u8: device uint8 [F, H, W, 3]; rgb_f32: device float32 [F, H, W, 3]."""
    from PIL import Image
    cc_u8, psnr_cc, scores = EO.color_corrected(gt_u8, rgb_f32, quantize, image_metrics, lpips_weights)
    for idx, img in enumerate(cc_u8):
        Image.fromarray(img).save(os.path.join(out_dir, 'color_cc_%03d.png' % idx))
    with open(os.path.join(out_dir, 'metric_cc_psnr_%d.txt' % step), 'w') as f:
        f.write(' '.join(str(float(v)) for v in psnr_cc))
    write_metric_files(out_dir, step, scores, 'cc_')
    return psnr_cc


def write_depth_vis(out_dir, device_render):
    """--depth_vis: upstream's vis.visualize_suite for the split in one device call (depth_vis.py) -> vis_depth_mean_,
    vis_depth_median_, vis_depth_triplet_, vis_color_matte_ and vis_coords_mod_{idx:03d}.png.  device_render: render_split's list."""
    from . import depth_vis as DV
    keys = ('rgb', 'acc', 'distance_mean', 'distance_median', 'distance_percentile_5', 'distance_percentile_95', 'origins', 'directions')
    rows = EO.FrameBatches(lambda *frames: DV.mip360_suite_async(*frames), [[r[k] for r in device_render] for k in keys]).get()
    for k in DV.SUITE_KEYS:
        DV.save_pngs([row[k] for row in rows], os.path.join(out_dir, 'vis_' + k + '_%03d.png'))


def test_render(tr, scene, frames, cfg, step, out_dir, train_frac, image_metrics=False, lpips_weights=None, depth_metrics_flag=False,
                quantize_psnr=False, disp_metrics=False, tiffs=False, color_correct=False, depth_vis=False, verbose=False):
    """The test render of train.py:304-388 and eval.py:45-260: color / depth PNGs, absrel maps, per-image PSNR / RMSE / AbsRel +
    mean -> the mean PSNR.  What only mip360_eval asks for: quantize_psnr (PSNR of the render rounded to 8 bits,
    Config.eval_quantize_metrics), disp_metrics (metric_disparity_{mean,median}_mse), tiffs (distance_mean_ / distance_median_ /
    acc_{idx:03d}.tiff), color_correct, depth_vis, verbose (a line per image and metric).  image_metrics, lpips_weights and
    depth_metrics_flag (--depth_metrics): metric_ssim / metric_psnr8, metric_lpips and metric_depth_{name}_{step}.txt, one device
    call per flag for the split."""
    os.makedirs(out_dir, exist_ok=True)
    path = lambda f: os.path.join(out_dir, f)
    model = M.Mip360Model.from_trainer(tr)
    gt_depth = frames['depth_gt'].cpu().numpy()
    gt_rgb = frames['rgb_u8'].cpu().numpy()
    metrics, pred_bytes = {}, []
    device_rgb = [] if color_correct else None                        # the float32 renders stay on the device for the flag
    device_render = [] if depth_vis else None                         # and the whole renderings with their rays for this one
    device_depth = [] if depth_metrics_flag else None                 # and the depth frames for this one
    for idx, r in render_split(model, scene, frames, cfg, train_frac, device_rgb=device_rgb, device_render=device_render,
                               device_depth=device_depth):
        rmse, absrel, absrel_map = EO.depth_errors(r['depth'], gt_depth[idx], scene.scale)
        np.save(path('absrel_%03d.npy' % idx), absrel_map)
        save_depth_png(r['depth'], scene.scale, path('depth_%03d.png' % idx))
        m = {'rmse': rmse, 'absrel': absrel}
        rgb = r['rgb'].astype(np.float64)
        if quantize_psnr:
            rgb = np.round(rgb * 255) / 255
        m['psnr'] = float(mse_to_psnr(((rgb - gt_rgb[idx].astype(np.float64) / 255.) ** 2).mean()))
        if disp_metrics:
            for tag in ('mean', 'median'):
                disparity = 1 / (1 + r['distance_' + tag])
                m['disparity_%s_mse' % tag] = float(((disparity - gt_depth[idx]) ** 2).mean())
        for k, v in m.items():
            metrics.setdefault(k, []).append(v)
            if verbose:
                print('%-30s = %.4f' % (k, v))
        save_u8(r['rgb'], path('color_%03d.png' % idx))
        if image_metrics or lpips_weights is not None:
            pred_bytes.append(to_u8(r['rgb']))
        if tiffs:
            for key in ('distance_mean', 'distance_median', 'acc'):
                save_f32(r[key], path('%s_%03d.tiff' % (key, idx)))
    write_metric_files(out_dir, step, metrics)
    if image_metrics:                                                 # libnerfpp_hip.so: the one call of an evaluator into it
        write_metric_files(out_dir, step, EO.image_scores(frames['rgb_u8'], pred_bytes))
    if lpips_weights is not None:                                     # liblpips_hip.so
        write_metric_files(out_dir, step, EO.lpips_scores(frames['rgb_u8'], pred_bytes, lpips_weights))
    if color_correct:                                                 # libcolorcc_hip.so: one call for the split
        write_color_corrected(out_dir, step, frames['rgb_u8'], torch.stack(device_rgb), quantize_psnr, image_metrics, lpips_weights)
    if depth_vis:                                                     # libdepthvis_hip.so: one call for the split
        write_depth_vis(out_dir, device_render)
    if depth_metrics_flag:                                            # libdepthmetrics_hip.so: one call for the split
        write_metric_files(out_dir, step, EO.depth_scores(device_depth, frames['depth_gt'], scene.scale), 'depth_')
    return np.mean(metrics['psnr'])


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
    if rank == 0:                                       # the one log line of every depth-prior stage that ran
        for line in PS.totals_lines(scene, train):
            print(line, flush=True)
    max_steps, every = int(cfg['max_steps']), int(cfg['checkpoint_every'])
    if every < 1:
        raise D.ConfigError('Config.checkpoint_every = %r: at least 1' % cfg['checkpoint_every'])
    # (an empty test split raises here when the run will render it, instead of writing NaN metrics later)
    test = scene.device_frames('test', device) if rank == 0 and every <= max_steps else None
    tr = make_trainer(cfg, device, world_size, n_train_frames=len(scene.indices('train')))
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
        std_kw = {}
        if DL.needs(tr.depth_loss_type, 'depth_std'):   # the prior's standard deviation at the batch's pixels (frame, x, y)
            std_kw['depth_std'] = batch_depth_std(train['depth_std'], b['pix'])
        sc = tr.train_step(b['rays'], b['rgb'], b['depth_sup'], jitter01=list(b['jitter01']),
                           cam_idx=b['pix'] if (tr.glo is not None or DL.needs(tr.depth_loss_type, 'cam_idx')) else None, **std_kw)
        step = tr.step
        rays_done += n * world_size
        if rank == 0 and (step % int(cfg['print_every']) == 0 or step == 1):
            s = sc.cpu().numpy()
            mse = float(((tr.last_rgb - b['rgb']) ** 2).mean())
            dt = time.time() - t0
            # ssi_fit: the share of the batch's supervised rays whose frame was fitted; gnll_gated: the share the gate let through
            # (NeRF level)
            tail = DL.depth_log_tail(tr.depth_loss_type, DL.kept_stats(tr, tr.depth_loss_type))
            print('step %d/%d: loss=%.5f data=%.5f depth=%.5f interlevel=%.5f distortion=%.5f psnr=%.2f lr=%.3e rays/s=%.0f%s'
                  % (step, max_steps, s[0], s[1], s[2], s[3], s[4], mse_to_psnr(mse),
                     M.learning_rate(step - 1, max_steps=max_steps, **tr.lr_kw), rays_done / max(dt, 1e-9), tail), flush=True)
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

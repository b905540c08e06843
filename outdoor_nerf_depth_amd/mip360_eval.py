"""MipNeRF-360 evaluation CLI: the counterpart of nerf-methods/mipnerf360/eval.py:45-260 (scripts/eval_kitti.sh) on the
HIP kernels.  Restores the newest `checkpoint_{step}` of Config.checkpoint_dir, renders every test frame
(mip360.render_image) and writes to `{checkpoint_dir}/test_eval_preds_{eval_suffix}/`:

  color_{idx:03d}.png, depth_{idx:03d}.png (uint16, metres x 256), absrel_{idx:03d}.npy,
  distance_mean_{idx:03d}.tiff, distance_median_{idx:03d}.tiff, acc_{idx:03d}.tiff (float32),
  metric_psnr_{step}.txt, metric_rmse_{step}.txt, metric_absrel_{step}.txt and, with Config.compute_disp_metrics,
  metric_disparity_mean_mse_{step}.txt / metric_disparity_median_mse_{step}.txt (per image, then the mean).

PSNR is taken on 8-bit-quantised renders when Config.eval_quantize_metrics (the default).  The disparity metrics keep
upstream's quirk: 1 / (1 + distance) is compared with `disps_gt`, which for these scenes holds the (scaled) ground-truth
DEPTH, not a disparity -- the numbers are comparable with the paper's tables, not a meaningful disparity error.
With --image_metrics also metric_ssim_{step}.txt and metric_psnr8_{step}.txt: SSIM and PSNR of the written 8-bit color_*.png
against the ground-truth bytes, as the reference's utils/eval.py scores a prediction folder (image_metrics.py).
With --lpips_weights A[,B] also metric_lpips_{step}.txt: LPIPS (VGG-16) of the same byte pairs from the user's weight files (lpips.py).
With --color_correct also color_cc_{idx:03d}.png and metric_cc_psnr_{step}.txt (upstream's eval.py: every render warped to its
ground-truth frame's colours, color_correct.py), plus the metric_cc_ twins of the two flags above when they are given.
With --depth_vis also vis_depth_mean_, vis_depth_median_, vis_depth_triplet_, vis_color_matte_ and vis_coords_mod_{idx:03d}.png:
the pictures upstream's eval.py draws of every frame (vis.visualize_suite), coloured on the device (depth_vis.py).
With --depth_metrics also metric_depth_{name}_{step}.txt for n_valid, rmse, absrel, sqrel, absdiff, rmse_log, a1, a2 and a3: the
whole KITTI depth-metric set of the rendered depth, in one device call for the split (depth_metrics.py).
"""
import argparse
import os

import numpy as np
import torch

from . import mip360 as M
from . import mip360_data as D
from . import mip360_train as T


def make_parser():
    p = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    D.add_gin_flags(p)
    p.add_argument('--image_metrics', action='store_true', help=T.IMAGE_METRICS_HELP)
    p.add_argument('--lpips_weights', type=str, default=None, help=T.LPIPS_WEIGHTS_HELP % 'metric_lpips_{step}.txt')
    p.add_argument('--color_correct', action='store_true', help=T.COLOR_CORRECT_HELP)
    p.add_argument('--depth_vis', action='store_true', help=T.DEPTH_VIS_HELP)
    p.add_argument('--depth_metrics', action='store_true', help=T.DEPTH_METRICS_HELP)
    return p


def main(argv=None):
    args = make_parser().parse_args(argv)
    lpips_weights = T.load_lpips_weights(args.lpips_weights)
    cfg = D.parse_gin(args.gin_configs, args.gin_bindings)
    ckpt_dir = cfg['checkpoint_dir']
    if not ckpt_dir:
        raise D.ConfigError('Config.checkpoint_dir is not set')
    found = T.checkpoints(ckpt_dir)
    if not found:
        raise FileNotFoundError('no checkpoint_{step} in %s' % ckpt_dir)
    device = torch.device('cuda', 0)
    scene = D.Scene(cfg)
    frames = scene.device_frames('test', device)
    tr = T.make_trainer(cfg, device)
    T.load_checkpoint(found[-1][1], tr)
    step = tr.step
    print('Evaluating checkpoint at step %d.' % step, flush=True)
    out_dir = os.path.join(ckpt_dir, 'test_eval_preds_%s' % cfg['eval_suffix'])
    os.makedirs(out_dir, exist_ok=True)
    path = lambda f: os.path.join(out_dir, f)
    model = M.Mip360Model.from_trainer(tr)
    train_frac = step / int(cfg['max_steps'])                         # eval.py: state.step / config.max_steps
    gt_depth = frames['depth_gt'].cpu().numpy()
    gt_rgb = frames['rgb_u8'].cpu().numpy()
    metrics, pred_bytes = {}, []
    device_rgb = [] if args.color_correct else None                   # the float32 renders stay on the device for the flag
    device_render = [] if args.depth_vis else None                    # and the whole renderings with their rays for this one
    device_depth = [] if args.depth_metrics else None                 # and the depth frames for this one
    for idx, r in T.render_split(model, scene, frames, cfg, train_frac, device_rgb=device_rgb, device_render=device_render,
                                 device_depth=device_depth):
        rmse, absrel, absrel_map = T.depth_metrics(r['depth'], gt_depth[idx], scene.scale)
        np.save(path('absrel_%03d.npy' % idx), absrel_map)
        T.save_depth_png(r['depth'], scene.scale, path('depth_%03d.png' % idx))
        m = {'rmse': rmse, 'absrel': absrel}
        rgb = r['rgb'].astype(np.float64)
        if cfg['eval_quantize_metrics']:
            rgb = np.round(rgb * 255) / 255
        m['psnr'] = float(T.mse_to_psnr(((rgb - gt_rgb[idx].astype(np.float64) / 255.) ** 2).mean()))
        if cfg['compute_disp_metrics']:
            for tag in ('mean', 'median'):
                disparity = 1 / (1 + r['distance_' + tag])
                m['disparity_%s_mse' % tag] = float(((disparity - gt_depth[idx]) ** 2).mean())
        for k, v in m.items():
            metrics.setdefault(k, []).append(v)
            print('%-30s = %.4f' % (k, v))
        T.save_u8(r['rgb'], path('color_%03d.png' % idx))
        if args.image_metrics or lpips_weights is not None:
            pred_bytes.append(T.to_u8(r['rgb']))
        for key in ('distance_mean', 'distance_median', 'acc'):
            T.save_f32(r[key], path('%s_%03d.tiff' % (key, idx)))
    for k, v in metrics.items():
        T.write_metric(path('metric_%s_%d.txt' % (k, step)), v)
    if args.image_metrics:                                            # libnerfpp_hip.so: the one call of this CLI into it
        T.write_image_metrics(out_dir, step, frames['rgb_u8'], pred_bytes)
    if lpips_weights is not None:                                     # liblpips_hip.so
        T.write_lpips(out_dir, step, frames['rgb_u8'], pred_bytes, lpips_weights)
    if args.color_correct:                                            # libcolorcc_hip.so: one call for the split
        T.write_color_corrected(out_dir, step, frames['rgb_u8'], torch.stack(device_rgb), bool(cfg['eval_quantize_metrics']),
                                args.image_metrics, lpips_weights)
    if args.depth_vis:                                                # libdepthvis_hip.so: one call for the split
        T.write_depth_vis(out_dir, device_render)
    if args.depth_metrics:                                            # libdepthmetrics_hip.so: one call for the split
        T.write_depth_metrics(out_dir, step, device_depth, frames['depth_gt'], scene.scale)


if __name__ == '__main__':
    main()

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

import torch

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
    train_frac = step / int(cfg['max_steps'])                         # eval.py: state.step / config.max_steps
    T.test_render(tr, scene, frames, cfg, step, out_dir, train_frac, args.image_metrics, lpips_weights, args.depth_metrics,
                  quantize_psnr=bool(cfg['eval_quantize_metrics']), disp_metrics=bool(cfg['compute_disp_metrics']), tiffs=True,
                  color_correct=args.color_correct, depth_vis=args.depth_vis, verbose=True)


if __name__ == '__main__':
    main()

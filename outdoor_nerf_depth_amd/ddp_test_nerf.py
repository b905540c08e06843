#!/usr/bin/env python
"""Offline test-set render + metrics: the counterpart of nerf-methods/nerfplusplus/ddp_test_nerf.py
(:23-160) on the HIP path.  Same parser as training (`--config`, `--render_splits`, `--ckpt_path`);
for every split renders each image with the newest (or given) checkpoint -- deterministic
sampling, no perturbation -- and writes under {basedir}/{expname}/render_{split}_{step:06d}/:
  {idx:06d}.png, fg_*.png, bg_*.png, depth_*.png (uint16 = metres*256), error_rgb_*.png / absrel_*.png (the min-max
  normalised error maps of the training loop's evaluation, ddp_train_nerf.py:561-596) and
  psnr_/rmse_/absrel_{step:06d}.txt (per image, then the mean).
With --image_metrics also ssim_/psnr8_{step:06d}.txt: SSIM and PSNR of the written 8-bit {idx:06d}.png against the ground-truth
bytes, as the reference's utils/eval.py scores a render folder (image_metrics.py), for splits that have ground-truth rgb.
With --lpips_weights A[,B] also lpips_{step:06d}.txt: LPIPS (VGG-16) of the same byte pairs from the user's weight files (lpips.py).
With --depth_vis also fg_depth_*.png / bg_depth_*.png (jet, min-max over the frame, coloured on the device: depth_vis.py) and
depth_range_{step:06d}.txt ('fg_vmin fg_vmax bg_vmin bg_vmax' per image, in place of the reference's colour bar).
With --depth_metrics also depth_{name}_{step:06d}.txt for n_valid, rmse, absrel, sqrel, absdiff, rmse_log, a1, a2 and a3: the whole
KITTI depth-metric set of the frames that have ground-truth depth, in one device call for the split (depth_metrics.py).
PSNR = mse2psnr(mean((gt-im)^2)) on float images; depth metrics use the 80 m cap and
1e-3 < gt < 80 validity of the reference (:87-116).
"""
import os
import sys

from .ddp_train_nerf import (config_parser, validate_args, setup_logger, load_checkpoint, find_latest_checkpoint, render_split,
                             load_lpips_weights, logger)


def ddp_test_nerf(rank, args):
    import torch
    from .trainer import NerfppTrainer
    from .data_loader_split import load_data_split, synthetic_ray_samplers
    from . import _lib as L
    setup_logger()
    lpips_weights = load_lpips_weights(args) if rank == 0 else None
    world = args.world_size
    torch.cuda.set_device(rank)
    device = torch.device('cuda', rank)
    if world > 1:
        import torch.distributed as dist
        os.environ.setdefault('MASTER_ADDR', '127.0.0.1')
        os.environ['MASTER_PORT'] = str(args.port)
        from .dist_utils import apply_rccl_env_defaults
        apply_rccl_env_defaults(world, None if getattr(args, 'rccl_channels', -1) < 0 else args.rccl_channels)
        dist.init_process_group('nccl', rank=rank, world_size=world, device_id=device)
    cascade = tuple(int(x.strip()) for x in args.cascade_samples.split(','))
    # forward only: bf16, the two-pass fp16x2w forward (1e-4 outputs), or split-bf16 (also for split_fwd: the same forward)
    trainer = NerfppTrainer(device, precision={'bf16': L.PREC_BF16, 'fp16_fwd': L.PREC_FP16_FWD}.get(args.precision, L.PREC_SPLIT_BF16),
                            cascade_samples=cascade, use_depth=False, world_size=1,
                            # the renders sample as training did (--depth_guide_samples: around the first level's depth and spread)
                            **(dict(depth_guide_samples=args.depth_guide_samples, depth_guide_min_std=args.depth_guide_min_std)
                               if args.depth_guide_samples > 0 else {}))
    ckpt, start = find_latest_checkpoint(args)
    if ckpt is None:
        raise SystemExit('no checkpoint found under %s' % os.path.join(args.basedir, args.expname))
    logger.info('Reloading from: {}'.format(ckpt))
    load_checkpoint(ckpt, trainer)
    for split in [x.strip() for x in args.render_splits.strip().split(',')]:
        out_dir = os.path.join(args.basedir, args.expname, 'render_{}_{:06d}'.format(split, start))
        if rank == 0:
            os.makedirs(out_dir, exist_ok=True)
        if args.synthetic:
            hw = [int(x) for x in args.synthetic_hw.split(',')] if args.synthetic_hw else [None, None]
            samplers = synthetic_ray_samplers(split, args.testskip, args.depth_sup_type, args.synthetic_frames,
                                              hw[0], hw[1])
        else:
            samplers = load_data_split(args.datadir, args.scene, split, skip=args.testskip,
                                       try_load_min_depth=args.load_min_depth, depth_sup_type=args.depth_sup_type)
        if trainer.depth_guide_samples > 0:       # metres -> the scene's depth units, as the training run scaled it
            trainer.depth_guide_min_std = args.depth_guide_min_std * (samplers[0].get_depth_scale() or 1.0)
        for name, mean in render_split(rank, world, trainer, samplers, args, out_dir, start, device, lpips_weights):
            logger.info('%s %s: %s' % (split, name if name in ('psnr', 'rmse', 'absrel') else 'test_' + name, mean))
    if world > 1:
        dist.destroy_process_group()


def test(argv=None):
    import torch
    args = config_parser().parse_args(argv)
    validate_args(args)
    if args.world_size == -1:
        args.world_size = torch.cuda.device_count()
    if args.world_size <= 1:
        args.world_size = 1
        ddp_test_nerf(0, args)
    else:
        torch.multiprocessing.spawn(ddp_test_nerf, args=(args,), nprocs=args.world_size, join=True)


if __name__ == '__main__':
    setup_logger()
    test()

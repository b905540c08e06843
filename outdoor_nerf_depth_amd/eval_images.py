#!/usr/bin/env python
"""Score a folder of written renders against the ground-truth images: the counterpart of the reference's utils/eval.py
(:66-95), the script behind the PSNR and SSIM columns of the paper's tables.

    python -m outdoor_nerf_depth_amd.eval_images --gt_dir D --pred_dir D --method {mipnerf360,mipnerf360_cc,nerfpp} --split N

Ground truth: `{gt_dir}/*.jpg`, else `*.png`, sorted, of which the test frames are indices 9, 19, 29, ...; predictions:
`{pred_dir}/color_*.png` without the colour-corrected `color_cc_*.png` (mipnerf360), exactly those `color_cc_*.png`
(mipnerf360_cc) or `{pred_dir}/00*.png` (nerfpp), sorted.  Writes `eval_psnr.txt` and `eval_ssim.txt`
into pred_dir (per image, then the mean): scikit-image's peak_signal_noise_ratio / structural_similarity with
data_range=255 on the 8-bit images, computed on the device (image_metrics.py).  Without --lpips_weights LPIPS is not
computed and no eval_lpips.txt is written; with `--lpips_weights A[,B]` (the user's VGG-16 and lin weight files: lpips.py)
eval_lpips.txt is written in the same format (utils/eval.py:93-95).  With --color_correct every selected prediction
(`byte / 255`) is colour-corrected against its ground-truth frame on the device (color_correct.py, upstream's
image.color_correct): `color_cc_*.png` are written next to the predictions and scored into eval_cc_psnr.txt / eval_cc_ssim.txt
(and eval_cc_lpips.txt with weights), in the same format.

    python -m outdoor_nerf_depth_amd.eval_images --pred_dir D --method {mipnerf360,nerfpp} --depth_vis

colourises the depth files of an existing folder on the device (depth_vis.py) and scores nothing: see --help.

    python -m outdoor_nerf_depth_amd.eval_images --depth_metrics --gt_depth_dir D --pred_dir P --method {mipnerf360,nerfpp}
        [--depth_frames {test,all}] [--pred_depth_dir Q]

scores the depth files of a folder against ground-truth depth PNGs on the device (depth_metrics.py) and reads no colour image:
`P/depth_*.png` -- or, with --pred_depth_dir, the `*.png` of a depth prior folder Q such as depths_mono_crop -- against `D/*.png`
(uint16, metres x 256), of which `test` takes indices 9, 19, ... (a MipNeRF-360 scene's depths_gt) and `all` every file (a NeRF++
`{split}/depth`).  Writes eval_depth_{name}.txt into P for n_valid, rmse, absrel, sqrel, absdiff, rmse_log, a1, a2 and a3 (per
image, then the mean).
"""
import argparse
import glob
import os

import numpy as np

from . import eval_outputs as EO

PRED_PATTERNS = {'mipnerf360': 'color_*.png', 'mipnerf360_cc': 'color_cc_*.png', 'nerfpp': '00*.png'}
CC_PREFIX = 'color_cc_'
NO_LPIPS = 'eval_lpips.txt is not written: LPIPS needs pretrained VGG weights, which this package does not ship'


class EvalImagesError(ValueError):
    pass


def _imread_rgb(path):
    from PIL import Image
    a = np.array(Image.open(path))
    if a.ndim == 3 and a.shape[2] == 4:
        a = a[..., :3]
    if a.ndim != 3 or a.shape[2] != 3 or a.dtype != np.uint8:
        raise EvalImagesError('%s: expected an 8-bit RGB image, got shape %s dtype %s' % (path, a.shape, a.dtype))
    return np.ascontiguousarray(a)


def select_files(gt_dir, pred_dir, method, split):
    """(ground-truth paths of the test frames, prediction paths) as utils/eval.py:66-79 picks them"""
    if method not in PRED_PATTERNS:
        raise EvalImagesError('--method %r: expected one of %s' % (method, sorted(PRED_PATTERNS)))
    if split < 1:
        raise EvalImagesError('--split %d: at least 1 (utils/eval.py defines the test frames only then)' % split)
    gt_names = sorted(glob.glob(os.path.join(gt_dir, '*.jpg'))) or sorted(glob.glob(os.path.join(gt_dir, '*.png')))
    gts = [gt_names[i] for i in range(9, len(gt_names), 10)]
    preds = sorted(glob.glob(os.path.join(pred_dir, PRED_PATTERNS[method])))
    if method == 'mipnerf360':                     # color_*.png also matches the colour-corrected twins: not predictions here
        preds = [p for p in preds if not os.path.basename(p).startswith(CC_PREFIX)]
    if not gts:
        raise EvalImagesError('%s holds %d ground-truth images (*.jpg, else *.png): no test frame (indices 9, 19, ...)'
                              % (gt_dir, len(gt_names)))
    if len(gts) != len(preds):
        raise EvalImagesError('%d ground-truth test frames in %s but %d predictions (%s) in %s'
                              % (len(gts), gt_dir, len(preds), PRED_PATTERNS[method], pred_dir))
    return gts, preds


def device_image_metrics(gts, preds):
    """(ssim [F], psnr8 [F]) of lists of uint8 [H, W, 3] arrays, on the device: one call per frame size"""
    scores = EO.image_scores(gts, preds)
    return scores['ssim'], scores['psnr8']


def cc_name(pred_name):
    """path of the colour-corrected twin of a prediction: color_007.png -> color_cc_007.png, 000007.png -> color_cc_000007.png"""
    d, b = os.path.split(pred_name)
    return os.path.join(d, CC_PREFIX + (b[len('color_'):] if b.startswith('color_') else b))


def device_color_correct(gts, preds):
    """colour-corrected bytes (list of uint8 [H, W, 3]) of lists of uint8 arrays, on the device (color_correct.py)"""
    from .color_correct import color_correct_u8_lists
    return color_correct_u8_lists(gts, preds)[0]


DEPTH_VIS_HELP = ('colourise the depth files of --pred_dir on the device and stop (no scores, --gt_dir is not read).  mipnerf360: '
                  'distance_mean_*.tiff, distance_median_*.tiff and acc_*.tiff -> vis_depth_mean_*.png, vis_depth_median_*.png, the '
                  'bytes mip360_eval --depth_vis writes (a NaN distance was written to the TIFF as 0 and is coloured as 0 here).  '
                  'The depth_triplet, color_matte and coords_mod pictures need the distance percentiles, the float colour and the '
                  'rays, which the folder does not hold: only mip360_eval --depth_vis writes them.  nerfpp: depth_*.png (uint16, '
                  'metres x 256) -> vis_depth_*.png, jet over the min-max of the frame')


def _read_gray(path, dtype):
    from PIL import Image
    a = np.array(Image.open(path))
    if a.ndim != 2 or a.dtype != dtype:
        raise EvalImagesError('%s: expected a single-channel %s image, got shape %s dtype %s' % (path, np.dtype(dtype), a.shape, a.dtype))
    return a


def depth_vis_folder(pred_dir, method='mipnerf360'):
    """--depth_vis: write the depth pictures of a prediction folder next to its files; returns the paths written"""
    from PIL import Image
    from . import depth_vis as DV
    written = []

    def save(image, name):
        written.append(os.path.join(pred_dir, name))
        Image.fromarray(image).save(written[-1])

    if method == 'nerfpp':
        names = sorted(glob.glob(os.path.join(pred_dir, 'depth_*.png')))
        if not names:
            raise EvalImagesError('%s holds no depth_*.png' % pred_dir)
        frames = [_read_gray(n, np.uint16).astype(np.float32) for n in names]
        for name, row in zip(names, EO.FrameBatches(lambda x: DV.minmax_colorize_async(x), (frames,)).get()):
            save(row['image'], 'vis_' + os.path.basename(name))
        return written
    names = sorted(glob.glob(os.path.join(pred_dir, 'distance_mean_*.tiff')))
    if not names:
        raise EvalImagesError('%s holds no distance_mean_*.tiff' % pred_dir)
    tags = [os.path.basename(n)[len('distance_mean_'):-len('.tiff')] for n in names]
    read = lambda key: [_read_gray(os.path.join(pred_dir, '%s_%s.tiff' % (key, t)), np.float32) for t in tags]
    pair = lambda dmean, dmedian, acc: DV.mip360_depth_pair_async(dmean, dmedian, acc)
    rows = EO.FrameBatches(pair, (read('distance_mean'), read('distance_median'), read('acc'))).get()
    for key in ('depth_mean', 'depth_median'):
        for tag, row in zip(tags, rows):
            save(row[key], 'vis_%s_%s.png' % (key, tag))
    return written


DEPTH_METRICS_HELP = ('score the depth files of a folder against --gt_depth_dir on the device and stop (no colour image is read): the '
                      "whole KITTI depth-metric set over 1e-3 < gt < 80 m with predictions clipped to [1e-3, 80] m -> eval_depth_{name}.txt "
                      'in --pred_dir for n_valid, rmse, absrel, sqrel, absdiff, rmse_log, a1, a2, a3 (per image, then the mean).  '
                      'Predictions are depth_*.png of --pred_dir (uint16, metres x 256), or the *.png of --pred_depth_dir.  With '
                      '--method mipnerf360 a ground-truth value below 2 / 256 m is invalid, as in the scene loader')


def select_depth_files(gt_depth_dir, pred_dir, depth_frames=None, pred_depth_dir=None):
    """(ground-truth depth paths, predicted depth paths) of --depth_metrics.  depth_frames: 'test' takes the ground-truth files
    9, 19, ... of the sorted *.png (as select_files), 'all' every one; None is 'test', or 'all' with a pred_depth_dir."""
    if depth_frames is None:
        depth_frames = 'all' if pred_depth_dir else 'test'
    if depth_frames not in ('test', 'all'):
        raise EvalImagesError("--depth_frames %r: expected 'test' or 'all'" % (depth_frames,))
    gt_names = sorted(glob.glob(os.path.join(gt_depth_dir, '*.png')))
    gts = gt_names if depth_frames == 'all' else [gt_names[i] for i in range(9, len(gt_names), 10)]
    src, pattern = (pred_depth_dir, '*.png') if pred_depth_dir else (pred_dir, 'depth_*.png')
    preds = sorted(glob.glob(os.path.join(src, pattern)))
    if not gts:
        raise EvalImagesError('%s holds %d ground-truth depth images (*.png): no frame for --depth_frames %s%s'
                              % (gt_depth_dir, len(gt_names), depth_frames, ' (indices 9, 19, ...)' if depth_frames == 'test' else ''))
    if len(gts) != len(preds):
        raise EvalImagesError('%d ground-truth depth frames (--depth_frames %s) in %s but %d predictions (%s) in %s'
                              % (len(gts), depth_frames, gt_depth_dir, len(preds), pattern, src))
    return gts, preds


def depth_metrics_folder(gt_depth_dir, pred_dir, method='mipnerf360', depth_frames=None, pred_depth_dir=None, metrics_fn=None):
    """--depth_metrics: write eval_depth_{name}.txt into pred_dir; returns {name: [...per image, mean]}.  Files decode as
    raw / 256 in float32 (metres, scale 1); with method 'mipnerf360' a ground-truth raw < 2 is invalid (mip360_data.convert_depth).
    With pred_depth_dir (a depth prior folder scored against the LiDAR) the pixels the prior leaves empty (raw < 2) leave the valid
    set: their ground truth is set to -1 before the upload, and n_valid shows how much was scored.
    metrics_fn(preds [F, H, W], gts [F, H, W]) -> {name: [F]} on host arrays: the device call (depth_metrics.py) unless a caller
    brings its own; frames of one size go in one call."""
    from .depth_metrics import METRIC_NAMES
    from .mip360_data import convert_depth
    if method not in ('mipnerf360', 'nerfpp'):
        raise EvalImagesError("--depth_metrics with --method %r: expected 'mipnerf360' or 'nerfpp'" % (method,))
    gt_names, pred_names = select_depth_files(gt_depth_dir, pred_dir, depth_frames, pred_depth_dir)
    gts, preds = [], []
    for gn, pn in zip(gt_names, pred_names):
        g_raw, p_raw = _read_gray(gn, np.uint16), _read_gray(pn, np.uint16)
        if g_raw.shape != p_raw.shape:
            raise EvalImagesError('%s is %d x %d but %s is %d x %d' % (gn, g_raw.shape[0], g_raw.shape[1], pn, p_raw.shape[0], p_raw.shape[1]))
        g = convert_depth(g_raw) if method == 'mipnerf360' else g_raw.astype(np.float32) / np.float32(256)
        if pred_depth_dir:
            g[p_raw < 2] = -1.
        gts.append(g)
        preds.append(p_raw.astype(np.float32) / np.float32(256))
    if metrics_fn is None:
        per_image = EO.depth_scores(preds, gts, 1.0)
    else:
        rows = EO.FrameBatches(metrics_fn, (preds, gts), upload=False).get()
        per_image = {name: [row[name] for row in rows] for name in METRIC_NAMES}
    return {name: EO.write_scores(os.path.join(pred_dir, 'eval_depth_%s.txt' % name), per_image[name]) for name in METRIC_NAMES}


def evaluate(gt_dir, pred_dir, method='mipnerf360', split=4, metrics_fn=None, lpips_fn=None, cc_fn=None):
    """Write eval_psnr.txt / eval_ssim.txt into pred_dir; returns {'psnr': [...per image, mean], 'ssim': [...]}.
    metrics_fn(gts, preds) -> (ssim, psnr8): device_image_metrics unless a caller brings its own.
    lpips_fn(gts, preds) -> lpips [F]: when given, eval_lpips.txt is written too and 'lpips' is in the result.
    cc_fn(gts, preds) -> corrected bytes [F]: when given, color_cc_*.png are written next to the predictions and scored into
    eval_cc_psnr.txt / eval_cc_ssim.txt (/ eval_cc_lpips.txt): 'cc_psnr', 'cc_ssim' (, 'cc_lpips') in the result."""
    if cc_fn is not None and method == 'mipnerf360_cc':
        raise EvalImagesError('--color_correct with --method mipnerf360_cc: those files are colour-corrected already')
    gt_names, pred_names = select_files(gt_dir, pred_dir, method, split)
    gts, preds = [_imread_rgb(n) for n in gt_names], [_imread_rgb(n) for n in pred_names]
    for g, p, gn, pn in zip(gts, preds, gt_names, pred_names):
        if g.shape != p.shape:
            raise EvalImagesError('%s is %d x %d but %s is %d x %d' % (gn, g.shape[0], g.shape[1], pn, p.shape[0], p.shape[1]))
    ssim, psnr = (metrics_fn or device_image_metrics)(gts, preds)
    scores = [('psnr', psnr), ('ssim', ssim)]
    if lpips_fn is not None:
        scores.append(('lpips', lpips_fn(gts, preds)))
    if cc_fn is not None:
        from PIL import Image
        ccs = [np.ascontiguousarray(c) for c in cc_fn(gts, preds)]
        for c, pn in zip(ccs, pred_names):
            Image.fromarray(c).save(cc_name(pn))
        ssim_cc, psnr_cc = (metrics_fn or device_image_metrics)(gts, ccs)
        scores += [('cc_psnr', psnr_cc), ('cc_ssim', ssim_cc)]
        if lpips_fn is not None:
            scores.append(('cc_lpips', lpips_fn(gts, ccs)))
    # (sum / len as these files always had it: np.mean adds pairwise and can differ in the last bit)
    return {name: EO.write_scores(os.path.join(pred_dir, 'eval_%s.txt' % name), vals, lambda v: sum(v) / len(v)) for name, vals in scores}


def make_parser():
    p = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    p.add_argument('--gt_dir', type=str, help='folder of all ground-truth frames (*.jpg, else *.png)', default='./ground_truth')
    p.add_argument('--pred_dir', type=str, help='render folder; receives eval_psnr.txt and eval_ssim.txt', default='./prediction')
    p.add_argument('--method', type=str, default='mipnerf360', choices=sorted(PRED_PATTERNS),
                   help='names of the renders: color_*.png without color_cc_*.png (mipnerf360), color_cc_*.png (mipnerf360_cc) '
                        'or 00*.png (nerfpp)')
    p.add_argument('--split', type=int, default=4, help='>= 1: test frames are every 10th ground-truth frame from index 9')
    p.add_argument('--lpips_weights', type=str, default=None,
                   help="A[,B]: one or two files (.npz or torch state dicts) holding torchvision's VGG-16 `features.*` tensors and "
                        "the lpips package's `lin{0..4}.model.1.weight`; also writes eval_lpips.txt (LPIPS v0.1, VGG-16, on the device)")
    p.add_argument('--color_correct', action='store_true',
                   help='also colour-correct the selected predictions against the ground truth on the device '
                        "(upstream's image.color_correct): writes color_cc_*.png next to them and eval_cc_psnr.txt / "
                        'eval_cc_ssim.txt (and eval_cc_lpips.txt with --lpips_weights)')
    p.add_argument('--depth_vis', action='store_true', help=DEPTH_VIS_HELP)
    p.add_argument('--depth_metrics', action='store_true', help=DEPTH_METRICS_HELP)
    p.add_argument('--gt_depth_dir', type=str, default=None,
                   help='--depth_metrics: folder of the ground-truth depth PNGs (uint16, metres x 256): a MipNeRF-360 scene\'s '
                        'depths_gt or a NeRF++ {split}/depth')
    p.add_argument('--depth_frames', type=str, default=None, choices=['test', 'all'],
                   help='--depth_metrics: which ground-truth depth files are scored: every 10th from index 9 (test, the default) or '
                        'every file (all, the default with --pred_depth_dir)')
    p.add_argument('--pred_depth_dir', type=str, default=None,
                   help='--depth_metrics: score the *.png of this folder (a depth prior such as depths_mono_crop) instead of the '
                        'depth_*.png of --pred_dir; pixels the prior leaves empty (raw < 2) are not scored')
    return p


def main(argv=None):
    args = make_parser().parse_args(argv)
    if args.depth_vis:
        written = depth_vis_folder(args.pred_dir, 'nerfpp' if args.method == 'nerfpp' else 'mipnerf360')
        print('%d depth pictures -> %s' % (len(written), args.pred_dir))
        if not args.depth_metrics:
            return
    if args.depth_metrics:
        if not args.gt_depth_dir:
            raise EvalImagesError('--depth_metrics needs --gt_depth_dir')
        out = depth_metrics_folder(args.gt_depth_dir, args.pred_dir, args.method, args.depth_frames, args.pred_depth_dir)
        print('rmse = %s  absrel = %s  a1 = %s  (%d images) -> %s' % (out['rmse'][-1], out['absrel'][-1], out['a1'][-1],
                                                                     len(out['rmse']) - 1, args.pred_dir))
        return
    lpips_fn = None
    if args.lpips_weights:
        from .lpips import load_weights, lpips_u8_lists
        weights = load_weights(args.lpips_weights)
        lpips_fn = lambda gts, preds: lpips_u8_lists(gts, preds, weights)
    out = evaluate(args.gt_dir, args.pred_dir, args.method, args.split, lpips_fn=lpips_fn,
                   cc_fn=device_color_correct if args.color_correct else None)
    if lpips_fn is None:
        print(NO_LPIPS)
    else:
        print('lpips = %s' % out['lpips'][-1])
    if args.color_correct:
        print('cc_psnr = %s  cc_ssim = %s' % (out['cc_psnr'][-1], out['cc_ssim'][-1]))
    print('psnr = %s  ssim = %s  (%d images) -> %s' % (out['psnr'][-1], out['ssim'][-1], len(out['psnr']) - 1, args.pred_dir))


if __name__ == '__main__':
    main()

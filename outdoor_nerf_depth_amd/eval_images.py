#!/usr/bin/env python
"""Score a folder of written renders against the ground-truth images: the counterpart of the reference's utils/eval.py
(:66-95), the script behind the PSNR and SSIM columns of the paper's tables.

    python -m outdoor_nerf_depth_amd.eval_images --gt_dir D --pred_dir D --method {mipnerf360,nerfpp} --split N

Ground truth: `{gt_dir}/*.jpg`, else `*.png`, sorted, of which the test frames are indices 9, 19, 29, ...; predictions:
`{pred_dir}/color_*.png` (mipnerf360) or `{pred_dir}/00*.png` (nerfpp), sorted.  Writes `eval_psnr.txt` and `eval_ssim.txt`
into pred_dir (per image, then the mean): scikit-image's peak_signal_noise_ratio / structural_similarity with
data_range=255 on the 8-bit images, computed on the device (image_metrics.py).  Without --lpips_weights LPIPS is not
computed and no eval_lpips.txt is written; with `--lpips_weights A[,B]` (the user's VGG-16 and lin weight files: lpips.py)
eval_lpips.txt is written in the same format (utils/eval.py:93-95).
"""
import argparse
import glob
import os

import numpy as np

PRED_PATTERNS = {'mipnerf360': 'color_*.png', 'nerfpp': '00*.png'}
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
    if not gts:
        raise EvalImagesError('%s holds %d ground-truth images (*.jpg, else *.png): no test frame (indices 9, 19, ...)'
                              % (gt_dir, len(gt_names)))
    if len(gts) != len(preds):
        raise EvalImagesError('%d ground-truth test frames in %s but %d predictions (%s) in %s'
                              % (len(gts), gt_dir, len(preds), PRED_PATTERNS[method], pred_dir))
    return gts, preds


def device_image_metrics(gts, preds):
    """(ssim [F], psnr8 [F]) of lists of uint8 [H, W, 3] arrays, on the device: one call when all frames have one size"""
    import torch
    from .image_metrics import image_metrics
    dev = torch.device('cuda', torch.cuda.current_device())
    up = lambda imgs: torch.from_numpy(np.stack(imgs)).to(dev)
    if len(set(g.shape for g in gts)) == 1:
        return image_metrics(up(gts), up(preds))
    each = [image_metrics(up([g]), up([p])) for g, p in zip(gts, preds)]
    return np.concatenate([e[0] for e in each]), np.concatenate([e[1] for e in each])


def evaluate(gt_dir, pred_dir, method='mipnerf360', split=4, metrics_fn=None, lpips_fn=None):
    """Write eval_psnr.txt / eval_ssim.txt into pred_dir; returns {'psnr': [...per image, mean], 'ssim': [...]}.
    metrics_fn(gts, preds) -> (ssim, psnr8): device_image_metrics unless a caller brings its own.
    lpips_fn(gts, preds) -> lpips [F]: when given, eval_lpips.txt is written too and 'lpips' is in the result."""
    gt_names, pred_names = select_files(gt_dir, pred_dir, method, split)
    gts, preds = [_imread_rgb(n) for n in gt_names], [_imread_rgb(n) for n in pred_names]
    for g, p, gn, pn in zip(gts, preds, gt_names, pred_names):
        if g.shape != p.shape:
            raise EvalImagesError('%s is %d x %d but %s is %d x %d' % (gn, g.shape[0], g.shape[1], pn, p.shape[0], p.shape[1]))
    ssim, psnr = (metrics_fn or device_image_metrics)(gts, preds)
    out = {}
    scores = [('psnr', psnr), ('ssim', ssim)]
    if lpips_fn is not None:
        scores.append(('lpips', lpips_fn(gts, preds)))
    for name, vals in scores:
        vals = [float(v) for v in vals]
        vals.append(sum(vals) / len(vals))
        with open(os.path.join(pred_dir, 'eval_%s.txt' % name), 'w') as f:
            f.write('\n'.join(str(m) for m in vals))
        out[name] = vals
    return out


def main(argv=None):
    p = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    p.add_argument('--gt_dir', type=str, help='folder of all ground-truth frames (*.jpg, else *.png)', default='./ground_truth')
    p.add_argument('--pred_dir', type=str, help='render folder; receives eval_psnr.txt and eval_ssim.txt', default='./prediction')
    p.add_argument('--method', type=str, default='mipnerf360', choices=sorted(PRED_PATTERNS),
                   help='names of the renders: color_*.png (mipnerf360) or 00*.png (nerfpp)')
    p.add_argument('--split', type=int, default=4, help='>= 1: test frames are every 10th ground-truth frame from index 9')
    p.add_argument('--lpips_weights', type=str, default=None,
                   help="A[,B]: one or two files (.npz or torch state dicts) holding torchvision's VGG-16 `features.*` tensors and "
                        "the lpips package's `lin{0..4}.model.1.weight`; also writes eval_lpips.txt (LPIPS v0.1, VGG-16, on the device)")
    args = p.parse_args(argv)
    lpips_fn = None
    if args.lpips_weights:
        from .lpips import load_weights, lpips_u8_lists
        weights = load_weights(args.lpips_weights)
        lpips_fn = lambda gts, preds: lpips_u8_lists(gts, preds, weights)
    out = evaluate(args.gt_dir, args.pred_dir, args.method, args.split, lpips_fn=lpips_fn)
    if lpips_fn is None:
        print(NO_LPIPS)
    else:
        print('lpips = %s' % out['lpips'][-1])
    print('psnr = %s  ssim = %s  (%d images) -> %s' % (out['psnr'][-1], out['ssim'][-1], len(out['psnr']) - 1, args.pred_dir))


if __name__ == '__main__':
    main()

"""What the five evaluators (mip360_train's and ddp_train_nerf's in-loop test renders, mip360_eval, ddp_test_nerf, eval_images)
share once a frame is rendered: the score-file writer, the way frames reach a device library (FrameBatches), one scorer per flag
on top of it, and the host depth errors.  A CLI names its files; the values and their format come from here.

The device entry points are reached through their modules when a call is made (`depth_metrics.depth_metrics_async`,
`lpips.lpips_u8`, ...), so a test that replaces one of those attributes is seen here.  torch is imported where it is used.
"""
import numpy as np

CAP = 80.0             # depth errors and depth PNGs: the 80 m cap of the reference's evaluators


def mse_to_psnr(mse):
    """image.mse_to_psnr (mipnerf360/internal/image.py)"""
    with np.errstate(divide='ignore'):
        return -10. / np.log(10.) * np.log(mse)


def load_lpips_weights(paths):
    """lpips.Weights of --lpips_weights A[,B] (read before any rendering, so a bad file fails early), or None without the flag.
    paths: the flag's value, or the parsed arguments that carry it."""
    paths = getattr(paths, 'lpips_weights', paths)
    if not paths:
        return None
    from .lpips import load_weights
    return load_weights(paths)


def nan_mean(values):
    """np.mean; NaN (a frame without a valid pixel) passes through without a warning"""
    with np.errstate(invalid='ignore'):
        return float(np.mean(values))


def write_scores(path, values, mean=nan_mean):
    """A score file: one value per image, then their mean, joined by newlines without a trailing one.  Returns the list written."""
    vals = [float(v) for v in values]
    vals.append(mean(vals))
    with open(path, 'w') as f:
        f.write('\n'.join(str(v) for v in vals))
    return vals


def depth_errors(pred, gt, scale):
    """(rmse, absrel, float32 map of |gt - pred| on the valid pixels, 0 elsewhere) of one frame, as the reference's evaluators
    compute them (mipnerf360 train.py:322-352, nerfplusplus ddp_train_nerf.py:566-600): over 1e-3 < gt < 80 in metres, predictions
    clipped to [1e-3, 80]; pred / gt in scene units, metres = value / scale."""
    g, p = gt / scale, pred / scale
    valid = (g < CAP) & (g > 1e-3)
    vg, vp = g[valid].clip(1e-3, CAP), p[valid].clip(1e-3, CAP)
    err_map = np.zeros(np.shape(p), np.float32)
    err_map[valid] = np.abs(vg - vp)
    with np.errstate(invalid='ignore', divide='ignore'):
        return float(np.sqrt(np.mean((vg - vp) ** 2))), float(np.mean(np.abs(vg - vp) / vg)), err_map


def depth_u16(pred, scale):
    """the depth PNG's values: uint16 = metres x 256, clipped to [1e-3, 80] m"""
    return (np.asarray(pred / scale).clip(1e-3, CAP) * 256.0).astype(np.uint16)


def _frame(host, r):
    """frame r of a group's host result: row r of every array in a dict or tuple"""
    if isinstance(host, dict):
        return {k: _frame(v, r) for k, v in host.items()}
    if isinstance(host, tuple):
        return tuple(_frame(v, r) for v in host)
    return None if host is None else host[r]


class FrameBatches(object):
    """Frames -> device calls -> per-frame results.  columns: equally long sequences of frames, frame i of every column being one
    call's arguments for image i: host arrays, device tensors, or one device tensor [F, ...] that holds a whole split.  Frames are
    grouped by the shape of the first column's frame, and by keys[i] when a caller has an extra key (a depth scale); every group is
    stacked, uploaded where it is on the host, and handed to call(*stacked) -- call(*stacked, key) with keys -- at once, so all
    device work is enqueued before anything is read.  call returns a pending object (`.get()` -> arrays, a tuple or a dict of
    arrays with one row per frame) or such a result itself.  A split of one frame size is one call.
    upload=False leaves the stacks on the host as numpy arrays (a stand-in call that needs no device)."""

    def __init__(self, call, columns, keys=None, device=None, upload=True):
        self.n, self.columns, self.device = len(columns[0]), columns, device
        groups = {}
        for i in range(self.n):
            groups.setdefault((tuple(columns[0][i].shape), None if keys is None else keys[i]), []).append(i)
        stack = self._stack if upload else (lambda col, rows: np.stack([col[k] for k in rows]))
        self.groups = []
        for (_, key), rows in groups.items():
            stacked = [stack(col, rows) for col in columns]
            self.groups.append((rows, call(*stacked) if keys is None else call(*stacked, key)))

    def _stack(self, col, rows):
        import torch
        if torch.is_tensor(col):                          # a whole split that is on the device already goes as it is
            return col if len(rows) == len(col) else col[rows]
        if torch.is_tensor(col[rows[0]]):
            return torch.stack([col[k] for k in rows])
        if self.device is None:                           # host frames go next to a column that is on a device, else to the current one
            on_device = [t.device for t in (c if torch.is_tensor(c) else c[0] for c in self.columns) if torch.is_tensor(t) and t.is_cuda]
            self.device = on_device[0] if on_device else torch.device('cuda', torch.cuda.current_device())
        return torch.from_numpy(np.stack([col[k] for k in rows])).to(self.device)

    def column(self, pick):
        """pick(pending) -> device tensor [n, ...] of every group, as a column of a later FrameBatches: the frames in input order,
        still on the device, nothing read"""
        if len(self.groups) == 1:
            return pick(self.groups[0][1])
        out = [None] * self.n
        for rows, pend in self.groups:
            for r, k in enumerate(rows):
                out[k] = pick(pend)[r]
        return out

    def get(self):
        """the per-frame results on the host, in input order"""
        out = [None] * self.n
        for rows, pend in self.groups:
            host = pend if isinstance(pend, (dict, tuple)) else pend.get()
            for r, k in enumerate(rows):
                out[k] = _frame(host, r)
        return out


def image_scores(gts, preds, device=None):
    """--image_metrics: {'ssim', 'psnr8'} per image of uint8 [H, W, 3] frames -- the ground-truth bytes and the bytes written to
    the PNG (image_metrics.py; utils/eval.py:45-60 of the reference)"""
    return _ssim_psnr8(_image_batches(gts, preds, device).get())


def _image_batches(gts, preds, device):
    from . import image_metrics as IM
    return FrameBatches(lambda g, p: IM.image_metrics_async(g, p), (gts, preds), device=device)


def _ssim_psnr8(rows):
    return {'ssim': [float(s) for s, _ in rows], 'psnr8': [float(p) for _, p in rows]}


def lpips_scores(gts, preds, weights, device=None):
    """--lpips_weights: {'lpips'} per image of the same byte pairs (lpips.py)"""
    from . import lpips as LP
    rows = FrameBatches(lambda g, p: LP.lpips_u8(g, p, weights), (gts, preds), device=device).get()
    return {'lpips': [float(total) for total, _ in rows]}


def depth_scores(preds, gts, scale, device=None):
    """--depth_metrics: {name: per image} for depth_metrics.METRIC_NAMES of float32 [H, W] frames in scene units (depth_metrics.py).
    scale: metres = value / scale, one number for the split or one per frame (frames of one scale share a call)."""
    from . import depth_metrics as DM
    keys = [float(scale)] * len(preds) if np.ndim(scale) == 0 else [float(s) for s in scale]
    rows = FrameBatches(lambda p, g, s: DM.depth_metrics_async(p, g, s), (preds, gts), keys=keys, device=device).get()
    return {name: [float(row[name]) for row in rows] for name in DM.METRIC_NAMES}


def color_corrected(gts, imgs, quantize=True, image_metrics=False, lpips_weights=None, device=None):
    """--color_correct: (corrected bytes per image on the host, psnr_cc per image, {'ssim', 'psnr8', 'lpips'} of the corrected bytes
    as asked) of float32 renders imgs against the ground-truth bytes gts (color_correct.py; upstream's eval.py:152-180).  The
    corrected bytes feed their scores from the device (the pending correction's .tensors['cc_u8']), without a host round trip."""
    from . import color_correct as CC
    batches = FrameBatches(lambda img, ref: CC.color_correct_async(img, ref, quantize), (imgs, gts), device=device)
    cc_dev = batches.column(lambda pend: pend.tensors['cc_u8'])
    pending = _image_batches(gts, cc_dev, device) if image_metrics else None     # enqueued before the correction is read
    rows = batches.get()
    scores = _ssim_psnr8(pending.get()) if image_metrics else {}
    if lpips_weights is not None:
        scores.update(lpips_scores(gts, cc_dev, lpips_weights, device))
    return [np.ascontiguousarray(row[1]) for row in rows], np.asarray([float(row[2]) for row in rows]), scores

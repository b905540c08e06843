"""SSIM and 8-bit PSNR of finished frames on the device: the image columns of the paper's tables.

The reference scores its runs with utils/eval.py:45-60, which re-reads the written PNGs and calls scikit-image's
`structural_similarity(gt, pred, data_range=255, multichannel=True)` and `peak_signal_noise_ratio(gt, pred, data_range=255)`.
`image_metrics` computes the same two numbers from the same bytes with one launch of nerfpp_image_metrics_u8
(include/nerfpp_hip.h) for a whole test split: exact integer window sums, float64 S, no atomics -- bit-reproducible.
There is no host path here: without libnerfpp_hip.so and a device the call raises.
"""
import ctypes as C

import numpy as np

from . import _lib as L

_workspaces = {}          # (device index, F, H, W) -> device buffer of nerfpp_image_metrics_workspace_bytes


def workspace_bytes(n_frames, H, W):
    """Size of the call's scratch buffer; raises NerfppError for sizes the library rejects (H < 7, W < 7).  Needs no GPU."""
    n = L.lib().nerfpp_image_metrics_workspace_bytes(int(n_frames), int(H), int(W))
    if n < 0:
        raise L.NerfppError(L.lib().nerfpp_last_error().decode('utf-8', 'replace'))
    return n


def _u8(t, name):
    import torch
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise L.NerfppError('%s: expected a CUDA/HIP uint8 tensor (image_metrics has no CPU path)' % name)
    if t.dtype != torch.uint8:
        raise L.NerfppError('%s: expected uint8 (the bytes written to the PNG), got %s' % (name, t.dtype))
    if t.dim() == 3:
        t = t[None]
    if t.dim() != 4 or t.shape[-1] != 3:
        raise L.NerfppError('%s: expected [H, W, 3] or [F, H, W, 3], got %s' % (name, tuple(t.shape)))
    return t.contiguous()


class PendingMetrics(object):
    """The device result of one image_metrics_async call; `.get()` synchronises (once) and returns (ssim [F], psnr8 [F])."""

    def __init__(self, out, keep):
        self._out, self._keep, self._host = out, keep, None

    def get(self):
        if self._host is None:
            self._host = self._out.cpu().numpy()          # the only synchronisation of the call
            self._keep = None
        return self._host[:, 0].copy(), self._host[:, 1].copy()


def image_metrics_async(gt_u8, pred_u8):
    """Enqueue the metric kernels on torch's current stream and return a PendingMetrics; nothing waits for the device."""
    import torch
    gt, pred = _u8(gt_u8, 'gt_u8'), _u8(pred_u8, 'pred_u8')
    if gt.shape != pred.shape:
        raise L.NerfppError('gt_u8 %s and pred_u8 %s differ in shape' % (tuple(gt.shape), tuple(pred.shape)))
    if gt.device != pred.device:
        raise L.NerfppError('gt_u8 and pred_u8 live on different devices')
    F, H, W = (int(v) for v in gt.shape[:3])
    nbytes = workspace_bytes(F, H, W)
    with torch.cuda.device(gt.device):
        key = (gt.device.index, F, H, W)
        ws = _workspaces.get(key)
        if ws is None:
            _workspaces.clear()                           # one shape at a time: a test split has one frame size
            ws = _workspaces[key] = torch.empty(nbytes // 8, dtype=torch.float64, device=gt.device)
        out = torch.empty((F, 2), dtype=torch.float64, device=gt.device)
        stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        L.check(L.lib().nerfpp_image_metrics_u8(stream, F, H, W, gt.data_ptr(), pred.data_ptr(), ws.data_ptr(), out.data_ptr()),
                'nerfpp_image_metrics_u8')
    return PendingMetrics(out, (gt, pred))


def image_metrics(gt_u8, pred_u8):
    """(ssim [F], psnr8 [F]) float64 numpy arrays of uint8 device tensors [F, H, W, 3] (or one frame [H, W, 3]): `gt_u8` the
    ground-truth bytes, `pred_u8` the very bytes written to the PNG.  One launch for the batch, one synchronisation when the
    values are read."""
    return image_metrics_async(gt_u8, pred_u8).get()


def to_bytes_nearest(img01):
    """uint8 of a float image in [0, 1], to nearest: the exact inverse of the loaders' `byte / 255`, i.e. the ground-truth
    file's own bytes for a frame that was read from disk."""
    return np.rint(np.clip(np.asarray(img01, np.float64), 0., 1.) * 255.).astype(np.uint8)

"""SSIM and 8-bit PSNR of finished frames on the device: the image columns of the paper's tables.

The reference scores its runs with utils/eval.py:45-60, which re-reads the written PNGs and calls scikit-image's
`structural_similarity(gt, pred, data_range=255, multichannel=True)` and `peak_signal_noise_ratio(gt, pred, data_range=255)`.
`image_metrics` computes the same two numbers from the same bytes with one launch of nerfpp_image_metrics_u8
(include/nerfpp_hip.h) for a whole test split: exact integer window sums, float64 S, no atomics -- bit-reproducible.
There is no host path here: without libnerfpp_hip.so and a device the call raises.
"""
import numpy as np

from . import _ctypes_util as U
from . import _lib as L


def workspace_bytes(n_frames, H, W):
    """Size of the call's scratch buffer; raises NerfppError for sizes the library rejects (H < 7, W < 7).  Needs no GPU."""
    return U.size(L.lib().nerfpp_image_metrics_workspace_bytes(int(n_frames), int(H), int(W)),
                  lambda: L.lib().nerfpp_last_error().decode('utf-8', 'replace'), L.NerfppError)


_workspaces = U.Workspaces(workspace_bytes, 1)            # one shape at a time: a test split has one frame size


def _host(tensors):
    rows = tensors['rows'].cpu().numpy()                  # the only synchronisation of the call
    return rows[:, 0].copy(), rows[:, 1].copy()


def image_metrics_async(gt_u8, pred_u8):
    """Enqueue the metric kernels on torch's current stream and return a Pending (`.tensors['rows']`: float64 [F, 2]) whose
    `.get()` is (ssim [F], psnr8 [F]); nothing waits for the device."""
    import torch
    gt, pred = U.u8_pair(gt_u8, pred_u8, L.NerfppError, 'image_metrics')
    F, H, W = (int(v) for v in gt.shape[:3])
    with torch.cuda.device(gt.device):
        ws = _workspaces.buffer(gt.device, F, H, W)
        out = torch.empty((F, 2), dtype=torch.float64, device=gt.device)
        L.check(L.lib().nerfpp_image_metrics_u8(U.stream(), F, H, W, U.p(gt), U.p(pred), U.p(ws), U.p(out)), 'nerfpp_image_metrics_u8')
    return U.Pending({'rows': out}, (gt, pred, ws), _host)


def image_metrics(gt_u8, pred_u8):
    """(ssim [F], psnr8 [F]) float64 numpy arrays of uint8 device tensors [F, H, W, 3] (or one frame [H, W, 3]): `gt_u8` the
    ground-truth bytes, `pred_u8` the very bytes written to the PNG.  One launch for the batch, one synchronisation when the
    values are read."""
    return image_metrics_async(gt_u8, pred_u8).get()


def to_bytes_nearest(img01):
    """uint8 of a float image in [0, 1], to nearest: the exact inverse of the loaders' `byte / 255`, i.e. the ground-truth
    file's own bytes for a frame that was read from disk."""
    return np.rint(np.clip(np.asarray(img01, np.float64), 0., 1.) * 255.).astype(np.uint8)

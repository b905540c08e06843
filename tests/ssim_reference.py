"""numpy statement of the image metrics of nerfpp_image_metrics_u8 (include/nerfpp_hip.h): what the reference's
utils/eval.py:45-60 computes through scikit-image on the written PNGs,

    structural_similarity(gt, pred, data_range=255, multichannel=True)     # defaults: uniform 7 x 7 window, sample covariance
    peak_signal_noise_ratio(gt, pred, data_range=255)

numpy only (the suite must not need scipy or scikit-image).  The inputs are bytes, so the five 7 x 7 window sums are formed as
exact integers from 2-D cumulative sums; the float64 expression below is scikit-image's, term for term
(skimage/metrics/_structural_similarity.py).  Only the windows that lie wholly inside the image count: scikit-image crops
(win_size - 1) // 2 = 3 pixels from every edge of S before the mean, so its border mode never reaches the result.
"""
import numpy as np

WIN = 7
NP = WIN * WIN
K1, K2, R = 0.01, 0.03, 255.0
C1, C2 = (K1 * R) ** 2, (K2 * R) ** 2
COV_NORM = NP / (NP - 1.0)


def box_sums(a):
    """exact int64 sums of `a` [H, W] over every whole WIN x WIN window: [H-6, W-6]"""
    c = np.zeros((a.shape[0] + 1, a.shape[1] + 1), np.int64)
    c[1:, 1:] = np.cumsum(np.cumsum(a.astype(np.int64), 0), 1)
    return c[WIN:, WIN:] - c[:-WIN, WIN:] - c[WIN:, :-WIN] + c[:-WIN, :-WIN]


def ssim_map(x, y):
    """S [H-6, W-6] float64 of one channel pair (uint8 [H, W])"""
    x, y = x.astype(np.int64), y.astype(np.int64)
    ux, uy = box_sums(x) / float(NP), box_sums(y) / float(NP)
    uxx, uyy, uxy = box_sums(x * x) / float(NP), box_sums(y * y) / float(NP), box_sums(x * y) / float(NP)
    vx = COV_NORM * (uxx - ux * ux)
    vy = COV_NORM * (uyy - uy * uy)
    vxy = COV_NORM * (uxy - ux * uy)
    A1, A2 = 2 * ux * uy + C1, 2 * vxy + C2
    B1, B2 = ux ** 2 + uy ** 2 + C1, vx + vy + C2
    return (A1 * A2) / (B1 * B2)


def _check(gt, pred):
    gt, pred = np.asarray(gt), np.asarray(pred)
    if gt.dtype != np.uint8 or pred.dtype != np.uint8:
        raise TypeError('uint8 images expected, got %s and %s' % (gt.dtype, pred.dtype))
    if gt.shape != pred.shape or gt.ndim != 3 or gt.shape[2] != 3:
        raise ValueError('two [H, W, 3] images of one size expected, got %s and %s' % (gt.shape, pred.shape))
    return gt, pred


def ssim(gt, pred):
    """float64 SSIM of two uint8 [H, W, 3] images: mean over the channels of the mean of S"""
    gt, pred = _check(gt, pred)
    if gt.shape[0] < WIN or gt.shape[1] < WIN:
        raise ValueError('win_size exceeds image extent: %s' % (gt.shape,))
    return float(np.mean([ssim_map(gt[..., c], pred[..., c]).mean(dtype=np.float64) for c in range(3)]))


def psnr8(gt, pred):
    """10 log10(255^2 / mse) over all H W 3 values; inf for identical images"""
    gt, pred = _check(gt, pred)
    d = gt.astype(np.int64) - pred.astype(np.int64)
    err = int((d * d).sum())
    if err == 0:
        return float('inf')
    return float(10 * np.log10((R ** 2) / (err / float(d.size))))


def image_metrics(gt, pred):
    """(ssim [F], psnr8 [F]) float64 of uint8 [F, H, W, 3] (or [H, W, 3]) arrays: the call face of
    outdoor_nerf_depth_amd.image_metrics.image_metrics"""
    gt, pred = np.asarray(gt), np.asarray(pred)
    if gt.ndim == 3:
        gt, pred = gt[None], pred[None]
    return (np.array([ssim(g, p) for g, p in zip(gt, pred)], np.float64),
            np.array([psnr8(g, p) for g, p in zip(gt, pred)], np.float64))

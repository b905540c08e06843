"""Depth-error metrics on the device: the depth columns of the paper's tables.  ctypes binding of libdepthmetrics_hip.so
(include/depthmetrics_hip.h).

The reference's evaluators (nerfplusplus/ddp_train_nerf.py:581-600, mipnerf360/eval.py:129-144) compute the standard KITTI depth
metrics of every test frame -- RMSE, AbsRel, SqRel, the mean absolute difference, RMSE of the logarithms and the threshold
ratios a1 / a2 / a3 -- over the pixels with 1e-3 < gt < 80 m, predictions clipped to [1e-3, 80] m, and write only the first two.
`depth_metrics_async` computes all of them for a split [F, H, W] in one call, and the absolute-error map the MipNeRF-360
evaluators save as absrel_{idx}.npy when asked.  The definition is DESIGN.md 8.5 (restated as code in
tests/depth_metrics_reference.py).

Everything is enqueued on torch's current stream and nothing synchronises until the numbers are read.  torch only allocates.
There is no host path: without libdepthmetrics_hip.so and a device every call raises.
"""
import ctypes as C
import os

from . import _ctypes_util as U

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get('DEPTHMETRICS_HIP_LIB') or os.path.join(_HERE, 'libdepthmetrics_hip.so')
OK = 0
ABI_VERSION = 1
MAX_FRAMES = 65535
MAX_PIXELS = 1 << 28
WG_PIXELS = 2048                  # DEPTHMETRICS_WG_PIXELS: a frame of more pixels than this is reduced by two or more workgroups
METRIC_NAMES = ('n_valid', 'rmse', 'absrel', 'sqrel', 'absdiff', 'rmse_log', 'a1', 'a2', 'a3')
DEPTH_METRICS_HELP = ('also score the rendered depth of every test frame that has ground-truth depth with the whole KITTI depth-metric '
                      'set on the device, in one call per split: n_valid, rmse, absrel, sqrel, absdiff, rmse_log and the threshold '
                      'ratios a1 / a2 / a3 (max(gt / pred, pred / gt) < 1.25, 1.25^2, 1.25^3) over 1e-3 < gt < 80 m with predictions '
                      'clipped to [1e-3, 80] m -> %s (per image, then the mean)')

_fp = C.c_void_p
# every symbol include/depthmetrics_hip.h declares: name -> (restype, argtypes)
SYMBOLS = {
    'depthmetrics_last_error': (C.c_char_p, []),
    'depthmetrics_abi_version': (C.c_int, []),
    'depthmetrics_workspace_bytes': (C.c_int64, [C.c_int, C.c_int64]),
    'depthmetrics_frames': (C.c_int, [_fp, C.c_int, C.c_int64, _fp, _fp, C.c_double, _fp, _fp, _fp]),
}

_lib = None


class DepthMetricsError(RuntimeError):
    pass


def lib():
    """The loaded library with typed prototypes.  Raises if it has not been built."""
    global _lib
    if _lib is None:
        _lib = U.load(LIB_PATH, 'libdepthmetrics_hip.so', SYMBOLS, 'depthmetrics_abi_version', ABI_VERSION, DepthMetricsError,
                      ' (hipcc --offload-arch=gfx950). There is no CPU fallback for the depth metrics.')
    return _lib


def last_error():
    return lib().depthmetrics_last_error().decode('utf-8', 'replace')


check = U.checker(lib, 'depthmetrics_last_error', DepthMetricsError, 'depthmetrics call')


def workspace_bytes(n_frames, n_pixels):
    """Size of the scratch buffer of a call on n_frames frames of n_pixels pixels; raises DepthMetricsError for sizes the library
    rejects (n_frames outside 1 .. 65535, n_pixels outside 1 .. 2^28).  Needs no GPU."""
    return U.size(lib().depthmetrics_workspace_bytes(int(n_frames), int(n_pixels)), last_error, DepthMetricsError)


_workspaces = U.Workspaces(workspace_bytes, 2)


def _frames(t, name):
    """t as float32 device [F, H, W]; one frame [H, W] gains the batch axis"""
    t = U.device_tensor(t, name, 'float32', DepthMetricsError, 'expected a CUDA/HIP float32 tensor (the depth metrics have no CPU path)',
                        'torch.float32')
    return U.contiguous(U.batched(t, name, 3, DepthMetricsError, '[F, H, W] or [H, W]'), name, DepthMetricsError)


def _host(tensors):
    rows = tensors['rows'].cpu().numpy()                  # the only synchronisation
    host = {name: rows[:, k].copy() for k, name in enumerate(METRIC_NAMES)}
    if 'err_map' in tensors:
        host['err_map'] = tensors['err_map'].cpu().numpy()
    return host


def depth_metrics_async(pred, gt, scale, err_map=False):
    """Pending of the nine metrics per frame (and the absolute-error map with err_map=True) of float32 device tensors pred, gt
    [F, H, W] (or [H, W]) in scene units; metres = value / float32(scale).  Enqueue only.  `.tensors`: 'rows' (float64 [F, 9] in
    METRIC_NAMES' order) and, when asked, 'err_map' (float32 [F, H, W]); `.get()`: {name: float64 numpy [F]} for METRIC_NAMES
    plus 'err_map'."""
    import torch
    pred, gt = _frames(pred, 'pred'), _frames(gt, 'gt')
    if pred.shape != gt.shape:
        raise DepthMetricsError('pred %s and gt %s: shapes differ' % (tuple(pred.shape), tuple(gt.shape)))
    if pred.device != gt.device:
        raise DepthMetricsError('pred on %s and gt on %s: devices differ' % (pred.device, gt.device))
    F, H, W = (int(v) for v in pred.shape)
    n = H * W
    with torch.cuda.device(pred.device):
        ws = _workspaces.buffer(pred.device, F, n)
        out = {'rows': torch.empty((F, len(METRIC_NAMES)), dtype=torch.float64, device=pred.device)}
        if err_map:
            out['err_map'] = torch.empty((F, H, W), dtype=torch.float32, device=pred.device)
        check(lib().depthmetrics_frames(U.stream(), F, n, U.p(pred), U.p(gt), float(scale), U.p(ws), U.p(out['rows']),
                                        U.p(out.get('err_map'))), 'depthmetrics_frames')
    return U.Pending(out, (pred, gt, ws), _host)


def depth_metrics(pred, gt, scale, err_map=False):
    """{name: float64 numpy [F]} (and 'err_map': float32 [F, H, W]): the blocking form of depth_metrics_async"""
    return depth_metrics_async(pred, gt, scale, err_map).get()

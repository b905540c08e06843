"""The distortion and opacity regularisers on the weights along a ray, on the device.  ctypes binding of librayreg_hip.so
(include/rayreg_hip.h).

Where no depth prior speaks, nothing else in the NeRF++ path constrains how weight is spread along a ray.  `ray_reg` puts two terms
on the foreground weights w [n, S] of one cascade level, with the ascending sample positions z [n, S] and the rays' bounds lo, hi [n]:

    distortion  (1 / n) sum over rays with hi > lo of  sum_ij w_i w_j |u_i - u_j| + (1/3) sum_i w_i^2 d_i
                u, d: the midpoints and widths of the intervals [z_s, z_{s+1}] (the last one ends at hi), normalised to [lo, hi]
    opacity     (1 / n) sum over rays of  -o log o,   o = sum_s w_s + 1e-10

with gradients to the weights (positions receive none).  The definition is DESIGN.md 9.11 (restated as code in
tests/ray_reg_reference.py).

One level per call, enqueued on torch's current stream; nothing synchronises.  torch only allocates.  There is no host path: without
librayreg_hip.so and a device `ray_reg` raises.
"""
import ctypes as C
import math
import os

from . import _ctypes_util as U

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get('RAYREG_HIP_LIB') or os.path.join(_HERE, 'librayreg_hip.so')
OK = 0
ABI_VERSION = 1
MAX_RAYS = 1 << 20
MAX_SAMPLES = 1024

_fp = C.c_void_p
# every symbol include/rayreg_hip.h declares: name -> (restype, argtypes)
SYMBOLS = {
    'rayreg_last_error': (C.c_char_p, []),
    'rayreg_abi_version': (C.c_int, []),
    'rayreg_workspace_bytes': (C.c_int64, [C.c_int]),
    'rayreg_level': (C.c_int, [_fp, C.c_int, C.c_int, _fp, _fp, _fp, _fp, C.c_double, C.c_double, _fp, _fp, _fp, _fp, _fp]),
}

_lib = None


class RayRegError(RuntimeError):
    pass


def lib():
    """The loaded library with typed prototypes.  Raises if it has not been built."""
    global _lib
    if _lib is None:
        _lib = U.load(LIB_PATH, 'librayreg_hip.so', SYMBOLS, 'rayreg_abi_version', ABI_VERSION, RayRegError,
                      ' (hipcc --offload-arch=gfx950). There is no CPU fallback for the ray regularisers.')
    return _lib


def last_error():
    return lib().rayreg_last_error().decode('utf-8', 'replace')


check = U.checker(lib, 'rayreg_last_error', RayRegError, 'rayreg call')


def workspace_bytes(n):
    """Size of the scratch buffer of a call; raises RayRegError for what the library rejects (n outside 1 .. 2^20).  Needs no GPU."""
    return U.size(lib().rayreg_workspace_bytes(int(n)), last_error, RayRegError)


# a training run calls with one n per level, step after step: (device, n) -> the scratch buffer.  Calls of one stream are ordered, so
# the next call may overwrite it.
_workspaces = U.Workspaces(workspace_bytes, held=4)


def _tensor(t, name, shape, dev):
    return U.inplace_f32(t, name, shape, dev, RayRegError, 'ray-regulariser', 'weights')


def _lambda(v, name):
    v = float(v)
    if not math.isfinite(v) or v < 0.0:
        raise RayRegError('%s = %r: expected a finite value that is not negative' % (name, v))
    return v


def ray_reg(weights, z, lo, hi, lambda_distortion, lambda_opacity, g_weights=None, fold_total=None):
    """Both regularisers of one level: weights [n, S], z [n, S] ascending sample positions, lo / hi [n] the rays' bounds (a ray with
    hi <= lo gets no distortion term): float32 device tensors, n in 1 .. 2^20, S in 1 .. 1024.  lambda_distortion, lambda_opacity:
    finite, not negative, at least one positive; a lambda of 0 removes its term and its value is 0.  g_weights: a float32 device
    tensor [n, S] or None; (lambda_distortion * d distortion + lambda_opacity * d opacity) / d weights is ACCUMULATED, a row that
    receives no term keeps its bits.  fold_total: a one-element float32 device tensor or None, updated on the device after the
    values: fold_total += lambda_distortion * distortion + lambda_opacity * opacity.
    Returns (values [2] = (distortion, opacity), stats [1] = (rays with hi > lo)), float32 device tensors.  Enqueue only."""
    import torch
    if not isinstance(weights, torch.Tensor) or weights.dim() != 2:
        raise RayRegError('weights: expected a float32 device tensor [n, S], got %s' % (tuple(getattr(weights, 'shape', ())),))
    n, S = int(weights.shape[0]), int(weights.shape[1])
    if not 1 <= n <= MAX_RAYS:
        raise RayRegError('weights: %d rays, expected 1 .. 2^20 (the regularisers are built for training batches)' % n)
    if not 1 <= S <= MAX_SAMPLES:
        raise RayRegError('weights: %d samples per ray, expected 1 .. %d' % (S, MAX_SAMPLES))
    dev = weights.device if weights.is_cuda else None
    _tensor(weights, 'weights', (n, S), dev)
    _tensor(z, 'z', (n, S), dev)
    _tensor(lo, 'lo', (n,), dev)
    _tensor(hi, 'hi', (n,), dev)
    if g_weights is not None:
        _tensor(g_weights, 'g_weights', (n, S), dev)
    if fold_total is not None:
        _tensor(fold_total, 'fold_total', tuple(getattr(fold_total, 'shape', ())), dev)
        if fold_total.numel() != 1:
            raise RayRegError('fold_total: expected a one-element float32 tensor, got shape %s' % (tuple(fold_total.shape),))
    lambda_distortion = _lambda(lambda_distortion, 'lambda_distortion')
    lambda_opacity = _lambda(lambda_opacity, 'lambda_opacity')
    if lambda_distortion == 0.0 and lambda_opacity == 0.0:
        raise RayRegError('lambda_distortion and lambda_opacity are both 0: there is nothing to compute')
    with torch.cuda.device(dev):
        ws = _workspaces.buffer(dev, n)
        out = torch.empty(3, device=dev)
        values, stats = out[:2], out[2:]
        check(lib().rayreg_level(U.stream(), n, S, U.p(weights), U.p(z), U.p(lo), U.p(hi), lambda_distortion, lambda_opacity,
                                 U.p(g_weights), U.p(ws), U.p(values), U.p(stats), U.p(fold_total)), 'rayreg_level')
    return values, stats

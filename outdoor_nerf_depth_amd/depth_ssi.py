"""The scale-and-shift-invariant depth loss ('ssi') on the device.  ctypes binding of libdepthssi_hip.so (include/depthssi_hip.h).

A monocular depth prior is known up to one scale and one shift per image, so a loss in absolute scene units ('mse', 'l1', 'kl',
'urf') pulls the geometry to a wrong scale.  `ssi_loss` is the loss of MiDaS / MonoSDF: per group of rays (= image) it fits the
scale w and the shift q that best map the rendered depth onto the prior and penalises what is left,

    L = (1 / D) sum over fitted groups, over their supervised rays, of (w d + q - p)^2,      dL/dd = 2 w (w d + q - p) / D

with D = n ('all', the MipNeRF-360 path's mean over all rays) or max(N_sup, 1) ('supervised', the NeRF++ path's mean over the
mask).  A group with fewer than min_rays supervised rays, or whose rendered depth is constant, is not fitted and earns nothing.
The definition is DESIGN.md 9.8 (restated as code in tests/depth_ssi_reference.py).

All levels of a step go through one call, enqueued on torch's current stream; nothing synchronises.  torch only allocates.  There
is no host path: without libdepthssi_hip.so and a device `ssi_loss` raises.
"""
import ctypes as C
import os

from . import _ctypes_util as U

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get('DEPTHSSI_HIP_LIB') or os.path.join(_HERE, 'libdepthssi_hip.so')
OK = 0
ABI_VERSION = 1
MAX_RAYS = 1 << 20
MAX_GROUPS = 65535
MAX_LEVELS = 8
NORMS = {'all': 0, 'supervised': 1}
FOLD_KEYS = U.FOLD_KEYS
DEFAULT_MIN_RAYS = 8

_fp = C.c_void_p
_fpp = C.POINTER(C.c_void_p)
# every symbol include/depthssi_hip.h declares: name -> (restype, argtypes)
SYMBOLS = {
    'depthssi_last_error': (C.c_char_p, []),
    'depthssi_abi_version': (C.c_int, []),
    'depthssi_workspace_bytes': (C.c_int64, [C.c_int, C.c_int]),
    'depthssi_levels': (C.c_int, [_fp, C.c_int, C.c_int, _fpp, _fp, _fp, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_float), _fpp,
                                  _fp, _fp, _fp, _fp, _fp, _fp, _fp, _fp]),
}

_lib = None


class DepthSsiError(RuntimeError):
    pass


def lib():
    """The loaded library with typed prototypes.  Raises if it has not been built."""
    global _lib
    if _lib is None:
        _lib = U.load(LIB_PATH, 'libdepthssi_hip.so', SYMBOLS, 'depthssi_abi_version', ABI_VERSION, DepthSsiError,
                      ' (hipcc --offload-arch=gfx950). There is no CPU fallback for the ssi depth loss.')
    return _lib


def last_error():
    return lib().depthssi_last_error().decode('utf-8', 'replace')


check = U.checker(lib, 'depthssi_last_error', DepthSsiError, 'depthssi call')


def workspace_bytes(n_levels, n_groups):
    """Size of the scratch buffer of a call; raises DepthSsiError for sizes the library rejects (n_levels outside 1 .. 8, n_groups
    outside 1 .. 65535).  Needs no GPU."""
    nbytes = lib().depthssi_workspace_bytes(int(n_levels), int(n_groups))
    if nbytes < 0:
        raise DepthSsiError(last_error())
    return nbytes


def _vector(t, name, n, dev):
    return U.inplace_f32(t, name, (n,), dev, DepthSsiError, 'ssi', 'pred_levels[0]')


def _group(group, n, dev):
    """(tensor, element stride) of the rays' group ids: an int32 device vector [n], or a pixel table [n, 3] (frame, x, y) as the
    MipNeRF-360 sampler returns it, whose frame column is read in place"""
    import torch
    if not isinstance(group, torch.Tensor) or not group.is_cuda:
        raise DepthSsiError('group: expected a CUDA/HIP int32 tensor (the ssi depth loss has no CPU path)')
    if group.dtype != torch.int32 or not group.is_contiguous():
        raise DepthSsiError('group: expected a contiguous torch.int32 tensor, got %s with strides %s' % (group.dtype, tuple(group.stride())))
    if group.device != dev:
        raise DepthSsiError('group on %s, pred_levels[0] on %s: devices differ' % (group.device, dev))
    if tuple(group.shape) == (n,):
        return group, 1
    if tuple(group.shape) == (n, 3):
        return group, 3
    raise DepthSsiError('group: expected shape (%d,) or (%d, 3), got %s' % (n, n, tuple(group.shape)))


def ssi_loss(pred_levels, prior, group=None, n_groups=1, min_rays=DEFAULT_MIN_RAYS, norm='all', scale=None, grads=None, fold=None):
    """The ssi loss of every level's rendered depth pred_levels[l] [n] against one prior [n] (> 0 = supervised), float32 device
    tensors.  group: the rays' group ids (int32 [n], or the sampler's pix [n, 3]: frame column) in 0 .. n_groups - 1, ids outside
    count as unsupervised; None = one group.  norm: 'all' (D = n) or 'supervised' (D = max(supervised rays, 1)).  scale: the
    levels' weights (default 1 each).  grads: one float32 [n] device tensor or None per level; scale[l] * dL/dd is ACCUMULATED,
    entries of unsupervised rays and of groups that are not fitted keep their bits.  fold: {'total' | 'last' | 'others' | 'n_sup':
    one-element float32 device tensor}, updated on the device after the loss: total += sum_l scale[l] * value[l], last = the last
    level's value, others = the sum of the other levels' values, n_sup = the number of supervised rays.
    Returns (values [L], fit [L, n_groups, 4] = (w, q, N, fitted), stats [L, 2] = (supervised rays, supervised rays in fitted
    groups)), float32 device tensors.  Enqueue only."""
    import torch
    pred_levels = list(pred_levels)
    L, n, dev = U.level_counts(pred_levels, 'pred_levels', 1, 'vector [n]', MAX_LEVELS, MAX_RAYS, DepthSsiError)
    pred_levels = [_vector(t, 'pred_levels[%d]' % k, n, dev) for k, t in enumerate(pred_levels)]
    prior = _vector(prior, 'prior', n, dev)
    n_groups = int(n_groups)
    if not 1 <= n_groups <= MAX_GROUPS:
        raise DepthSsiError('n_groups = %d, expected 1 .. %d' % (n_groups, MAX_GROUPS))
    if group is None and n_groups != 1:
        raise DepthSsiError('n_groups = %d without `group`: rays without ids form one group' % n_groups)
    g, g_stride = _group(group, n, dev) if group is not None else (None, 1)
    if norm not in NORMS:
        raise DepthSsiError("norm %r: 'all' (mean over all rays) or 'supervised' (mean over the supervised rays)" % (norm,))
    if int(min_rays) < 1:
        raise DepthSsiError('min_rays = %r, expected at least 1' % (min_rays,))
    scale = U.level_scale(scale, L, DepthSsiError)
    if grads is not None:
        grads = list(grads)
        if len(grads) != L:
            raise DepthSsiError('grads: %d entries for %d levels' % (len(grads), L))
        grads = [None if t is None else _vector(t, 'grads[%d]' % k, n, dev) for k, t in enumerate(grads)]
    fold = U.fold_dict(fold, dev, DepthSsiError)
    with torch.cuda.device(dev):
        ws = torch.empty(workspace_bytes(L, n_groups) // 8, dtype=torch.float64, device=dev)
        values = torch.empty(L, device=dev)
        fit = torch.empty((L, n_groups, 4), device=dev)
        stats = torch.empty((L, 2), device=dev)
        check(lib().depthssi_levels(U.stream(), n, L, U.ptr_array(pred_levels), U.p(prior), U.p(g), g_stride, n_groups, int(min_rays),
                                    NORMS[norm], (C.c_float * L)(*scale), U.ptr_array(grads), U.p(ws),
                                    U.p(values), U.p(fit), U.p(stats), *[U.p(fold.get(k)) for k in FOLD_KEYS]), 'depthssi_levels')
    return values, fit, stats

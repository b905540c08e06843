"""The uncertainty-aware Gaussian negative-log-likelihood depth loss ('gnll') on the device.  ctypes binding of
libdepthgnll_hip.so (include/depthgnll_hip.h).

Every other depth loss trusts each prior pixel equally.  `gnll_loss` is the loss of Dense Depth Priors for NeRF (Roessle et al.),
for priors that come with a per-pixel standard deviation (a completion network's uncertainty, a stereo confidence): the rendered
depth D of a ray is a Gaussian whose variance V = sum w (x - D)^2 + 1e-5 is the spread of the ray's weights, and a supervised ray
(p > 0, sigma > 0, p < limit) is penalised only while |D - p| > sigma or V > sigma^2,

    value = (1 / n) sum over those rays of 0.5 (log Vc + (D - p)^2 / Vc),      Vc = max(V, 1e-3)

with gradients to D and to the weights (the gate is a constant, positions receive none).  The definition is DESIGN.md 9.9
(restated as code in tests/depth_gnll_reference.py).  The value can be negative.

All levels of a step go through one call, enqueued on torch's current stream; nothing synchronises.  torch only allocates.  There
is no host path: without libdepthgnll_hip.so and a device `gnll_loss` raises.
"""
import ctypes as C
import os

from . import _ctypes_util as U

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get('DEPTHGNLL_HIP_LIB') or os.path.join(_HERE, 'libdepthgnll_hip.so')
OK = 0
ABI_VERSION = 1
MAX_RAYS = 1 << 20
MAX_LEVELS = 8
MAX_SAMPLES = 1024
STATS_ROW = 3
FOLD_KEYS = U.FOLD_KEYS

_fp = C.c_void_p
_fpp = C.POINTER(C.c_void_p)
# every symbol include/depthgnll_hip.h declares: name -> (restype, argtypes)
SYMBOLS = {
    'depthgnll_last_error': (C.c_char_p, []),
    'depthgnll_abi_version': (C.c_int, []),
    'depthgnll_workspace_bytes': (C.c_int64, [C.c_int, C.c_int]),
    'depthgnll_levels': (C.c_int, [_fp, C.c_int, C.c_int, C.POINTER(C.c_int), C.c_int, _fpp, _fpp, _fpp, _fp, _fp, _fp,
                                   C.POINTER(C.c_float), _fpp, _fpp, _fp, _fp, _fp, _fp, _fp, _fp, _fp]),
}

_lib = None


class DepthGnllError(RuntimeError):
    pass


def lib():
    """The loaded library with typed prototypes.  Raises if it has not been built."""
    global _lib
    if _lib is None:
        _lib = U.load(LIB_PATH, 'libdepthgnll_hip.so', SYMBOLS, 'depthgnll_abi_version', ABI_VERSION, DepthGnllError,
                      ' (hipcc --offload-arch=gfx950). There is no CPU fallback for the gnll depth loss.')
    return _lib


def last_error():
    return lib().depthgnll_last_error().decode('utf-8', 'replace')


check = U.checker(lib, 'depthgnll_last_error', DepthGnllError, 'depthgnll call')


def workspace_bytes(n_levels, n):
    """Size of the scratch buffer of a call; raises DepthGnllError for sizes the library rejects (n_levels outside 1 .. 8, n outside
    1 .. 2^20).  Needs no GPU."""
    nbytes = lib().depthgnll_workspace_bytes(int(n_levels), int(n))
    if nbytes < 0:
        raise DepthGnllError(last_error())
    return nbytes


def _tensor(t, name, shape, dev):
    return U.inplace_f32(t, name, shape, dev, DepthGnllError, 'gnll', 'weights[0]')


def gnll_loss(weights, x, pred_levels, prior, prior_std, limit=None, edges=False, scale=None, g_weights=None, g_pred=None, fold=None):
    """The gnll loss of every level against one prior: weights[l] [n, S_l], x[l] [n, S_l] sample positions (edges=False) or
    [n, S_l + 1] interval edges (edges=True: the position is the interval's midpoint, formed in float32), pred_levels[l] [n] the
    rendered depth, prior / prior_std [n] (a ray with prior <= 0 or prior_std <= 0 is unsupervised), limit [n] or None (a ray with
    prior >= limit is unsupervised): float32 device tensors.  scale: the levels' weights (default 1 each).  g_weights / g_pred:
    one float32 device tensor [n, S_l] / [n] or None per level; scale[l] * gradient is ACCUMULATED, entries of rays the gate does
    not let through keep their bits.  fold: {'total' | 'last' | 'others' | 'n_sup': one-element float32 device tensor}, updated on
    the device after the loss: total += sum_l scale[l] * value[l], last = the last level's value, others = the sum of the other
    levels' values, n_sup = the number of supervised rays.
    Returns (values [L], stats [L, 3] = (supervised rays, gated rays, gated rays with V < 1e-3)), float32 device tensors.
    Enqueue only."""
    import torch
    weights, x, pred_levels = list(weights), list(x), list(pred_levels)
    L, n, dev = U.level_counts(weights, 'weights', 2, 'tensor [n, S]', MAX_LEVELS, MAX_RAYS, DepthGnllError)
    for name, lst in (('x', x), ('pred_levels', pred_levels)):
        if len(lst) != L:
            raise DepthGnllError('%s: %d entries for %d levels' % (name, len(lst), L))
    S = []
    for k, t in enumerate(weights):
        if not isinstance(t, torch.Tensor) or t.dim() != 2 or not 1 <= int(t.shape[1]) <= MAX_SAMPLES:
            raise DepthGnllError('weights[%d]: expected a float32 device tensor [%d, S] with S in 1 .. %d, got shape %s'
                                 % (k, n, MAX_SAMPLES, tuple(getattr(t, 'shape', ()))))
        S.append(int(t.shape[1]))
        _tensor(t, 'weights[%d]' % k, (n, S[k]), dev)
        _tensor(x[k], 'x[%d]' % k, (n, S[k] + 1 if edges else S[k]), dev)
        _tensor(pred_levels[k], 'pred_levels[%d]' % k, (n,), dev)
    _tensor(prior, 'prior', (n,), dev)
    _tensor(prior_std, 'prior_std', (n,), dev)
    if limit is not None:
        _tensor(limit, 'limit', (n,), dev)
    scale = U.level_scale(scale, L, DepthGnllError)
    for name, lst in (('g_weights', g_weights), ('g_pred', g_pred)):
        if lst is not None and len(list(lst)) != L:
            raise DepthGnllError('%s: %d entries for %d levels' % (name, len(list(lst)), L))
    if g_weights is not None:
        g_weights = [None if t is None else _tensor(t, 'g_weights[%d]' % k, (n, S[k]), dev) for k, t in enumerate(g_weights)]
    if g_pred is not None:
        g_pred = [None if t is None else _tensor(t, 'g_pred[%d]' % k, (n,), dev) for k, t in enumerate(g_pred)]
    fold = U.fold_dict(fold, dev, DepthGnllError)
    arr = U.ptr_array
    with torch.cuda.device(dev):
        ws = torch.empty(workspace_bytes(L, n) // 8, dtype=torch.float64, device=dev)
        values = torch.empty(L, device=dev)
        stats = torch.empty((L, STATS_ROW), device=dev)
        check(lib().depthgnll_levels(U.stream(), n, L, (C.c_int * L)(*S), int(bool(edges)), arr(weights), arr(x), arr(pred_levels),
                                     U.p(prior), U.p(prior_std), U.p(limit), (C.c_float * L)(*scale), arr(g_weights), arr(g_pred),
                                     U.p(ws), U.p(values), U.p(stats), *[U.p(fold.get(k)) for k in FOLD_KEYS]), 'depthgnll_levels')
    return values, stats

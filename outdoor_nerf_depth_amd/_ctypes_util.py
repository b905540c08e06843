"""What the ctypes bindings of this package's HIP libraries share: the loader, the return-code check and the tensor -> argument
helpers.  (torch is imported where it is used: lpips.py and color_correct.py answer their host-side questions without it.)"""
import ctypes as C
import os


def load(path, name, symbols, abi_fn, abi_version, error, how, probe=None):
    """The library at `path` with typed prototypes (symbols: name -> (restype, argtypes)), or `error`: a missing file (`how` says
    how to build it and what does not exist instead), a stale one (probe(handle) raises; a missing symbol is an AttributeError) or
    another ABI version."""
    if not os.path.exists(path):
        raise error('%s not found at %s -- build it with `python -c "import __graft_entry__ as g; g.build()"`%s' % (name, path, how))
    # PyTorch-ROCm ships its own libamdhip64; device pointers and streams only make sense inside ONE HIP runtime, so torch's
    # must be the copy already in the process when the library resolves its libamdhip64 dependency (whichever is loaded
    # first wins the SONAME).
    import torch  # noqa: F401
    handle = C.CDLL(path)
    if probe is not None:
        probe(handle)
    for sym, (res, args) in symbols.items():
        fn = getattr(handle, sym)
        fn.restype, fn.argtypes = res, args
    if getattr(handle, abi_fn)() != abi_version:
        raise error('%s ABI version mismatch' % name)
    return handle


def checker(lib, last_error, error, default):
    """check(rc, what=''): raise `error` with the library's own message (its `last_error` symbol) for a non-zero return code"""
    def check(rc, what=''):
        if rc != 0:
            raise error('%s failed (code %d): %s' % (what or default, rc, getattr(lib(), last_error)().decode('utf-8', 'replace')))
    return check


def stream():
    import torch
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def p(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def ptr_array(ts):
    """The device pointers of a list of tensors as a C array of void* (None entries are null; None stays None)"""
    if ts is None:
        return None
    return (C.c_void_p * max(1, len(ts)))(*[None if t is None else t.data_ptr() for t in ts])


# ---- what the calls that take every level of a step at once share (depth_ssi.ssi_loss, depth_gnll.gnll_loss, mip360.depth_loss_rays)
FOLD_KEYS = ('total', 'last', 'others', 'n_sup')


def level_counts(levels, name, dim, what, max_levels, max_rays, error):
    """(levels, rays, device or None) of a call whose first per-level list is `levels`, called `name`, of `dim`-dimensional tensors
    (`what` describes one); the counts checked against the library's limits"""
    import torch
    L = len(levels)
    if not 1 <= L <= max_levels:
        raise error('%s: %d levels, expected 1 .. %d' % (name, L, max_levels))
    first = levels[0]
    if not isinstance(first, torch.Tensor) or first.dim() != dim:
        raise error('%s[0]: expected a float32 device %s' % (name, what))
    n = int(first.shape[0])
    if not 1 <= n <= max_rays:
        raise error('%s[0]: %d rays, expected 1 .. 2^20 (the loss is built for training batches)' % (name, n))
    return L, n, first.device if first.is_cuda else None


def is_inplace_f32(t, shape):
    import torch
    return t.is_cuda and t.dtype == torch.float32 and t.is_contiguous() and tuple(t.shape) == tuple(shape)


def inplace_f32(t, name, shape, dev, error, label, anchor):
    """t checked as a contiguous float32 device tensor of `shape` on dev (the device of the tensor called `anchor`).  No copy: the
    gradient buffers are accumulated in place."""
    import torch
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise error('%s: expected a CUDA/HIP float32 tensor (the %s depth loss has no CPU path)' % (name, label))
    if t.dtype != torch.float32:
        raise error('%s: expected torch.float32, got %s' % (name, t.dtype))
    if tuple(t.shape) != tuple(shape) or not t.is_contiguous():
        raise error('%s: expected a contiguous tensor of shape %s, got shape %s with strides %s'
                    % (name, tuple(shape), tuple(t.shape), tuple(t.stride())))
    if dev is not None and t.device != dev:
        raise error('%s on %s, %s on %s: devices differ' % (name, t.device, anchor, dev))
    return t


def level_scale(scale, n_levels, error, message='scale: %d entries for %d levels'):
    """The levels' weights as floats: 1 each by default, one per level"""
    scale = [1.0] * n_levels if scale is None else [float(v) for v in scale]
    if len(scale) != n_levels:
        raise error(message % (len(scale), n_levels))
    return scale


def fold_dict(fold, dev, error):
    """fold checked: {one of FOLD_KEYS: one-element float32 tensor on dev} (None = nothing is folded)"""
    import torch
    fold = dict(fold or {})
    for key, t in fold.items():
        if key not in FOLD_KEYS:
            raise error('fold[%r]: the folds are %s' % (key, ', '.join(FOLD_KEYS)))
        if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.float32 and t.numel() == 1 and t.device == dev):
            raise error('fold[%r]: expected a one-element float32 tensor on %s' % (key, dev))
    return fold


def f32(t, shape=None, error=RuntimeError, fallback='no CPU fallback'):
    """t as a contiguous float32 device tensor (None stays None), of `shape` when one is given"""
    if t is None:
        return None
    if not t.is_cuda:
        raise error('expected a CUDA/HIP tensor (%s)' % fallback)
    t = t.contiguous().float()
    if shape is not None and tuple(t.shape) != tuple(shape):
        raise error('bad tensor shape %s, expected %s' % (tuple(t.shape), tuple(shape)))
    return t

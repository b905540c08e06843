"""What the ctypes bindings of this package's HIP libraries share: the loader, the return-code check, the tensor -> argument
helpers, the depth losses' per-level helpers and, for the evaluator bindings (image_metrics, lpips, color_correct, depth_vis,
depth_metrics, depth_consistency, depth_accumulate, depth_align, depth_complete, depth_mvs, depth_mvs_smooth, depth_points), the pending result, the workspace cache and the tensor checks.  (torch is imported where it
is used: lpips.py and color_correct.py answer their host-side questions without it.)"""
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
    device_tensor(t, name, 'float32', error, 'expected a CUDA/HIP float32 tensor (the %s depth loss has no CPU path)' % label,
                  'torch.float32')
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


# ---- what the evaluator bindings share.  Every check raises the binding's `error`; the words that name a binding are its own.
class Pending(object):
    """Device results of an *_async call: `.tensors` (name -> device tensor, usable by later work on the same stream without
    waiting).  `.get()` synchronises (once) and returns them on the host -- {name: numpy array}, or host(tensors) -- and the same
    object on every later call.  keep: what the queued work reads and nobody else holds -- the inputs (or their contiguous
    copies) and the workspace -- held until the results are read, then dropped."""

    def __init__(self, tensors, keep=None, host=None):
        self.tensors, self._keep, self._to_host, self._host = tensors, keep, host, None

    def get(self):
        if self._host is None:
            if self._to_host is None:
                self._host = {name: t.cpu().numpy() for name, t in self.tensors.items()}     # the only synchronisation
            else:
                self._host = self._to_host(self.tensors)
            self._keep = None
        return self._host


def size(nbytes, last_error, error):
    """The answer of a library's size query; a negative one is `error` with the library's last-error text"""
    if nbytes < 0:
        raise error(last_error())
    return nbytes


class Workspaces(dict):
    """(device index, *sizes) -> the device scratch buffer of one library's calls of those sizes.  workspace_bytes: the binding's
    size query (it refuses what the library refuses); held: the shapes kept at a time -- when a new one arrives with that
    many there, all go; dtype: the buffer's elements.  A buffer that goes may still be read by queued work: the call's Pending
    keeps it."""
    ITEM = {'float64': 8, 'int32': 4}

    def __init__(self, workspace_bytes, held, dtype='float64'):
        dict.__init__(self)
        self.workspace_bytes, self.held, self.dtype = workspace_bytes, held, dtype

    def buffer(self, device, *sizes):
        key = (device.index,) + sizes
        ws = self.get(key)
        if ws is None:
            import torch
            nbytes = self.workspace_bytes(*sizes)         # a refused size is refused before anything is evicted, and never held
            if len(self) >= self.held:
                self.clear()
            ws = self[key] = torch.empty(nbytes // self.ITEM[self.dtype], dtype=getattr(torch, self.dtype), device=device)
        return ws


def device_tensor(t, name, dtype, error, expected, want):
    """The two opening refusals: t is a torch tensor on a device (else `expected`: the binding's words for what it takes and that
    it has no host path) of the dtype torch.`dtype` (else 'expected `want`, got ...')"""
    import torch
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise error('%s: %s' % (name, expected))
    if t.dtype != getattr(torch, dtype):
        raise error('%s: expected %s, got %s' % (name, want, t.dtype))
    return t


def batched(t, name, rank, error, shapes, trailing=()):
    """t with the batch axis that one frame lacks: `rank` dimensions that end in `trailing`, else 'expected `shapes`, got ...'"""
    if t.dim() == rank - 1:
        t = t[None]
    if t.dim() != rank or tuple(t.shape[rank - len(trailing):]) != tuple(trailing):
        raise error('%s: expected %s, got %s' % (name, shapes, tuple(t.shape)))
    return t


def contiguous(t, name, error):
    """Contiguous or refused, where a copy would hide a caller's mistake (a binding that copies calls t.contiguous())"""
    if not t.is_contiguous():
        raise error('%s: expected a contiguous tensor, got strides %s for shape %s' % (name, tuple(t.stride()), tuple(t.shape)))
    return t


def same_frames(a, a_name, b, b_name, error):
    """The pair's refusals: one shape, one device"""
    if a.shape != b.shape:
        raise error('%s %s and %s %s differ in shape' % (a_name, tuple(a.shape), b_name, tuple(b.shape)))
    if a.device != b.device:
        raise error('%s and %s live on different devices' % (a_name, b_name))


def u8_pair(gt_u8, pred_u8, error, call):
    """(gt, pred) as contiguous uint8 device [F, H, W, 3] of one shape on one device: the byte pairs image_metrics and lpips score"""
    pair = []
    for t, name in ((gt_u8, 'gt_u8'), (pred_u8, 'pred_u8')):
        t = device_tensor(t, name, 'uint8', error, 'expected a CUDA/HIP uint8 tensor (%s has no CPU path)' % call,
                          'uint8 (the bytes written to the PNG)')
        pair.append(batched(t, name, 4, error, '[H, W, 3] or [F, H, W, 3]', (3,)).contiguous())
    same_frames(pair[0], 'gt_u8', pair[1], 'pred_u8', error)
    return pair

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

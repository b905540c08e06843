"""LPIPS (v0.1, VGG-16, linear heads, spatial mean) of finished frames on the device, from weights the user supplies: the
last image column of the paper's tables.  ctypes binding of liblpips_hip.so (include/lpips_hip.h).

The reference scores a render folder with utils/eval.py:12-22, `lpips.LPIPS(net='vgg')` in float32 on the CPU.  This package
ships no weights; `load_weights` reads the two public files a user of that script already has: torchvision's VGG-16
state dict (`features.{0,2,5,...,28}.{weight,bias}`) and the `lpips` package's linear heads (`lin{0..4}.model.1.weight`).
The metric's definition is DESIGN.md 8.2 (restated as code in tests/lpips_reference.py); it could not be compared with
the `lpips` package itself, which is on none of this project's machines.

There is no host path: without liblpips_hip.so and a device `lpips_u8` raises.
"""
import ctypes as C
import os

import numpy as np

from . import _ctypes_util as U

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get('LPIPS_HIP_LIB') or os.path.join(_HERE, 'liblpips_hip.so')
OK = 0
ABI_VERSION = 1
MIN_SIDE = 16
CONV_INDEX = (0, 2, 5, 7, 10, 12, 14, 17, 19, 21, 24, 26, 28)            # positions in torchvision's vgg16().features
CONV_SHAPES = ((3, 64), (64, 64), (64, 128), (128, 128), (128, 256), (256, 256), (256, 256), (256, 512), (512, 512),
               (512, 512), (512, 512), (512, 512), (512, 512))            # (Cin, Cout)
TAP_CHANNELS = (64, 128, 256, 512, 512)
_PREFIXES = ('net.', 'module.')

_fp = C.c_void_p
# every symbol include/lpips_hip.h declares: name -> (restype, argtypes)
SYMBOLS = {
    'lpips_last_error': (C.c_char_p, []),
    'lpips_abi_version': (C.c_int, []),
    'lpips_packed_conv_floats': (C.c_int64, [C.c_int, C.c_int]),
    'lpips_pack_conv': (C.c_int, [_fp, C.c_int, C.c_int, _fp, _fp]),
    'lpips_conv3x3_relu': (C.c_int, [_fp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _fp, _fp, _fp, _fp]),
    'lpips_flat_floats': (C.c_int64, []),
    'lpips_packed_bytes': (C.c_int64, []),
    'lpips_pack_weights': (C.c_int, [_fp, _fp, _fp]),
    'lpips_workspace_bytes': (C.c_int64, [C.c_int, C.c_int, C.c_int]),
    'lpips_u8': (C.c_int, [_fp, C.c_int, C.c_int, C.c_int, _fp, _fp, _fp, _fp, _fp]),
}

_lib = None


class LpipsError(RuntimeError):
    pass


def lib():
    """The loaded library with typed prototypes.  Raises if it has not been built."""
    global _lib
    if _lib is None:
        _lib = U.load(LIB_PATH, 'liblpips_hip.so', SYMBOLS, 'lpips_abi_version', ABI_VERSION, LpipsError,
                      ' (hipcc --offload-arch=gfx950). There is no CPU fallback for LPIPS.')
    return _lib


def last_error():
    return lib().lpips_last_error().decode('utf-8', 'replace')


check = U.checker(lib, 'lpips_last_error', LpipsError, 'lpips call')


def workspace_bytes(n_pairs, H, W):
    """Size of the call's scratch buffer; raises LpipsError for sizes the library rejects (H < 16, W < 16).  Needs no GPU."""
    return U.size(lib().lpips_workspace_bytes(int(n_pairs), int(H), int(W)), last_error, LpipsError)


_workspaces = U.Workspaces(workspace_bytes, 1)            # one shape at a time: a test split has one frame size


def weight_keys():
    """The 31 state-dict keys and shapes load_weights needs, in the order of the library's flat layout"""
    keys = []
    for idx, (cin, cout) in zip(CONV_INDEX, CONV_SHAPES):
        keys.append(('features.%d.weight' % idx, (cout, cin, 3, 3)))
        keys.append(('features.%d.bias' % idx, (cout,)))
    for l, c in enumerate(TAP_CHANNELS):
        keys.append(('lin%d.model.1.weight' % l, (1, c, 1, 1)))
    return keys


class Weights(object):
    """The float32 tensors of the metric on the host (`.tensors`: key -> numpy array) and, per device, the operand layout of
    the kernels (lpips_pack_weights, once per device and process)."""

    def __init__(self, tensors):
        self.tensors = {}
        for key, shape in weight_keys():
            if key not in tensors:
                raise LpipsError('LPIPS weights: key %r is missing' % key)
            a = np.asarray(tensors[key], np.float32)
            if tuple(a.shape) != shape:
                raise LpipsError('LPIPS weights: key %r has shape %s, expected %s' % (key, tuple(a.shape), shape))
            self.tensors[key] = np.ascontiguousarray(a)
        self._packed = {}

    def flat(self):
        return np.concatenate([self.tensors[k].reshape(-1) for k, _ in weight_keys()])

    def packed(self, device):
        import torch
        t = self._packed.get(device.index)
        if t is None:
            flat = self.flat()
            if flat.size != lib().lpips_flat_floats():
                raise LpipsError('flat weight count %d != lpips_flat_floats() %d' % (flat.size, lib().lpips_flat_floats()))
            with torch.cuda.device(device):
                src = torch.from_numpy(flat).to(device)
                t = torch.empty(lib().lpips_packed_bytes() // 4, dtype=torch.float32, device=device)
                check(lib().lpips_pack_weights(U.stream(), U.p(src), U.p(t)), 'lpips_pack_weights')
                torch.cuda.current_stream().synchronize()         # src may go
            self._packed[device.index] = t
        return t


def _read_state(path):
    if not os.path.isfile(path):
        raise LpipsError('LPIPS weights: no such file %r' % path)
    if path.endswith('.npz'):
        with np.load(path) as z:
            return {k: z[k] for k in z.files}
    import torch
    try:
        sd = torch.load(path, map_location='cpu', weights_only=True)
    except Exception as e:
        raise LpipsError('LPIPS weights: %r is neither an .npz nor a torch.load-able state dict (%s)' % (path, e))
    if isinstance(sd, dict) and 'state_dict' in sd and isinstance(sd['state_dict'], dict):
        sd = sd['state_dict']
    if not isinstance(sd, dict):
        raise LpipsError('LPIPS weights: %r holds a %s, expected a state dict' % (path, type(sd).__name__))
    return {k: v.detach().cpu().numpy() for k, v in sd.items() if hasattr(v, 'detach')}


def _strip(key):
    while key.startswith(_PREFIXES):
        key = key[key.index('.') + 1:]
    return key


def load_weights(paths):
    """Weights from one or two files ('A' or 'A,B' or a list): each an `.npz` or a torch.load-able state dict.  Together they
    must hold the 26 VGG-16 tensors `features.{i}.{weight,bias}` and the five `lin{l}.model.1.weight`; a leading `net.` /
    `module.` is tolerated, other keys (the classifier, dropout-free heads' other entries) are ignored.  A missing or
    mis-shaped key is an LpipsError that names it."""
    if isinstance(paths, str):
        paths = [p for p in paths.split(',') if p]
    paths = list(paths)
    if not 1 <= len(paths) <= 2:
        raise LpipsError('--lpips_weights: expected one or two files (A or A,B), got %d' % len(paths))
    merged = {}
    for p in paths:
        for k, v in _read_state(p).items():
            merged[_strip(k)] = v
    return Weights(merged)


def save_npz(path, tensors):
    """Write a {key: array} dict as an .npz load_weights reads (for converting weights on a machine that has them)"""
    np.savez(path, **{k: np.asarray(v, np.float32) for k, v in tensors.items()})


def lpips_u8(gt_u8, pred_u8, weights):
    """(total [F], per_tap [F, 5]) float64 numpy arrays of uint8 device tensors [F, H, W, 3] (or one frame [H, W, 3]): `gt_u8`
    the ground-truth bytes, `pred_u8` the very bytes written to the PNG, `weights` from load_weights.  One library call for
    the batch, one synchronisation when the values are read."""
    import torch
    if not isinstance(weights, Weights):
        raise LpipsError('weights: expected lpips.Weights (load_weights), got %s' % type(weights).__name__)
    gt, pred = U.u8_pair(gt_u8, pred_u8, LpipsError, 'lpips_u8')
    F, H, W = (int(v) for v in gt.shape[:3])
    with torch.cuda.device(gt.device):
        ws = _workspaces.buffer(gt.device, F, H, W)       # first: a frame the library refuses is refused before the weights are packed
        packed = weights.packed(gt.device)
        out = torch.empty((F, 6), dtype=torch.float64, device=gt.device)
        check(lib().lpips_u8(U.stream(), F, H, W, U.p(gt), U.p(pred), U.p(packed), U.p(ws), U.p(out)), 'lpips_u8')
        host = out.cpu().numpy()                          # the only synchronisation of the call
    return host[:, 5].copy(), host[:, :5].copy()


def lpips_u8_lists(gts, preds, weights, device=None):
    """total [F] of lists of uint8 [H, W, 3] numpy arrays: one call per frame size (eval_outputs.lpips_scores)"""
    from .eval_outputs import lpips_scores
    return np.asarray(lpips_scores(gts, preds, weights, device)['lpips'])

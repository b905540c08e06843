"""Colour-corrected test renders on the device: upstream's image.color_correct (mipnerf360/internal/image.py:81-124), the
step behind eval.py's `color_cc_{idx:03d}.png` and `metric_cc_psnr_{step}.txt`.  ctypes binding of libcolorcc_hip.so
(include/colorcc_hip.h).

A model trained with per-image appearance embeddings is rendered with the zero embedding, so every test
render carries an exposure / white-balance offset against its ground-truth frame.  color_correct fits, five times over, a
quadratic colour warp of the render to the ground truth on the unsaturated values and applies it.  The definition is
DESIGN.md 8.3 (restated as code in tests/color_correct_reference.py); it could not be compared with the jax original, which
is on none of this project's machines.

One library call corrects a whole split: 12 launches, the 10 x 10 systems solved on the device, nothing synchronises until
the values are read.  There is no host path: without libcolorcc_hip.so and a device `color_correct` raises.
"""
import ctypes as C
import os

import numpy as np

from . import _ctypes_util as U
from .eval_outputs import mse_to_psnr

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get('COLORCC_HIP_LIB') or os.path.join(_HERE, 'libcolorcc_hip.so')
OK = 0
ABI_VERSION = 1
NUM_ITERS = 5
N_SUMS = 66
N_OUT = 2 + 3 * NUM_ITERS

_fp = C.c_void_p
# every symbol include/colorcc_hip.h declares: name -> (restype, argtypes)
SYMBOLS = {
    'colorcc_last_error': (C.c_char_p, []),
    'colorcc_abi_version': (C.c_int, []),
    'colorcc_workspace_bytes': (C.c_int64, [C.c_int, C.c_int, C.c_int]),
    'colorcc_correct': (C.c_int, [_fp, C.c_int, C.c_int, C.c_int, _fp, _fp, C.c_int, _fp, _fp, _fp, _fp]),
    'colorcc_normal_equations': (C.c_int, [_fp, C.c_int, C.c_int, C.c_int, _fp, _fp, _fp, _fp]),
}

_lib = None
_workspaces = {}          # (device index, F, H, W) -> device buffer of colorcc_workspace_bytes


class ColorCorrectError(RuntimeError):
    pass


def lib():
    """The loaded library with typed prototypes.  Raises if it has not been built."""
    global _lib
    if _lib is None:
        _lib = U.load(LIB_PATH, 'libcolorcc_hip.so', SYMBOLS, 'colorcc_abi_version', ABI_VERSION, ColorCorrectError,
                      ' (hipcc --offload-arch=gfx950). There is no CPU fallback for color_correct.')
    return _lib


def last_error():
    return lib().colorcc_last_error().decode('utf-8', 'replace')


check = U.checker(lib, 'colorcc_last_error', ColorCorrectError, 'colorcc call')


def workspace_bytes(n_frames, H, W):
    """Size of a call's scratch buffer; raises ColorCorrectError for sizes the library rejects.  Needs no GPU."""
    n = lib().colorcc_workspace_bytes(int(n_frames), int(H), int(W))
    if n < 0:
        raise ColorCorrectError(last_error())
    return n


def _frames(img_f32, ref_u8):
    import torch
    for t, name, dtype in ((img_f32, 'img_f32', torch.float32), (ref_u8, 'ref_u8', torch.uint8)):
        if not isinstance(t, torch.Tensor) or not t.is_cuda:
            raise ColorCorrectError('%s: expected a CUDA/HIP %s tensor (color_correct has no CPU path)' % (name, dtype))
        if t.dtype != dtype:
            raise ColorCorrectError('%s: expected %s, got %s' % (name, dtype, t.dtype))
    if img_f32.dim() == 3:
        img_f32 = img_f32[None]
    if ref_u8.dim() == 3:
        ref_u8 = ref_u8[None]
    if img_f32.dim() != 4 or img_f32.shape[-1] != 3:
        raise ColorCorrectError('img_f32: expected [H, W, 3] or [F, H, W, 3], got %s' % (tuple(img_f32.shape),))
    if img_f32.shape != ref_u8.shape:
        raise ColorCorrectError('img_f32 %s and ref_u8 %s differ in shape' % (tuple(img_f32.shape), tuple(ref_u8.shape)))
    if img_f32.device != ref_u8.device:
        raise ColorCorrectError('img_f32 and ref_u8 live on different devices')
    return img_f32.contiguous(), ref_u8.contiguous()


def _workspace(device, F, H, W):
    import torch
    nbytes = workspace_bytes(F, H, W)
    key = (device.index, F, H, W)
    ws = _workspaces.get(key)
    if ws is None:
        _workspaces.clear()                               # one shape at a time: a test split has one frame size
        ws = _workspaces[key] = torch.empty(nbytes // 8, dtype=torch.float64, device=device)
    return ws


class PendingCorrection(object):
    """The device result of one color_correct_async call.  `.rgb_cc` (float64 [F, H, W, 3]) and `.cc_u8` (uint8, the PNG's
    bytes) are device tensors, usable by later work on the same stream without waiting; `.get()` synchronises (once) and
    returns (rgb_cc, cc_u8, psnr_cc [F], mask_counts [F, 5, 3]) as numpy arrays."""

    def __init__(self, rgb_cc, cc_u8, out, keep):
        self.rgb_cc, self.cc_u8, self._out, self._keep, self._host = rgb_cc, cc_u8, out, keep, None

    def get(self):
        if self._host is None:
            out = self._out.cpu().numpy()                 # the only synchronisation of the call
            self._host = (self.rgb_cc.cpu().numpy(), self.cc_u8.cpu().numpy(), mse_to_psnr(out[:, 0] / out[:, 1]),
                          out[:, 2:].reshape(-1, NUM_ITERS, 3).copy())
            self._keep = None
        return self._host


def color_correct_async(img_f32, ref_u8, quantize=True):
    """Enqueue the correction of float32 renders [F, H, W, 3] (or one frame) against the ground-truth bytes on torch's current
    stream and return a PendingCorrection; nothing waits for the device.  quantize: PSNR of the corrected frame rounded to
    8 bits (Config.eval_quantize_metrics), else of the float64 values."""
    import torch
    img, ref = _frames(img_f32, ref_u8)
    F, H, W = (int(v) for v in img.shape[:3])
    with torch.cuda.device(img.device):
        ws = _workspace(img.device, F, H, W)
        rgb_cc = torch.empty((F, H, W, 3), dtype=torch.float64, device=img.device)
        cc_u8 = torch.empty((F, H, W, 3), dtype=torch.uint8, device=img.device)
        out = torch.empty((F, N_OUT), dtype=torch.float64, device=img.device)
        stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        check(lib().colorcc_correct(stream, F, H, W, img.data_ptr(), ref.data_ptr(), 1 if quantize else 0, ws.data_ptr(),
                                    rgb_cc.data_ptr(), cc_u8.data_ptr(), out.data_ptr()), 'colorcc_correct')
    return PendingCorrection(rgb_cc, cc_u8, out, (img, ref))


def color_correct(img_f32, ref_u8, quantize=True):
    """(rgb_cc float64 [F, H, W, 3], cc_u8 uint8 [F, H, W, 3], psnr_cc [F], mask_counts [F, 5, 3]) as numpy arrays: the blocking
    form of color_correct_async."""
    return color_correct_async(img_f32, ref_u8, quantize).get()


def normal_equations(img_f32, ref_u8):
    """[F, 3, 66] float64 numpy: the masked sums of the first fit (55 Gram entries, 10 right-hand sides, count) -- for tests"""
    import torch
    img, ref = _frames(img_f32, ref_u8)
    F, H, W = (int(v) for v in img.shape[:3])
    with torch.cuda.device(img.device):
        ws = _workspace(img.device, F, H, W)
        sums = torch.empty((F, 3, N_SUMS), dtype=torch.float64, device=img.device)
        stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        check(lib().colorcc_normal_equations(stream, F, H, W, img.data_ptr(), ref.data_ptr(), ws.data_ptr(), sums.data_ptr()),
              'colorcc_normal_equations')
        return sums.cpu().numpy()


def color_correct_u8_lists(gts, preds, quantize=True, device=None):
    """(cc_u8 list, psnr_cc [F]) of lists of uint8 [H, W, 3] numpy arrays, `byte / 255` of a prediction being its img: one call
    per frame size (eval_images --color_correct)"""
    from .eval_outputs import color_corrected
    imgs = [p.astype(np.float32) / np.float32(255) for p in preds]                        # on the host: IEEE float32 division
    return color_corrected(gts, imgs, quantize, device=device)[:2]

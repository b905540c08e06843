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
    return U.size(lib().colorcc_workspace_bytes(int(n_frames), int(H), int(W)), last_error, ColorCorrectError)


_workspaces = U.Workspaces(workspace_bytes, 1)            # one shape at a time: a test split has one frame size


def _frames(img_f32, ref_u8):
    for t, name, dtype in ((img_f32, 'img_f32', 'float32'), (ref_u8, 'ref_u8', 'uint8')):
        U.device_tensor(t, name, dtype, ColorCorrectError, 'expected a CUDA/HIP torch.%s tensor (color_correct has no CPU path)' % dtype,
                        'torch.' + dtype)
    if ref_u8.dim() == 3:                                 # no more is asked of ref_u8 by itself: it has img_f32's shape or is refused
        ref_u8 = ref_u8[None]
    img_f32 = U.batched(img_f32, 'img_f32', 4, ColorCorrectError, '[H, W, 3] or [F, H, W, 3]', (3,))
    U.same_frames(img_f32, 'img_f32', ref_u8, 'ref_u8', ColorCorrectError)
    return img_f32.contiguous(), ref_u8.contiguous()


def _host(tensors):
    out = tensors['rows'].cpu().numpy()                   # the only synchronisation of the call
    return (tensors['rgb_cc'].cpu().numpy(), tensors['cc_u8'].cpu().numpy(), mse_to_psnr(out[:, 0] / out[:, 1]),
            out[:, 2:].reshape(-1, NUM_ITERS, 3).copy())


def color_correct_async(img_f32, ref_u8, quantize=True):
    """Enqueue the correction of float32 renders [F, H, W, 3] (or one frame) against the ground-truth bytes on torch's current
    stream and return a Pending; nothing waits for the device.  Its `.tensors['rgb_cc']` (float64 [F, H, W, 3]) and
    `.tensors['cc_u8']` (uint8, the PNG's bytes) are usable by later work on the same stream without waiting ('rows': the sums
    behind the PSNR and the mask counts); `.get()` synchronises (once) and returns (rgb_cc, cc_u8, psnr_cc [F], mask_counts
    [F, 5, 3]) as numpy arrays.  quantize: PSNR of the corrected frame rounded to 8 bits (Config.eval_quantize_metrics), else of
    the float64 values."""
    import torch
    img, ref = _frames(img_f32, ref_u8)
    F, H, W = (int(v) for v in img.shape[:3])
    with torch.cuda.device(img.device):
        ws = _workspaces.buffer(img.device, F, H, W)
        rgb_cc = torch.empty((F, H, W, 3), dtype=torch.float64, device=img.device)
        cc_u8 = torch.empty((F, H, W, 3), dtype=torch.uint8, device=img.device)
        out = torch.empty((F, N_OUT), dtype=torch.float64, device=img.device)
        check(lib().colorcc_correct(U.stream(), F, H, W, U.p(img), U.p(ref), 1 if quantize else 0, U.p(ws), U.p(rgb_cc), U.p(cc_u8),
                                    U.p(out)), 'colorcc_correct')
    return U.Pending({'rgb_cc': rgb_cc, 'cc_u8': cc_u8, 'rows': out}, (img, ref, ws), _host)


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
        ws = _workspaces.buffer(img.device, F, H, W)
        sums = torch.empty((F, 3, N_SUMS), dtype=torch.float64, device=img.device)
        check(lib().colorcc_normal_equations(U.stream(), F, H, W, U.p(img), U.p(ref), U.p(ws), U.p(sums)), 'colorcc_normal_equations')
        return sums.cpu().numpy()


def color_correct_u8_lists(gts, preds, quantize=True, device=None):
    """(cc_u8 list, psnr_cc [F]) of lists of uint8 [H, W, 3] numpy arrays, `byte / 255` of a prediction being its img: one call
    per frame size (eval_images --color_correct)"""
    from .eval_outputs import color_corrected
    imgs = [p.astype(np.float32) / np.float32(255) for p in preds]                        # on the host: IEEE float32 division
    return color_corrected(gts, imgs, quantize, device=device)[:2]

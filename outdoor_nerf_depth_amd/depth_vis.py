"""Depth pictures on the device: what upstream's evaluators draw from rendered depth.  ctypes binding of libdepthvis_hip.so
(include/depthvis_hip.h).

MipNeRF-360: eval.py sends every frame through internal/vis.py: visualize_suite -- turbo-coloured `depth_mean` and
`depth_median`, clipped at acc-weighted percentiles of the frame, `depth_triplet`, `color_matte` and `coords_mod`
(`mip360_suite_async`).  NeRF++: ddp_test_nerf.py:129-137 writes jet-coloured, min-max normalised fg_ / bg_ depth
(`minmax_colorize_async`).  The definition is DESIGN.md 8.4 (restated as code in tests/depth_vis_reference.py); it could not
be compared with the jax original, which is on none of this project's machines.

One call handles a whole split [F, H, W]; everything is enqueued on torch's current stream and nothing synchronises until
the bytes are read.  torch only allocates.  There is no host path: without libdepthvis_hip.so and a device every call raises.
"""
import ctypes as C
import os

import numpy as np

from . import _ctypes_util as U

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get('DEPTHVIS_HIP_LIB') or os.path.join(_HERE, 'libdepthvis_hip.so')
OK = 0
ABI_VERSION = 1
MAX_N = 1 << 22
MAX_PS = 4
MODE_CMAP, MODE_CMAP3, MODE_MINMAX, MODE_MATTE_RGB, MODE_COORDS_MOD = range(5)
CMAPS = {'turbo': 0, 'jet': 1}
CURVES = {'identity': 0, 'neg_log': 1, 'log': 2}
SUITE_PS = (0.5, 99.5)            # visualize_cmap's percentile = 99: [50 - 99 / 2, 50 + 99 / 2]
SUITE_KEYS = ('depth_mean', 'depth_median', 'depth_triplet', 'color_matte', 'coords_mod')

_fp = C.c_void_p
# every symbol include/depthvis_hip.h declares: name -> (restype, argtypes)
SYMBOLS = {
    'depthvis_last_error': (C.c_char_p, []),
    'depthvis_abi_version': (C.c_int, []),
    'depthvis_workspace_bytes': (C.c_int64, [C.c_int, C.c_int64]),
    'depthvis_percentiles': (C.c_int, [_fp, C.c_int, C.c_int64, _fp, _fp, C.c_int, C.POINTER(C.c_double), _fp, _fp]),
    'depthvis_minmax': (C.c_int, [_fp, C.c_int, C.c_int64, _fp, _fp, _fp]),
    'depthvis_prepare': (C.c_int, [_fp, C.c_int, C.c_int64, _fp, _fp, _fp, _fp, _fp, _fp, _fp, _fp]),
    'depthvis_colorize': (C.c_int, [_fp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _fp, _fp, _fp, _fp, _fp, _fp, _fp]),
}

_lib = None


class DepthVisError(RuntimeError):
    pass


def lib():
    """The loaded library with typed prototypes.  Raises if it has not been built."""
    global _lib
    if _lib is None:
        _lib = U.load(LIB_PATH, 'libdepthvis_hip.so', SYMBOLS, 'depthvis_abi_version', ABI_VERSION, DepthVisError,
                      ' (hipcc --offload-arch=gfx950). There is no CPU fallback for the depth pictures.')
    return _lib


def last_error():
    return lib().depthvis_last_error().decode('utf-8', 'replace')


check = U.checker(lib, 'depthvis_last_error', DepthVisError, 'depthvis call')


def workspace_bytes(n_frames, n):
    """Size of the scratch buffer of percentiles / minmax for frames of n values; raises DepthVisError for sizes the library
    rejects (n < 1, n > 2^22).  Needs no GPU."""
    return U.size(lib().depthvis_workspace_bytes(int(n_frames), int(n)), last_error, DepthVisError)


_workspaces = U.Workspaces(workspace_bytes, 2)            # a split has two sizes: H * W and, for the triplet, 3 * H * W


def _device_f32(t, name, trailing=()):
    """t as contiguous float32 [F, ...]: a device tensor whose shape ends in `trailing`; one frame gains the batch axis"""
    U.device_tensor(t, name, 'float32', DepthVisError, 'expected a CUDA/HIP float32 tensor (the depth pictures have no CPU path)',
                    'torch.float32')
    if tuple(t.shape[t.dim() - len(trailing):]) != tuple(trailing):
        raise DepthVisError('%s: shape %s does not end in %s' % (name, tuple(t.shape), tuple(trailing)))
    return t.contiguous()


def _percentiles(value, weight, ps, keep):
    """device float64 [F, len(ps)] of contiguous float32 [F, n] device tensors (enqueue only); the workspace joins `keep`, the list
    the call's Pending holds"""
    import torch
    F, n = (int(v) for v in value.shape)
    ps = [float(p) for p in ps]
    if not 1 <= len(ps) <= MAX_PS:
        raise DepthVisError('ps: %d percentiles, expected 1 .. %d' % (len(ps), MAX_PS))
    ws = _workspaces.buffer(value.device, F, n)
    keep.append(ws)
    out = torch.empty((F, len(ps)), dtype=torch.float64, device=value.device)
    check(lib().depthvis_percentiles(U.stream(), F, n, U.p(value), U.p(weight), len(ps), (C.c_double * len(ps))(*ps), U.p(ws),
                                     U.p(out)), 'depthvis_percentiles')
    return out


def weighted_percentiles_async(value, weight, ps):
    """Pending {'percentiles': float64 [F, len(ps)]} of float32 device tensors value, weight [F, N] (or [N]): upstream's
    vis.weighted_percentile per frame, np.interp(ps * (cw[-1] / 100), cw, sorted value)."""
    import torch
    value, weight = _device_f32(value, 'value'), _device_f32(weight, 'weight')
    if value.dim() == 1:
        value, weight = value[None], weight[None]
    if value.dim() != 2 or value.shape != weight.shape or value.device != weight.device:
        raise DepthVisError('value %s and weight %s: expected two [F, N] tensors on one device' % (tuple(value.shape), tuple(weight.shape)))
    with torch.cuda.device(value.device):
        keep = [value, weight]
        return U.Pending({'percentiles': _percentiles(value, weight, ps, keep)}, keep)


def weighted_percentiles(value, weight, ps):
    """float64 numpy [F, len(ps)]: the blocking form of weighted_percentiles_async"""
    return weighted_percentiles_async(value, weight, ps).get()['percentiles']


def _minmax(value, keep):
    """device float32 [F, 4] (min, max, nanmin, nanmax) of a contiguous float32 [F, n] device tensor (enqueue only); the workspace
    joins `keep`"""
    import torch
    F, n = (int(v) for v in value.shape)
    ws = _workspaces.buffer(value.device, F, n)
    keep.append(ws)
    out = torch.empty((F, 4), dtype=torch.float32, device=value.device)
    check(lib().depthvis_minmax(U.stream(), F, n, U.p(value), U.p(ws), U.p(out)), 'depthvis_minmax')
    return out


def minmax(value):
    """float32 numpy [F, 4]: min, max (NaN when the frame holds one, as numpy's), nanmin, nanmax of float32 [F, N] (or [N])"""
    import torch
    value = _device_f32(value, 'value')
    if value.dim() == 1:
        value = value[None]
    with torch.cuda.device(value.device):
        return _minmax(value.reshape(value.shape[0], -1), []).cpu().numpy()


def _colorize(F, H, W, mode, value, acc=None, origins=None, directions=None, lohi=None, mm=None, cmap='turbo', curve='identity'):
    import torch
    out = torch.empty((F, H, W, 3), dtype=torch.uint8, device=value.device)
    check(lib().depthvis_colorize(U.stream(), F, H, W, mode, CMAPS[cmap], CURVES[curve], U.p(value), U.p(acc), U.p(origins),
                                  U.p(directions), U.p(lohi), U.p(mm), U.p(out)), 'depthvis_colorize')
    return out


def _frames(t, name, channels=None):
    """float32 device [F, H, W] (channels None) or [F, H, W, channels]; one frame gains the batch axis"""
    t = _device_f32(t, name, () if channels is None else (channels,))
    return U.batched(t, name, 3 if channels is None else 4, DepthVisError, '[F, H, W%s]' % ('' if channels is None else ', %d' % channels))


def colorize_cmap_async(value, acc, lohi=None, cmap='turbo', curve='neg_log', ps=SUITE_PS):
    """Pending {'image': uint8 [F, H, W, 3], 'lohi': float64 [F, 2]}: upstream's visualize_cmap(value, acc, colormap, curve_fn)
    with the matte.  value [F, H, W] with a colour table, [F, H, W, 3] with cmap=None (depth_triplet's form, which needs lohi).
    lohi: device float64 [F, 2] to use instead of the acc-weighted percentiles `ps` of the frame."""
    import torch
    three = cmap is None
    value = _frames(value, 'value', 3 if three else None)
    acc = _frames(acc, 'acc')
    F, H, W = (int(v) for v in acc.shape)
    if tuple(value.shape[:3]) != (F, H, W) or value.device != acc.device:
        raise DepthVisError('value %s and acc %s differ in frame shape or device' % (tuple(value.shape), tuple(acc.shape)))
    keep = [value, acc]
    with torch.cuda.device(value.device):
        if lohi is None:
            if three:
                raise DepthVisError('colorize_cmap_async: a 3-channel value needs lohi (mip360_suite_async computes it)')
            lohi = _percentiles(value.reshape(F, -1), acc.reshape(F, -1), ps, keep)
        img = _colorize(F, H, W, MODE_CMAP3 if three else MODE_CMAP, value, acc, lohi=lohi, cmap=cmap or 'turbo', curve=curve)
    return U.Pending({'image': img, 'lohi': lohi}, keep)


def minmax_colorize_async(value, cmap='jet'):
    """Pending {'image': uint8 [F, H, W, 3], 'minmax': float32 [F, 4]}: the reference's utils.colorize_np without a mask and
    without the colour bar -- (x - min) / (max + 1e-6 - min) in float32 through the colour table.  value: float32 [F, H, W]."""
    import torch
    value = _frames(value, 'value')
    F, H, W = (int(v) for v in value.shape)
    keep = [value]
    with torch.cuda.device(value.device):
        mm = _minmax(value.reshape(F, -1), keep)
        img = _colorize(F, H, W, MODE_MINMAX, value, mm=mm, cmap=cmap)
    return U.Pending({'image': img, 'minmax': mm}, keep)


def matte_rgb_async(rgb, acc):
    """Pending {'image'}: vis.matte(rgb, acc) as bytes"""
    import torch
    rgb, acc = _frames(rgb, 'rgb', 3), _frames(acc, 'acc')
    F, H, W = (int(v) for v in acc.shape)
    if tuple(rgb.shape[:3]) != (F, H, W):
        raise DepthVisError('rgb %s and acc %s differ in frame shape' % (tuple(rgb.shape), tuple(acc.shape)))
    with torch.cuda.device(rgb.device):
        return U.Pending({'image': _colorize(F, H, W, MODE_MATTE_RGB, rgb, acc)}, (rgb, acc))


def coords_mod_async(origins, directions, distance, acc):
    """Pending {'image'}: vis.visualize_coord_mod(origins + directions * distance[..., None], acc) as bytes"""
    import torch
    origins, directions = _frames(origins, 'origins', 3), _frames(directions, 'directions', 3)
    distance, acc = _frames(distance, 'distance'), _frames(acc, 'acc')
    F, H, W = (int(v) for v in acc.shape)
    for t, name in ((origins, 'origins'), (directions, 'directions'), (distance, 'distance')):
        if tuple(t.shape[:3]) != (F, H, W):
            raise DepthVisError('%s %s and acc %s differ in frame shape' % (name, tuple(t.shape), tuple(acc.shape)))
    with torch.cuda.device(acc.device):
        return U.Pending({'image': _colorize(F, H, W, MODE_COORDS_MOD, distance, acc, origins, directions)},
                       (origins, directions, distance, acc))


def mip360_suite_async(rgb, acc, distance_mean, distance_median, distance_p5, distance_p95, origins, directions):
    """Pending with the five pictures of upstream's visualize_suite as uint8 [F, H, W, 3] (SUITE_KEYS) plus 'acc' (float32, zeroed
    where distance_mean is NaN) and the percentile bounds 'lohi_mean', 'lohi_median', 'lohi_triplet' (float64 [F, 2]).
    All inputs float32 device tensors: rgb, origins, directions [F, H, W, 3], the others [F, H, W]."""
    import torch
    acc = _frames(acc, 'acc')
    F, H, W = (int(v) for v in acc.shape)
    maps = [_frames(t, n) for t, n in ((distance_mean, 'distance_mean'), (distance_median, 'distance_median'),
                                       (distance_p5, 'distance_percentile_5'), (distance_p95, 'distance_percentile_95'))]
    vecs = [_frames(t, n, 3) for t, n in ((rgb, 'rgb'), (origins, 'origins'), (directions, 'directions'))]
    for t in maps + vecs:
        if tuple(t.shape[:3]) != (F, H, W) or t.device != acc.device:
            raise DepthVisError('mip360_suite_async: inputs differ in frame shape %s or device' % ((F, H, W),))
    dmean, dmedian, p5, p95 = maps
    rgb, origins, directions = vecs
    n = H * W
    workspace_bytes(F, 3 * n)                                 # the triplet's size decides whether the frame fits
    dev = acc.device
    with torch.cuda.device(dev):
        acc_eff = torch.empty_like(acc)
        trip_v = torch.empty((F, H, W, 3), dtype=torch.float32, device=dev)
        trip_w = torch.empty((F, H, W, 3), dtype=torch.float32, device=dev)
        keep = [maps, vecs, acc, trip_v, trip_w]
        check(lib().depthvis_prepare(U.stream(), F, n, U.p(acc), U.p(dmean), U.p(dmedian), U.p(p5), U.p(p95), U.p(acc_eff), U.p(trip_v),
                                     U.p(trip_w)), 'depthvis_prepare')
        w = acc_eff.reshape(F, n)
        out = {'acc': acc_eff}
        for key, v in (('mean', dmean), ('median', dmedian)):
            lohi = out['lohi_' + key] = _percentiles(v.reshape(F, n), w, SUITE_PS, keep)
            out['depth_' + key] = _colorize(F, H, W, MODE_CMAP, v, acc_eff, lohi=lohi, cmap='turbo', curve='neg_log')
        lohi = out['lohi_triplet'] = _percentiles(trip_v.reshape(F, 3 * n), trip_w.reshape(F, 3 * n), SUITE_PS, keep)
        out['depth_triplet'] = _colorize(F, H, W, MODE_CMAP3, trip_v, acc_eff, lohi=lohi, curve='log')
        out['color_matte'] = _colorize(F, H, W, MODE_MATTE_RGB, rgb, acc_eff)
        out['coords_mod'] = _colorize(F, H, W, MODE_COORDS_MOD, dmean, acc_eff, origins, directions)
    return U.Pending(out, keep)


def mip360_depth_pair_async(distance_mean, distance_median, acc):
    """Pending {'depth_mean', 'depth_median', 'acc', 'lohi_mean', 'lohi_median'}: the two pictures of mip360_suite_async that
    need nothing but a prediction folder's TIFFs (eval_images --depth_vis)"""
    import torch
    acc, dmean, dmedian = _frames(acc, 'acc'), _frames(distance_mean, 'distance_mean'), _frames(distance_median, 'distance_median')
    F, H, W = (int(v) for v in acc.shape)
    if tuple(dmean.shape) != (F, H, W) or tuple(dmedian.shape) != (F, H, W):
        raise DepthVisError('mip360_depth_pair_async: inputs differ in frame shape')
    keep = [acc, dmean, dmedian]
    with torch.cuda.device(acc.device):
        acc_eff = torch.empty_like(acc)
        check(lib().depthvis_prepare(U.stream(), F, H * W, U.p(acc), U.p(dmean), None, None, None, U.p(acc_eff), None, None),
              'depthvis_prepare')
        out = {'acc': acc_eff}
        for key, v in (('mean', dmean), ('median', dmedian)):
            lohi = out['lohi_' + key] = _percentiles(v.reshape(F, -1), acc_eff.reshape(F, -1), SUITE_PS, keep)
            out['depth_' + key] = _colorize(F, H, W, MODE_CMAP, v, acc_eff, lohi=lohi, cmap='turbo', curve='neg_log')
    return U.Pending(out, keep)


def save_pngs(images, pattern, indices=None):
    """write uint8 [F, H, W, 3] as pattern % index"""
    from PIL import Image
    for k, img in enumerate(images):
        Image.fromarray(np.ascontiguousarray(img)).save(pattern % (k if indices is None else indices[k]))

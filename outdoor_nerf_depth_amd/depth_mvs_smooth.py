"""The plane sweep with semi-global smoothing on the device (restated as code in
tests/depth_mvs_smooth_reference.py): ctypes binding of libdepthsgm_hip.so (include/depthsgm_hip.h).  The aggregated cost C(p, k) of
depth_mvs's sweep is summed along `smooth_paths` scanline directions,

    L_r(p, k) = C(p, k) + min(L_r(q, k), L_r(q, k - 1) + P1, L_r(q, k + 1) + P1, M + P2') - M,   q = p - r,  M = min_k L_r(q, k),

with L_r(p, k) = C(p, k) where q is outside the frame, and the winner, the uniqueness test and the parabola are taken on
S = sum_r L_r.  P1 and P2 are smooth_p1 and smooth_p2 times best_views times the taps of the aggregation window: penalties per
census bit in the units of C.  With smooth_edge > 0, P2' = max(P1, P2 // (1 + |Y(p) - Y(q)| // smooth_edge)) with the census' luma.

This module is reached through depth_mvs (sweep_async, sweep_priors, sweep_samplers, the CLI and both trainers' flags) when
smooth_paths is not 0, and is not imported otherwise.  The parameters, their checks and the error class are depth_mvs's.

The library keeps C (uint16) and S (uint32) of `slab_frames` frames at a time, 6 bytes per pixel and plane, and loops over chunks of
that many; the results do not depend on it.  It follows from a byte budget, slab_bytes (4 GiB by default), at least one frame.

Everything is enqueued on torch's current stream.  There is no host path: without libdepthsgm_hip.so and a device every call raises.
"""
import ctypes as C
import os

import numpy as np

from . import _ctypes_util as U
from . import depth_mvs as M

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get('DEPTHSGM_HIP_LIB') or os.path.join(_HERE, 'libdepthsgm_hip.so')
ABI_VERSION = 1
PLANE_ALIGN, SLAB_ENTRY_BYTES = 8, 6
SLAB_BYTES = 4 << 30
_fp = C.c_void_p
# every symbol include/depthsgm_hip.h declares: name -> (restype, argtypes)
SYMBOLS = {
    'depthsgm_last_error': (C.c_char_p, []),
    'depthsgm_abi_version': (C.c_int, []),
    'depthsgm_workspace_bytes': (C.c_int64, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int]),
    'depthsgm_sweep': (C.c_int, [_fp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _fp, _fp, _fp, _fp, C.c_int, C.c_int, C.c_double,
                                 C.c_double, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _fp, _fp, _fp, _fp, _fp, _fp, _fp, _fp, _fp]),
}
OPTIONAL = (('plane', 'uint8'), ('cost', 'int32'), ('second', 'int32'), ('census', 'int32'))

_lib = None


def lib():
    """The loaded library with typed prototypes.  Raises if it has not been built."""
    global _lib
    if _lib is None:
        _lib = U.load(LIB_PATH, 'libdepthsgm_hip.so', SYMBOLS, 'depthsgm_abi_version', ABI_VERSION, M.DepthMvsError,
                      ' (hipcc --offload-arch=gfx950). There is no CPU fallback for the smoothed plane sweep.')
    return _lib


def last_error():
    return lib().depthsgm_last_error().decode('utf-8', 'replace')


check = U.checker(lib, 'depthsgm_last_error', M.DepthMvsError, 'depthsgm call')


def workspace_bytes(n_frames, height, width, planes, slab_frames):
    """Size of the scratch buffer of a call: the plain sweep's census and partials, and the slabs of min(slab_frames, n_frames)
    frames, 6 bytes per pixel and plane with the planes rounded up to a multiple of 8.  Raises DepthMvsError for sizes the library
    rejects.  Needs no GPU."""
    return U.size(lib().depthsgm_workspace_bytes(int(n_frames), int(height), int(width), int(planes), int(slab_frames)), last_error,
                  M.DepthMvsError)


_workspaces = U.Workspaces(workspace_bytes, 2, 'float64')


def slab_frames_of(n_frames, height, width, planes, slab_bytes=None):
    """The frames the slabs hold under a budget of slab_bytes (SLAB_BYTES by default): all of them if they fit, at least one"""
    budget = SLAB_BYTES if slab_bytes is None else int(slab_bytes)
    if budget < 0:
        raise M.DepthMvsError('slab_bytes = %r: expected a number of bytes >= 0' % (slab_bytes,))
    dp = (int(planes) + PLANE_ALIGN - 1) // PLANE_ALIGN * PLANE_ALIGN
    return int(max(1, min(int(n_frames), budget // (SLAB_ENTRY_BYTES * dp * int(height) * int(width)))))


def enqueue(rgb, cams_d, nbr_d, inv_d, prm, plane=True, cost=True, second=True, census=False, rows=True, out=None, slab_bytes=None,
            slab_frames=None):
    """depth_mvs.enqueue for parameters with smooth_paths: the same tensors, with 'cost' and 'second' int32 holding the uint32 of
    S.  slab_frames: the frames the slabs hold, instead of what slab_bytes gives."""
    import torch
    rgb, F, H, W, V, D, dev = M.call_tensors(rgb, cams_d, nbr_d, inv_d)
    if slab_frames is None:
        slab_frames = slab_frames_of(F, H, W, D, slab_bytes)
    slab_frames = min(M._integer(slab_frames, 'slab_frames', 1, 1 << 30), F)
    P1, P2 = M.smooth_penalties(prm)
    with torch.cuda.device(dev):
        ws = _workspaces.buffer(dev, F, H, W, D, slab_frames)
        if out is None:
            out = M.new_outputs(F, H, W, dev, OPTIONAL, dict(plane=plane, cost=cost, second=second, census=census), rows)
        check(lib().depthsgm_sweep(U.stream(), F, H, W, V, D, U.p(rgb), U.p(cams_d), U.p(nbr_d), U.p(inv_d), prm['best_views'],
                                   prm['agg_radius'], prm['uniqueness'], prm['std_planes'], prm['smooth_paths'], P1, P2,
                                   prm['smooth_edge'], slab_frames, U.p(ws), U.p(out['depth']), U.p(out['std']), U.p(out['status']),
                                   U.p(out.get('plane')), U.p(out.get('cost')), U.p(out.get('second')), U.p(out.get('census')),
                                   U.p(out.get('rows'))), 'depthsgm_sweep')
    return U.Pending(out, (rgb, cams_d, nbr_d, inv_d, ws), _to_host)


def _to_host(tensors):
    """numpy arrays of the tensors; cost, second and census in the unsigned type torch lacks"""
    views = ('cost', 'second', 'census')
    return {name: t.cpu().numpy().view(np.uint32) if name in views else t.cpu().numpy() for name, t in tensors.items()}

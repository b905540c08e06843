"""A plane-sweep multi-view stereo depth prior on the device: the classical, weight-free stand-in for the paper's stereo prior, made
from the scene's own frames and poses.  ctypes binding of libdepthmvs_hip.so (include/depthmvs_hip.h), the adapters of both front
ends, and the CLI

    python -m outdoor_nerf_depth_amd.depth_mvs --data_dir SCENE [--gin_bindings ...]      (COLMAP layout)
    python -m outdoor_nerf_depth_amd.depth_mvs --datadir DIR --scene SCENE                (NeRF++ layout)

Every frame is swept through `planes` fronto-parallel depth planes against its `views` nearest frames: the 5 x 5 census of the luma
is matched by Hamming distance, the `best_views` best views of a plane are summed (the occlusion rule), the sums are aggregated
over a window of `agg_radius`, and the winning plane is refined by a parabola through its two neighbours.  A pixel whose winner too
few views see, that wins at an end of the table (the sky, a pixel without parallax) or whose winner is not `uniqueness` times
better than the best plane elsewhere is refused.  Every accepted pixel carries a standard deviation: `std_planes` plane steps
carried into depth.  The definition is DESIGN.md 8.11 (restated as code in tests/depth_mvs_reference.py).

With `smooth_paths` 4 or 8 the aggregated costs are first summed along that many scanline directions, with a penalty `smooth_p1` for
a change of one plane between neighbouring pixels and `smooth_p2` for a jump (semi-global smoothing): the winner,
the uniqueness test and the parabola are taken on the sum, which carries a pixel without texture by its neighbours.  That call is
depth_mvs_smooth.py's, on libdepthsgm_hip.so; with `smooth_paths` 0, the default, neither is loaded and the call is the plain one.

Out of scope: learned stereo, left/right pairs, sub-pixel matching, slanted planes, distorted cameras and moving objects (the
consistency check is the filter for those).

The CLI writes the folders the loaders already find under `--depth_sup_type mvs` (the prior and its `_std` twin for the 'gnll'
loss), plus mvs.txt with the counts.  The load-time flags (Config.depth_mvs_views, --depth_mvs_views) run the same call when a
training run loads its frames instead, before alignment, accumulation, the consistency check and the completion; they use the
float32 value, which the CLI's folders round to the PNG's 1 / 256 m.  For COLMAP scenes the CLI takes all frames together while
the flag takes the training split.

Everything is enqueued on torch's current stream and nothing synchronises until the numbers are read.  torch only allocates.
There is no host path: without libdepthmvs_hip.so and a device every call raises.
"""
import ctypes as C
import os

import numpy as np

from . import _ctypes_util as U
from . import depth_consistency as DC
from . import depth_prior_io as IO
from .depth_prior_io import overlaps as _overlaps, write_png16 as _write_png16, absrel, encode_metres as encode_std   # noqa: F401
from .depth_mvs_flags import (MAX_VIEWS, MIN_PLANES, MAX_PLANES, MAX_RADIUS, PARAMS, SMOOTH, STD_FLOOR_HELP, VIEWS_HELP,     # noqa: F401
                              add_flags, args_params, scene_params)

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get('DEPTHMVS_HIP_LIB') or os.path.join(_HERE, 'libdepthmvs_hip.so')
ABI_VERSION = 1
MAX_FRAMES = 65535
ROW_NAMES = ('n_accepted', 'n_end', 'n_ambiguous', 'n_unseen')
ACCEPTED, END, AMBIGUOUS, UNSEEN = 0, 1, 2, 3
MAX_P2, MAX_EDGE = 32767, 255                # of the smoothing: one path's value, at most 31104 + P2, fits 16 bits
_fp = C.c_void_p
# every symbol include/depthmvs_hip.h declares: name -> (restype, argtypes)
SYMBOLS = {
    'depthmvs_last_error': (C.c_char_p, []),
    'depthmvs_abi_version': (C.c_int, []),
    'depthmvs_workspace_bytes': (C.c_int64, [C.c_int, C.c_int, C.c_int]),
    'depthmvs_sweep': (C.c_int, [_fp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _fp, _fp, _fp, _fp, C.c_int, C.c_int, C.c_double,
                                 C.c_double, _fp, _fp, _fp, _fp, _fp, _fp, _fp, _fp, _fp]),
}

_lib = None


class DepthMvsError(RuntimeError):
    pass


def lib():
    """The loaded library with typed prototypes.  Raises if it has not been built."""
    global _lib
    if _lib is None:
        _lib = U.load(LIB_PATH, 'libdepthmvs_hip.so', SYMBOLS, 'depthmvs_abi_version', ABI_VERSION, DepthMvsError,
                      ' (hipcc --offload-arch=gfx950). There is no CPU fallback for the plane sweep.')
    return _lib


def last_error():
    return lib().depthmvs_last_error().decode('utf-8', 'replace')


check = U.checker(lib, 'depthmvs_last_error', DepthMvsError, 'depthmvs call')


def workspace_bytes(n_frames, height, width):
    """Size of the scratch buffer of a call on n_frames frames of height x width pixels; raises DepthMvsError for sizes the library
    rejects (n_frames outside 1 .. 65535, height * width outside 1 .. 2^28).  It does not depend on the planes.  Needs no GPU."""
    return U.size(lib().depthmvs_workspace_bytes(int(n_frames), int(height), int(width)), last_error, DepthMvsError)


_workspaces = U.Workspaces(workspace_bytes, 2, 'float64')


# ------------------------------------------------------------------------------------------------------ host side
def _integer(v, name, lo, hi, zero=''):
    if isinstance(v, bool) or int(v) != v or not lo <= int(v) <= hi:
        raise DepthMvsError('%s = %r: expected an integer %d .. %d%s' % (name, v, lo, hi, zero))
    return int(v)


def check_views(views, what='views'):
    return _integer(views, what, 1, MAX_VIEWS)


def check_params(views=4, planes=64, near=2.0, far=100.0, best_views=0, agg_radius=2, uniqueness=0.9, std_planes=0.5, std_floor=0.0,
                 smooth_paths=0, smooth_p1=1, smooth_p2=8, smooth_edge=0):
    """The parameters as the call takes them; best_views 0 (or None) is the default, half of the views rounded up.  The four smooth_*
    are among them only when smooth_paths is not 0, and are not looked at otherwise."""
    views = check_views(views)
    p = dict(views=views, planes=_integer(planes, 'planes', MIN_PLANES, MAX_PLANES), near=float(near), far=float(far),
             best_views=(views + 1) // 2 if not best_views else _integer(best_views, 'best_views', 1, views, ' (0 = half of the views)'),
             agg_radius=_integer(agg_radius, 'agg_radius', 0, MAX_RADIUS), uniqueness=float(uniqueness),
             std_planes=float(std_planes), std_floor=float(std_floor))
    if not (np.isfinite(p['near']) and p['near'] > 0):
        raise DepthMvsError('near = %r: expected a finite depth > 0' % p['near'])
    if not p['far'] > p['near']:
        raise DepthMvsError('far = %r: expected a depth above near = %r (inf: the plane at infinity)' % (p['far'], p['near']))
    if not 0 < p['uniqueness'] <= 1:
        raise DepthMvsError('uniqueness = %r: expected a number in (0, 1]' % p['uniqueness'])
    if not (np.isfinite(p['std_planes']) and p['std_planes'] > 0):
        raise DepthMvsError('std_planes = %r: expected a finite number > 0' % p['std_planes'])
    if not (np.isfinite(p['std_floor']) and p['std_floor'] >= 0):
        raise DepthMvsError('std_floor = %r: expected a finite number >= 0' % p['std_floor'])
    if isinstance(smooth_paths, bool) or smooth_paths not in (0, 4, 8):
        raise DepthMvsError('smooth_paths = %r: expected 0 (off), 4 or 8' % (smooth_paths,))
    if smooth_paths:
        p.update(smooth_paths=int(smooth_paths), smooth_p1=_integer(smooth_p1, 'smooth_p1', 1, MAX_P2),
                 smooth_p2=_integer(smooth_p2, 'smooth_p2', 1, MAX_P2), smooth_edge=_integer(smooth_edge, 'smooth_edge', 0, MAX_EDGE))
        P1, P2 = smooth_penalties(p)
        if not P1 <= P2 <= MAX_P2:
            raise DepthMvsError('smooth_p1 = %d, smooth_p2 = %d: in the units of the cost (times best_views = %d times the window of %d taps) '
                                'P1 = %d, P2 = %d, expected P1 <= P2 <= %d' % (p['smooth_p1'], p['smooth_p2'], p['best_views'],
                                                                             (2 * p['agg_radius'] + 1) ** 2, P1, P2, MAX_P2))
    return p


def smooth_penalties(prm):
    """(P1, P2) of checked parameters: smooth_p1 and smooth_p2, which are per census bit, in the units of the aggregated cost"""
    unit = prm['best_views'] * (2 * prm['agg_radius'] + 1) ** 2
    return prm['smooth_p1'] * unit, prm['smooth_p2'] * unit


def planes_table(near, far, planes):
    """float64 [planes]: the planes as inverse depths, uniform between 1 / far (entry 0; 0 for far = inf) and 1 / near"""
    lo, hi = 1.0 / np.float64(far), 1.0 / np.float64(near)
    t = lo + (hi - lo) * (np.arange(int(planes), dtype=np.float64) / np.float64(int(planes) - 1))
    t[0], t[-1] = lo, hi
    return t


def check_table(inv_depth):
    """The caller's planes as a contiguous float64 host array: 4 .. 256 entries, finite, >= 0, strictly increasing"""
    t = np.ascontiguousarray(np.asarray(inv_depth, np.float64).reshape(-1))
    if not MIN_PLANES <= t.size <= MAX_PLANES:
        raise DepthMvsError('inv_depth: %d planes, expected %d .. %d' % (t.size, MIN_PLANES, MAX_PLANES))
    if not (np.isfinite(t).all() and (t >= 0).all()):
        raise DepthMvsError('inv_depth: every entry must be finite and >= 0')
    if not (np.diff(t) > 0).all():
        raise DepthMvsError('inv_depth: the entries must be strictly increasing (entry %d is not above the one before it)'
                            % (int(np.argmax(~(np.diff(t) > 0))) + 1))
    return t


# ---------------------------------------------------------------------------------------------------- the call
NO_CPU = 'rgb: expected a CUDA/HIP uint8 tensor (the plane sweep has no CPU path)'
OPTIONAL = (('plane', 'uint8'), ('cost', 'int16'), ('second', 'int16'), ('census', 'int32'))


def _rgb_ok(rgb):
    """rgb checked as a contiguous uint8 [F, H, W, 3] tensor; where it lives is asked by the caller, last"""
    import torch
    if not isinstance(rgb, torch.Tensor):
        raise DepthMvsError(NO_CPU)
    if rgb.dtype != torch.uint8:
        raise DepthMvsError('rgb: expected torch.uint8, got %s' % rgb.dtype)
    if rgb.dim() != 4 or rgb.shape[3] != 3:
        raise DepthMvsError('rgb: expected [F, H, W, 3] (frames of one size), got %s' % (tuple(rgb.shape),))
    return U.contiguous(rgb, 'rgb', DepthMvsError)


def _cams_ok(cams, nbr, n_frames):
    cams_h, nbr_h = DC.validate(cams, nbr)
    if cams_h.shape[0] != n_frames:
        raise DepthMvsError('cams: %d cameras for %d frames of rgb' % (cams_h.shape[0], n_frames))
    if not 1 <= nbr_h.shape[1] <= MAX_VIEWS:
        raise DepthMvsError('nbr: %d neighbours per frame, expected 1 .. %d' % (nbr_h.shape[1], MAX_VIEWS))
    return cams_h, nbr_h


def call_tensors(rgb, cams_d, nbr_d, inv_d):
    """(rgb, F, H, W, V, D, device) of a library call's device tensors, checked"""
    import torch
    rgb = _rgb_ok(rgb)
    if not rgb.is_cuda:
        raise DepthMvsError(NO_CPU)
    F, H, W = (int(v) for v in rgb.shape[:3])
    dev = rgb.device
    V, D = int(nbr_d.shape[1]), int(inv_d.numel())
    for name, t, dtype, shape in (('cams', cams_d, torch.float64, (F, DC.CAM)), ('nbr', nbr_d, torch.int32, (F, V)),
                                  ('inv_depth', inv_d, torch.float64, (D,))):
        if not (isinstance(t, torch.Tensor) and t.dtype == dtype and tuple(t.shape) == shape and t.is_contiguous() and t.device == dev):
            raise DepthMvsError('%s: expected a contiguous %s tensor of shape %s on %s' % (name, dtype, shape, dev))
    return rgb, F, H, W, V, D, dev


def new_outputs(F, H, W, dev, optional, want, rows):
    """The output tensors of a call: depth, std, status, those of `optional` (name, dtype) that `want` asks for, and rows"""
    import torch
    out = {'depth': torch.empty((F, H, W), dtype=torch.float32, device=dev),
           'std': torch.empty((F, H, W), dtype=torch.float32, device=dev),
           'status': torch.empty((F, H, W), dtype=torch.uint8, device=dev)}
    for name, dtype in optional:
        if want[name]:
            out[name] = torch.empty((F, H, W), dtype=getattr(torch, dtype), device=dev)
    if rows:
        out['rows'] = torch.empty((F, len(ROW_NAMES)), dtype=torch.int64, device=dev)
    return out


def enqueue(rgb, cams_d, nbr_d, inv_d, prm, plane=True, cost=True, second=True, census=False, rows=True, out=None, **slab):
    """The library call alone, on cameras, neighbour lists and planes that are on the device already: Pending.  prm: check_params()
    (views, planes, near and far are not read here: the tensors say them).  out: the `.tensors` of an earlier call of the same
    shape and outputs, to write into again instead of allocating.  `.tensors`: 'depth', 'std' (float32 [F, H, W]), 'status' (uint8:
    0 accepted, 1 end, 2 ambiguous, 3 unseen) and, when asked, 'plane' (uint8), 'cost', 'second' (int16 holding the uint16),
    'census' (int32 holding the uint32) and 'rows' (int64 [F, 4] in ROW_NAMES' order); `.get()`: the same as numpy arrays, the
    three in their unsigned types.  With prm['smooth_paths'] the call is depth_mvs_smooth.enqueue's (cost and second are int32
    holding uint32 there; slab: its slab_bytes or slab_frames), which is imported here and not before."""
    if prm.get('smooth_paths'):
        from . import depth_mvs_smooth
        return depth_mvs_smooth.enqueue(rgb, cams_d, nbr_d, inv_d, prm, plane, cost, second, census, rows, out, **slab)
    if slab:
        raise DepthMvsError('%s: the plain sweep keeps no slab (smooth_paths = 0)' % ', '.join(sorted(slab)))
    import torch
    rgb, F, H, W, V, D, dev = call_tensors(rgb, cams_d, nbr_d, inv_d)
    with torch.cuda.device(dev):
        ws = _workspaces.buffer(dev, F, H, W)
        if out is None:
            out = new_outputs(F, H, W, dev, OPTIONAL, dict(plane=plane, cost=cost, second=second, census=census), rows)
        check(lib().depthmvs_sweep(U.stream(), F, H, W, V, D, U.p(rgb), U.p(cams_d), U.p(nbr_d), U.p(inv_d), prm['best_views'],
                                   prm['agg_radius'], prm['uniqueness'], prm['std_planes'], U.p(ws), U.p(out['depth']), U.p(out['std']),
                                   U.p(out['status']), U.p(out.get('plane')), U.p(out.get('cost')), U.p(out.get('second')),
                                   U.p(out.get('census')), U.p(out.get('rows'))), 'depthmvs_sweep')
    return U.Pending(out, (rgb, cams_d, nbr_d, inv_d, ws), _to_host)


def _to_host(tensors):
    """numpy arrays of the tensors; cost, second and census in the unsigned types torch lacks"""
    views = {'cost': np.uint16, 'second': np.uint16, 'census': np.uint32}
    return {name: t.cpu().numpy().view(views[name]) if name in views else t.cpu().numpy() for name, t in tensors.items()}


def sweep_async(rgb, cams, nbr, inv_depth=None, near=2.0, far=100.0, planes=64, plane=True, cost=True, second=True, census=False,
                rows=True, out=None, slab_bytes=None, slab_frames=None, **params):
    """Pending of the sweep of the uint8 device tensor rgb [F, H, W, 3] with the host arrays cams float64 [F, 16]
    (depth_consistency.pack_cams) and nbr int [F, V] (depth_consistency.neighbours; -1: no neighbour).  inv_depth: a host table of
    the planes as inverse depths to use instead of planes_table(near, far, planes), in the units of the cameras.  params:
    best_views, agg_radius, uniqueness, std_planes and smooth_paths, smooth_p1, smooth_p2, smooth_edge; slab_bytes, slab_frames: the
    smoothed call's (depth_mvs_smooth.enqueue).  Everything is checked on the host first; then three small uploads and the library
    call.  Enqueue only."""
    import torch
    rgb = _rgb_ok(rgb)
    nbr = np.asarray(nbr)
    n_views = nbr.shape[1] if nbr.ndim == 2 else 0
    if inv_depth is None:
        prm = check_params(check_views(n_views, 'nbr: neighbours per frame'), planes, near, far, **params)
        table = check_table(planes_table(prm['near'], prm['far'], prm['planes']))
    else:
        table = check_table(inv_depth)
        prm = check_params(check_views(n_views, 'nbr: neighbours per frame'), table.size, **params)
    cams_h, nbr_h = _cams_ok(cams, nbr, int(rgb.shape[0]))
    if not rgb.is_cuda:
        raise DepthMvsError(NO_CPU)
    dev = rgb.device
    slab = {k: v for k, v in (('slab_bytes', slab_bytes), ('slab_frames', slab_frames)) if v is not None}
    return enqueue(rgb, torch.from_numpy(cams_h).to(dev), torch.from_numpy(nbr_h).to(dev), torch.from_numpy(table).to(dev), prm,
                   plane, cost, second, census, rows, out, **slab)


def sweep_priors(rgb, cams, views=4, nbr=None, **params):
    """(prior float32 [F, H, W], its standard deviation float32 [F, H, W] floored at std_floor where accepted, status uint8
    [F, H, W], rows int64 [F, 4]) on rgb's device: the sweep of every frame against its `views` nearest frames (or the lists nbr).
    params: those of check_params, near and far in the units of the cameras.  Enqueue only."""
    cams = np.asarray(cams, np.float64)
    if nbr is None:
        nbr = DC.neighbours(cams.reshape(len(cams), -1)[:, [7, 11, 15]], check_views(views))
    prm = check_params(np.asarray(nbr).shape[1], **params)
    call = {k: prm[k] for k in ('planes', 'near', 'far', 'best_views', 'agg_radius', 'uniqueness', 'std_planes') + tuple(SMOOTH) if k in prm}
    t = sweep_async(rgb, cams, nbr, plane=False, cost=False, second=False, rows=True, **call).tensors
    std = t['std']
    if prm['std_floor'] > 0:
        std = std.clamp_min(prm['std_floor']) * (t['status'] == ACCEPTED)
    return t['depth'], std, t['status'], t['rows']


def totals_line(rows, views, planes):
    """The one log line of a load-time sweep; rows: int64 [F, 4] (host)"""
    rows = np.asarray(rows, np.int64)
    tot = rows.sum(0)
    px = max(int(tot.sum()), 1)
    return ('depth plane sweep (%d views, %d planes): %d frames, %d pixels accepted, %d at an end of the table, %d ambiguous, %d unseen '
            '(coverage %.1f %%)' % (views, planes, len(rows), tot[0], tot[1], tot[2], tot[3], 100.0 * tot[0] / px))


# -------------------------------------------------------------------------------------------------------- adapters
def sweep_samplers(samplers, device, views, want_std=False, **params):
    """The load-time sweep of the NeRF++ path: the prior of the ray samplers (one frame each, all of one size) is computed from their
    images and cameras and written into them (IO.write_back; with want_std its standard deviation too).  Returns the rows int64
    [F, 4] (host).  Every rank computes the same bits; nothing is communicated."""
    import torch
    from .depth_complete import guide_u8
    if any(s.img is None for s in samplers):
        raise DepthMvsError('--depth_mvs_views: the training frames carry no image to sweep')
    H, W = IO.one_size(samplers, '--depth_mvs_views: the frames differ in size; the sweep takes frames of one size', DepthMvsError)
    rgb = np.stack([guide_u8(s.img).reshape(H, W, 3) for s in samplers], 0)
    out, std, _, rows = sweep_priors(torch.from_numpy(rgb).to(device), DC.cams_from_samplers(samplers), views, **params)
    IO.write_back(samplers, out.cpu().numpy(), std.cpu().numpy() if want_std else None)
    return rows.cpu().numpy()


# ------------------------------------------------------------------------------------------------------ PNG encoding
encode_prior = IO.encode_metres          # the prior's PNG: the metres where accepted


def write_report(path, names, rows, status, out=None, gt=None):
    """mvs.txt: per frame and in total the four counts, the coverage (accepted pixels / pixels) and, where ground-truth depth
    exists, AbsRel of the accepted pixels against it"""
    have_gt = gt is not None
    px = int(np.prod(status.shape[1:]))
    IO.write_rows_report(path, names, rows, '%s coverage%s' % (' '.join(ROW_NAMES), ' absrel_accepted' if have_gt else ''),
                         lambda sel, r, n: ' %.6f%s' % (r[0] / (px * n), ' %.6f' % absrel(out[sel], gt[sel], status[sel] == ACCEPTED)
                                                        if have_gt else ''))


# --------------------------------------------------------------------------------------------------------------- CLI
def _run(rgb, cams, views, device, params):
    """(depth, std, status, rows) on the host"""
    import torch
    out = sweep_priors(torch.from_numpy(np.ascontiguousarray(rgb)).to(device), cams, views, **params)
    return tuple(t.cpu().numpy() for t in out)


def run_colmap(args, device):
    """The COLMAP layout: all frames of the scene together -> depths{sfx}_mvs/, depths{sfx}_mvs_std/, mvs.txt"""
    from . import mip360_data as D
    cfg = D.parse_gin(args.gin_configs, list(args.gin_bindings) + ['Config.data_dir = %r' % args.data_dir, "Config.depth_sup_type = 'mvs'",
                                                                   "Config.depth_loss_type = 'mse'"])
    for key in ('depth_cons_views', 'depth_acc_views', 'depth_comp_iters'):
        cfg[key] = 0
    cfg['depth_align_anchor'], cfg['depth_mvs_views'] = '', args.views     # (with the flag the Scene does not look for depths_mvs/)
    scene = D.Scene(cfg)
    out, std, status, rows = _run(scene.images, DC.cams_from_scene(scene), args.views, device, args_params(args, scene.scale, ''))
    out_dir = os.path.join(args.data_dir, 'depths%s_mvs' % IO.colmap_suffix(cfg))
    std_dir = out_dir + '_std'
    for d in (out_dir, std_dir):
        os.makedirs(d, exist_ok=True)
    for i, name in enumerate(scene.names):
        png = os.path.splitext(name)[0] + '.png'
        _write_png16(os.path.join(out_dir, png), encode_prior(out[i].astype(np.float64) / scene.scale, status[i] == ACCEPTED))
        _write_png16(os.path.join(std_dir, png), encode_std(std[i] / scene.scale, status[i] == ACCEPTED))
    report = os.path.join(args.data_dir, 'mvs.txt')
    write_report(report, scene.names, rows, status, out, scene.depths_gt)
    print(totals_line(rows, args.views, args.planes), flush=True)
    print('wrote %s, %s and %s' % (out_dir, std_dir, report), flush=True)
    return rows


def run_nerfpp(args, device):
    """The NeRF++ layout, each of train / test by itself -> {split}/depth_mvs/, {split}/depth_mvs_std/, {split}/mvs.txt"""
    from .depth_complete import guide_u8
    done = {}
    for split, split_dir, files, samplers in IO.nerfpp_splits(args, 'rgb', ['*.png', '*.jpg'], '{split}: no frames in {folder}'):
        H, W = IO.one_size(samplers, '%s: the frames differ in size; the sweep takes frames of one size' % split_dir, DepthMvsError)
        scale = float(getattr(samplers[0], 'depth_scale', None) or 1.0)
        rgb = np.stack([guide_u8(s.img).reshape(H, W, 3) for s in samplers], 0)
        out, std, status, rows = _run(rgb, DC.cams_from_samplers(samplers), args.views, device, args_params(args, scale, ''))
        out_dir, std_dir = os.path.join(split_dir, 'depth_mvs'), os.path.join(split_dir, 'depth_mvs_std')
        for d in (out_dir, std_dir):
            os.makedirs(d, exist_ok=True)
        names = IO.png_names(files)
        for i in range(len(files)):
            _write_png16(os.path.join(out_dir, names[i]), encode_prior(out[i].astype(np.float64) / scale, status[i] == ACCEPTED))
            _write_png16(os.path.join(std_dir, names[i]), encode_std(std[i] / scale, status[i] == ACCEPTED))
        report = os.path.join(split_dir, 'mvs.txt')
        write_report(report, names, rows, status, out, IO.stack_gt(samplers))
        print('%s: %s' % (split, totals_line(rows, args.views, args.planes)), flush=True)
        print('wrote %s, %s and %s' % (out_dir, std_dir, report), flush=True)
        done[split] = rows
    if not done:
        raise DepthMvsError('no frames under %s' % os.path.join(args.datadir, args.scene))
    return done


def make_parser():
    p = IO.base_parser('python -m outdoor_nerf_depth_amd.depth_mvs', __doc__)
    p.add_argument('--views', type=int, default=4, help='nearest frames every frame is swept against (1 .. %d; default 4)' % MAX_VIEWS)
    add_flags(p, '')
    IO.add_device_flag(p)
    return p


def main(argv=None):
    import torch
    args = make_parser().parse_args(argv)
    run = {'colmap': run_colmap, 'nerfpp': run_nerfpp}[IO.pick_layout(args)]
    try:
        check_params(args.views, **args_params(args, 1.0, ''))
    except DepthMvsError as e:
        raise SystemExit(str(e))
    return run(args, torch.device(args.device))


if __name__ == '__main__':
    main()

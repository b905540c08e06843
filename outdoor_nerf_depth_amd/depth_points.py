"""A sparse depth prior from the scene's own reconstruction on the device: the 3D points of the COLMAP model, z-buffered into the
frames, with a per-pixel standard deviation and the index of the winning point.  It is DS-NeRF's prior, the metric measurement every
COLMAP scene already carries: the anchor a monocular prior is aligned to (depth_align.py), a seed for the completion and the
accumulation, and a standard deviation for the 'gnll' loss.  ctypes binding of libdepthpoints_hip.so (include/depthpoints_hip.h),
the host side that selects the points, the adapters of both front ends, and the CLI

    python -m outdoor_nerf_depth_amd.depth_points --data_dir SCENE [--vis all] [--gin_bindings ...]                 (COLMAP layout)
    python -m outdoor_nerf_depth_amd.depth_points --datadir DIR --scene SCENE --points_model MODEL_DIR [--vis all]  (NeRF++ layout)

A point is used when its coordinates are finite, its mean reprojection error is at most `max_error` pixels, at least `min_track`
images of the model observe it and those images' cameras do not coincide.  `track` draws a point into the frames that observed it
(COLMAP matched it there, so it is visible there); `all` draws every point into every frame that holds it, which is denser and
relies on the visibility window: a point behind the nearest point of its (2 occl_radius + 1)^2 window by more than `occl_tol`
(relative) is hidden.  The nearest point of a pixel wins, the lower index among equal depths.  A kept pixel's standard deviation is
max(std_floor, std_scale * max(error, err_floor) / B * z^2 / fx) with B the diagonal of the bounding box of the observing cameras'
centres: the first-order two-view model dz = z^2 / (f B) d(disparity) with the reprojection error standing in for the disparity
error.  It is a model, nobody has measured it, and for forward motion it is optimistic: that is what std_scale and std_floor are
for.  The definition is DESIGN.md 8.12 (restated as code in tests/depth_points_reference.py).

Out of scope: distorted cameras (refused by name), splats wider than a pixel, the observed 2D keypoint instead of the projection,
dense clouds (fused.ply) and .ply input, moving objects, and reconstructions whose scale is not metric (points.txt's error against
depths_gt is where a wrong scale shows).

The COLMAP-layout CLI takes all frames together and writes depths_points/, depths_points_std/ and points.txt; the loaders then find
the result under `--depth_sup_type points`.  The NeRF++ layout holds normalised pose files and no reconstruction: --points_model
names the model, the frames are matched to its images by file stem, and the shift and scale between the two are fitted from the
matched camera centres (a run whose pose files are not a shifted, scaled copy of the model's cameras is refused).  The load-time
flags (Config.depth_points_vis, --depth_points_model) run the same call when a training run loads its frames instead, first of all;
they use the float32 value, which the CLI's folders round to the PNG's 1 / 256 m.

Everything is enqueued on torch's current stream and nothing synchronises until the numbers are read.  torch only allocates.
There is no host path: without libdepthpoints_hip.so and a device every call raises.
"""
import ctypes as C
import os

import numpy as np

from . import _ctypes_util as U
from . import depth_prior_io as IO
from .depth_consistency import pack_cams, validate, cams_from_scene, cams_from_samplers, DepthConsError, CAM   # noqa: F401
from .depth_prior_io import write_png16 as _write_png16, absrel   # noqa: F401
from .depth_points_flags import PARAMS, MODES, DEFAULT_RADIUS, MAX_RADIUS, add_flags, args_params, scene_params   # noqa: F401

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get('DEPTHPOINTS_HIP_LIB') or os.path.join(_HERE, 'libdepthpoints_hip.so')
ABI_VERSION = 1
MAX_FRAMES = 65535
MAX_POINTS = 2 ** 31 - 1
ROW_NAMES = ('n_obs', 'n_projected', 'n_kept', 'n_hidden')
ORIGIN_NONE, ORIGIN_POINT, ORIGIN_HIDDEN = 0, 1, 2
FIT_TOL = 1e-6                    # largest residual of the fitted shift and scale, relative to the largest centred camera centre
HOST_PARAMS = ('max_error', 'min_track', 'err_floor')
CALL_PARAMS = ('near', 'far', 'occl_radius', 'occl_tol', 'std_scale', 'std_floor')

_fp = C.c_void_p
# every symbol include/depthpoints_hip.h declares: name -> (restype, argtypes)
SYMBOLS = {
    'depthpoints_last_error': (C.c_char_p, []),
    'depthpoints_abi_version': (C.c_int, []),
    'depthpoints_workspace_bytes': (C.c_int64, [C.c_int, C.c_int, C.c_int]),
    'depthpoints_splat': (C.c_int, [_fp, C.c_int, C.c_int, C.c_int, _fp, C.c_int64, _fp, C.c_int64, _fp, C.c_double, C.c_double, C.c_int,
                                    C.c_double, C.c_double, C.c_double, _fp, _fp, _fp, _fp, _fp, _fp]),
}

_lib = None


class DepthPointsError(DepthConsError):
    pass


def _shared(fn, *args):
    """fn(*args) of depth_consistency's host side, its refusals raised as this module's error"""
    try:
        return fn(*args)
    except DepthPointsError:
        raise
    except DepthConsError as e:
        raise DepthPointsError(str(e)) from None


def lib():
    """The loaded library with typed prototypes.  Raises if it has not been built."""
    global _lib
    if _lib is None:
        _lib = U.load(LIB_PATH, 'libdepthpoints_hip.so', SYMBOLS, 'depthpoints_abi_version', ABI_VERSION, DepthPointsError,
                      ' (hipcc --offload-arch=gfx950). There is no CPU fallback for the sparse-point depth prior.')
    return _lib


def last_error():
    return lib().depthpoints_last_error().decode('utf-8', 'replace')


check = U.checker(lib, 'depthpoints_last_error', DepthPointsError, 'depthpoints call')


def workspace_bytes(n_frames, height, width):
    """Size of the scratch buffer of a call on n_frames frames of height x width pixels (the 8-byte z-buffer, the row partials and the
    counters); raises DepthPointsError for sizes the library rejects (n_frames outside 1 .. 65535, height * width outside 1 .. 2^28).
    Needs no GPU."""
    return U.size(lib().depthpoints_workspace_bytes(int(n_frames), int(height), int(width)), last_error, DepthPointsError)


_workspaces = U.Workspaces(workspace_bytes, 2, 'float64')


def check_params(vis='track', max_error=2.0, min_track=3, err_floor=0.5, near=0.5, far=200.0, occl_radius=None, occl_tol=0.05,
                 std_scale=1.0, std_floor=0.0):
    """The mode and the nine parameters as the host selection and the call take them; near, far and std_floor in the units of the
    cameras; occl_radius None = the mode's default (0 for track, 4 for all)"""
    if vis not in MODES:
        raise DepthPointsError('vis = %r: expected %s' % (vis, ' or '.join(repr(m) for m in MODES)))
    radius = DEFAULT_RADIUS[vis] if occl_radius is None else occl_radius
    p = dict(vis=vis, max_error=float(max_error), min_track=int(min_track), err_floor=float(err_floor), near=float(near), far=float(far),
             occl_radius=int(radius), occl_tol=float(occl_tol), std_scale=float(std_scale), std_floor=float(std_floor))
    if not (np.isfinite(p['max_error']) and p['max_error'] >= 0):
        raise DepthPointsError('max_error = %r: expected a finite number of pixels >= 0' % max_error)
    if p['min_track'] < 1 or p['min_track'] != min_track:
        raise DepthPointsError('min_track = %r: expected an integer >= 1' % (min_track,))
    if not (np.isfinite(p['err_floor']) and p['err_floor'] >= 0):
        raise DepthPointsError('err_floor = %r: expected a finite number of pixels >= 0' % err_floor)
    if not (np.isfinite(p['near']) and np.isfinite(p['far']) and 0 < p['near'] < p['far']):
        raise DepthPointsError('near = %r, far = %r: expected finite numbers with 0 < near < far' % (near, far))
    if not 0 <= p['occl_radius'] <= MAX_RADIUS or p['occl_radius'] != radius:
        raise DepthPointsError('occl_radius = %r: expected an integer 0 .. %d' % (occl_radius, MAX_RADIUS))
    if not (np.isfinite(p['occl_tol']) and p['occl_tol'] >= 0):
        raise DepthPointsError('occl_tol = %r: expected a finite number >= 0' % occl_tol)
    if not (np.isfinite(p['std_scale']) and p['std_scale'] > 0):
        raise DepthPointsError('std_scale = %r: expected a finite number > 0' % std_scale)
    if not (np.isfinite(p['std_floor']) and p['std_floor'] >= 0):
        raise DepthPointsError('std_floor = %r: expected a finite number >= 0' % std_floor)
    return p


def _split(prm):
    """(vis, the host selection's parameters, the call's) of check_params' dict"""
    return prm['vis'], {k: prm[k] for k in HOST_PARAMS}, {k: prm[k] for k in CALL_PARAMS}


# ---------------------------------------------------------------------------------------------------- the host side
def select_points(xyz, error, off, track_pos, centres, frame_of, max_error=2.0, min_track=3, err_floor=0.5):
    """(points float64 [P', 4] = x y z coef, obs int32 [T', 2] = (point, frame) sorted by (frame, point)) of a cloud in the cameras'
    frame.  xyz [P, 3], error [P]; the track of point p is track_pos[off[p]:off[p + 1]], positions into centres [N, 3] (all the
    model's cameras); frame_of [N]: a camera's position among the frames of the call, or -1.  A point is kept iff its coordinates are
    finite, 0 <= error <= max_error, its track has at least min_track entries (over the whole model) and B > 0, the diagonal of the
    bounding box of its track's camera centres; coef = max(error, err_floor) / B."""
    xyz, error = np.asarray(xyz, np.float64).reshape(-1, 3), np.asarray(error, np.float64).reshape(-1)
    off, track_pos = np.asarray(off, np.int64), np.asarray(track_pos, np.int64)
    centres, frame_of = np.asarray(centres, np.float64).reshape(-1, 3), np.asarray(frame_of, np.int64)
    P = len(xyz)
    length = np.diff(off)
    B = np.zeros(P, np.float64)
    if track_pos.size:
        c = centres[track_pos]
        some = length > 0
        starts = off[:-1][some]                                      # (an empty track between two others adds no entry to either)
        d = np.maximum.reduceat(c, starts, axis=0) - np.minimum.reduceat(c, starts, axis=0)
        dx, dy, dz = d[:, 0], d[:, 1], d[:, 2]
        B[some] = np.sqrt((dx * dx + dy * dy) + dz * dz)
    with np.errstate(invalid='ignore'):
        keep = np.isfinite(xyz).all(1) & (error >= 0) & (error <= max_error) & (length >= min_track) & (B > 0)
    with np.errstate(all='ignore'):
        coef = np.maximum(error, err_floor) / B
    points = np.concatenate([xyz[keep], coef[keep, None]], 1)
    new_index = np.cumsum(keep) - 1
    owner = np.repeat(np.arange(P), length)
    frame = frame_of[track_pos] if track_pos.size else np.zeros(0, np.int64)
    sel = keep[owner] & (frame >= 0)
    p, f = new_index[owner[sel]], frame[sel]
    order = np.lexsort((p, f))
    return np.ascontiguousarray(points), np.ascontiguousarray(np.stack([p[order], f[order]], 1).astype(np.int32))


def _track_positions(image_id, images, position_of_name, what):
    """track entries (COLMAP image ids) -> positions of those images in a list of names; an id the model does not hold is refused"""
    ids, inverse = np.unique(np.asarray(image_id, np.int64), return_inverse=True)
    pos = np.empty(len(ids), np.int64)
    for k, iid in enumerate(ids.tolist()):
        if iid not in images:
            raise DepthPointsError('%s: a track names image id %d, which is not among the model\'s images' % (what, iid))
        pos[k] = position_of_name[images[iid][3]]
    return pos[inverse.reshape(-1)] if len(ids) else np.zeros(0, np.int64)


def scene_points(scene, idx=None, max_error=2.0, min_track=3, err_floor=0.5):
    """(points float64 [P', 4], obs int32 [T', 2]) of a MipNeRF-360 Scene and the frames idx of it (None = all): the model's 3D points
    taken into the scene's frame with scene.transform -- the similarity the poses went through, so z-depths come out in scene units
    like depths_sup -- and selected by select_points; the tracks' COLMAP image ids become positions in idx by image name, and entries
    outside idx become no observation (they still count towards min_track and B)."""
    from . import mip360_data as D
    _, images = D.read_model(scene.sparse_dir)
    xyz, error, off, image_id = D.read_points3d(scene.sparse_dir)
    names = list(scene.names)
    track_pos = _track_positions(image_id, images, {n: i for i, n in enumerate(names)}, scene.sparse_dir)
    frame_of = np.full(len(names), -1, np.int64)
    idx = np.arange(len(names)) if idx is None else np.asarray(idx, np.int64)
    frame_of[idx] = np.arange(len(idx))
    T = np.asarray(scene.transform, np.float64)
    xyz = xyz @ T[:3, :3].T + T[:3, 3]
    return select_points(xyz, error, off, track_pos, np.asarray(scene.poses, np.float64)[:, :3, 3], frame_of, max_error, min_track, err_floor)


def fit_similarity(model_centres, centres, names):
    """(s, t) with centres = s model_centres + t: the closed-form fit of a shift and a scale (no rotation) to matched camera centres,
    s = sum((c' - mean c') . (c - mean c)) / sum |c - mean c|^2 and t = mean c' - s mean c.  Refused, with the worst frame's name,
    when max |s c + t - c'| exceeds 1e-6 of the largest centred |c'|."""
    c, c2 = np.asarray(model_centres, np.float64).reshape(-1, 3), np.asarray(centres, np.float64).reshape(-1, 3)
    if len(c) != len(c2) or len(c) != len(names):
        raise DepthPointsError('fit_similarity: %d model centres, %d centres and %d names' % (len(c), len(c2), len(names)))
    dc, dc2 = c - c.mean(0), c2 - c2.mean(0)
    den = float((dc * dc).sum())
    if len(c) < 2 or not den > 0:
        raise DepthPointsError('the shift and scale between the pose files and the model need at least two frames whose cameras do not '
                               'coincide (%d frames)' % len(c))
    s = float((dc2 * dc).sum()) / den
    t = c2.mean(0) - s * c.mean(0)
    res = np.sqrt((((s * c + t) - c2) ** 2).sum(1))
    extent = float(np.sqrt((dc2 * dc2).sum(1)).max())
    worst = int(np.argmax(res))
    if not (s > 0 and res[worst] <= FIT_TOL * extent):
        raise DepthPointsError('the pose files are not a shifted, scaled copy of the model\'s cameras: with the fitted scale %.9g frame %s '
                               'is off by %.3g, %.3g of the cameras\' extent (at most %g; a rotated or re-optimised set of poses does not '
                               'carry the model\'s points)' % (s, names[worst], res[worst], res[worst] / extent, FIT_TOL))
    return s, t


def model_points(model_dir, stems, centres, max_error=2.0, min_track=3, err_floor=0.5):
    """(points, obs, s) of a COLMAP model directory and frames that are a shifted, scaled copy of some of its cameras: stems are the
    frames' file stems, matched to the model's image names by stem, centres [F, 3] their camera centres.  The points come out in the
    frames' units; s is the fitted scale."""
    from . import mip360_data as D
    _, images = D.read_model(model_dir)
    xyz, error, off, image_id = D.read_points3d(model_dir)
    names, model_centres = [], []
    for iid in images:
        q, t, _, name = images[iid]
        names.append(name)
        model_centres.append(-D.qvec_to_rotmat(q).T @ t)
    model_centres = np.asarray(model_centres, np.float64).reshape(-1, 3)
    by_stem = {os.path.splitext(os.path.basename(n))[0]: i for i, n in enumerate(names)}
    missing = [s for s in stems if s not in by_stem]
    if missing:
        raise DepthPointsError('frame %s is missing from the model in %s (%d of %d frames are; frames are matched to the model\'s images '
                               'by file stem)' % (missing[0], model_dir, len(missing), len(stems)))
    where = np.array([by_stem[s] for s in stems], np.int64)
    s, t = fit_similarity(model_centres[where], centres, list(stems))
    frame_of = np.full(len(names), -1, np.int64)
    frame_of[where] = np.arange(len(stems))
    track_pos = _track_positions(image_id, images, {n: i for i, n in enumerate(names)}, model_dir)
    points, obs = select_points(s * xyz + t, error, off, track_pos, s * model_centres + t, frame_of, max_error, min_track, err_floor)
    return points, obs, s


# ---------------------------------------------------------------------------------------------------- the call
def _host_inputs(cams, points, obs, shape):
    """(cams [F, 16], points [P, 4], obs int32 [T, 2] or None, (F, H, W)) checked on the host before upload"""
    cams_h, _ = _shared(validate, cams, np.zeros((len(np.asarray(cams)), 0), np.int32))
    if len(tuple(shape)) != 3:
        raise DepthPointsError('shape: expected (F, H, W), got %r' % (tuple(shape),))
    F, H, W = (int(v) for v in shape)
    if cams_h.shape[0] != F:
        raise DepthPointsError('cams: %d cameras for %d frames' % (cams_h.shape[0], F))
    points = np.ascontiguousarray(points, np.float64)
    if points.ndim != 2 or points.shape[1] != 4:
        raise DepthPointsError('points: expected float64 [P, 4] (x, y, z, coef), got %s' % (tuple(points.shape),))
    if len(points) > MAX_POINTS:
        raise DepthPointsError('points: %d points, at most 2^31 - 1' % len(points))
    if obs is not None:
        obs = np.asarray(obs)
        if obs.dtype.kind not in 'iu':
            raise DepthPointsError('obs: expected an integer array, got %s' % obs.dtype)
        if obs.ndim != 2 or obs.shape[1] != 2:
            raise DepthPointsError('obs: expected [T, 2] (point, frame), got %s' % (tuple(obs.shape),))
        bad = (obs[:, 0] < 0) | (obs[:, 0] >= len(points))
        if bad.any():
            row = int(np.argmax(bad))
            raise DepthPointsError('obs: row %d names point %d, but the table holds %d points' % (row, int(obs[row, 0]), len(points)))
        obs = np.ascontiguousarray(np.clip(obs, -1, 2 ** 31 - 1), np.int32)       # (a frame outside the call is skipped on the device)
    return cams_h, points, obs, (F, H, W)


def _device(device):
    import torch
    dev = torch.device('cuda' if device is None else device)
    if dev.type != 'cuda':
        raise DepthPointsError('device %s: expected a CUDA/HIP device (the sparse-point depth prior has no CPU path)' % dev)
    return torch.device('cuda', torch.cuda.current_device()) if dev.index is None else dev


def upload(cams_h, points_h, obs_h, device):
    """(cams_d, points_d, obs_d or None, n_points, n_obs) on the device, of _host_inputs' arrays"""
    import torch
    dev = _device(device)
    up = lambda a: torch.from_numpy(a if a.flags.writeable else a.copy()).to(dev)      # (torch takes no read-only array)
    # (an empty tensor has no address: a table without rows is still a table, and obs_d's address is what selects the mode)
    points_d = up(points_h) if len(points_h) else torch.zeros((1, 4), dtype=torch.float64, device=dev)
    obs_d = None
    if obs_h is not None:
        obs_d = up(obs_h) if len(obs_h) else torch.zeros((1, 2), dtype=torch.int32, device=dev)
    return up(cams_h), points_d, obs_d, len(points_h), 0 if obs_h is None else len(obs_h)


def enqueue(cams_d, points_d, obs_d, n_points, n_obs, shape, prm, std=True, point=True, origin=True, rows=True, out=None):
    """The library call alone, on tables that upload() put on the device: Pending.  prm: check_params() of the mode obs_d selects.
    out: the `.tensors` of an earlier call of the same shape and outputs, to write into again instead of allocating."""
    import torch
    F, H, W = shape
    dev = cams_d.device
    with torch.cuda.device(dev):
        ws = _workspaces.buffer(dev, F, H, W)
        if out is None:
            out = {'depth': torch.empty((F, H, W), dtype=torch.float32, device=dev)}
            if std:
                out['std'] = torch.empty((F, H, W), dtype=torch.float32, device=dev)
            if point:
                out['point'] = torch.empty((F, H, W), dtype=torch.int32, device=dev)
            if origin:
                out['origin'] = torch.empty((F, H, W), dtype=torch.uint8, device=dev)
            if rows:
                out['rows'] = torch.empty((F, len(ROW_NAMES)), dtype=torch.int64, device=dev)
        check(lib().depthpoints_splat(U.stream(), F, H, W, U.p(cams_d), n_points, U.p(points_d), n_obs, U.p(obs_d), prm['near'], prm['far'],
                                      prm['occl_radius'], prm['occl_tol'], prm['std_scale'], prm['std_floor'], U.p(ws), U.p(out['depth']),
                                      U.p(out.get('std')), U.p(out.get('point')), U.p(out.get('origin')), U.p(out.get('rows'))),
              'depthpoints_splat')
    return U.Pending(out, (cams_d, points_d, obs_d, ws))


def splat_async(cams, points, obs, shape, device=None, near=0.5, far=200.0, occl_radius=None, occl_tol=0.05, std_scale=1.0, std_floor=0.0,
                std=True, point=True, origin=True, rows=True):
    """Pending of the splat of the host arrays points float64 [P, 4] (x, y, z, coef) into shape = (F, H, W) frames with cams float64
    [F, 16] (pack_cams).  obs int [T, 2] = (point, frame): the `track` mode, a point goes into the frames that observed it; a row
    whose point is outside the table is refused with its number, one whose frame is outside the call is skipped.  obs None: the `all`
    mode, every point into every frame.  occl_radius None = the mode's default.  `.tensors`: 'depth' float32 [F, H, W] (0 where no
    point is kept) and, when asked, 'std' float32, 'point' int32 (-1 where none), 'origin' uint8 (0 nothing, 1 point, 2 hidden)
    and 'rows' int64 [F, 4] in ROW_NAMES' order.  Everything is checked on the host first; then three uploads and the library
    call.  Enqueue only."""
    prm = check_params('all' if obs is None else 'track', near=near, far=far, occl_radius=occl_radius, occl_tol=occl_tol,
                       std_scale=std_scale, std_floor=std_floor)
    cams_h, points_h, obs_h, shape = _host_inputs(cams, points, obs, shape)
    return enqueue(*upload(cams_h, points_h, obs_h, _device(device)), shape, prm, std, point, origin, rows)


def splat_priors(cams, points, obs, shape, device=None, **params):
    """(depth float32 [F, H, W], std float32 [F, H, W], point int32 [F, H, W], rows int64 [F, 4]) on the device: splat_async's
    tensors.  params: the six of the call.  Enqueue only."""
    t = splat_async(cams, points, obs, shape, device, std=True, point=True, origin=False, rows=True, **params).tensors
    return t['depth'], t['std'], t['point'], t['rows']


def totals_line(rows, vis):
    """The one log line of a load-time splat; rows: int64 [F, 4] (host)"""
    rows = np.asarray(rows, np.int64)
    tot = rows.sum(0)
    empty = int((rows[:, 2] == 0).sum())
    return ('sparse-point depth prior (%s): %d frames, %d observations, %d projected, %d pixels kept (%.1f per frame), %d hidden%s'
            % (vis, len(rows), tot[0], tot[1], tot[2], tot[2] / max(len(rows), 1), tot[3],
               '' if empty == 0 else ' -- %d frames are left without a point' % empty))


# -------------------------------------------------------------------------------------------------------- adapters
def splat_scene(scene, idx, device, prm):
    """The load-time splat of the MipNeRF-360 path: (depth, std, point, rows) on the device for the frames idx of the scene; prm:
    check_params()"""
    vis, host, call = _split(prm)
    points, obs = scene_points(scene, idx, **host)
    return splat_priors(cams_from_scene(scene, idx), points, obs if vis == 'track' else None, (len(idx), scene.height, scene.width),
                        device, **call)


def _sampler_stem(s, i):
    if not getattr(s, 'img_path', None):
        raise DepthPointsError('--depth_points_model: frame %d has no image file to match to the model\'s images by file stem' % i)
    return os.path.splitext(os.path.basename(s.img_path))[0]


def splat_samplers(samplers, device, model_dir, vis='track', target='prior', want_std=False, **params):
    """The load-time splat of the NeRF++ path: the 3D points of the COLMAP model in model_dir, fitted to the ray samplers' cameras
    (one frame each, all of one size; matched by file stem), drawn into every frame.  target 'prior': written into the samplers
    (IO.write_back; with want_std the standard deviation too); 'anchor': the samplers are left alone.  Returns (rows int64 [F, 4]
    (host), depth float32 [F, H * W] (host)).  params: near, far and std_floor in scene units.  Every rank computes the same bits."""
    vis, host, call = _split(check_params(vis, **params))
    H, W = IO.one_size(samplers, '--depth_points_model: the frames differ in size; the splat takes frames of one size', DepthPointsError)
    cams = _shared(cams_from_samplers, samplers)
    points, obs, _ = model_points(model_dir, [_sampler_stem(s, i) for i, s in enumerate(samplers)], cams[:, [7, 11, 15]], **host)
    depth, std, _, rows = splat_priors(cams, points, obs if vis == 'track' else None, (len(samplers), H, W), device, **call)
    depth = depth.cpu().numpy().reshape(len(samplers), -1)
    if target == 'prior':
        IO.write_back(samplers, depth, std.cpu().numpy() if want_std else None)
    return rows.cpu().numpy(), depth


class _Anchor(object):
    """What depth_align.align_samplers reads of an anchor's sampler"""

    def __init__(self, sampler, depth):
        self.H, self.W, self.depth_sup = sampler.H, sampler.W, depth


def anchors_of(samplers, depth):
    return [_Anchor(s, depth[i]) for i, s in enumerate(samplers)]


# ------------------------------------------------------------------------------------------------------ PNG encoding
encode = IO.encode_metres                # the PNGs of depth and standard deviation: the metres where a point is kept


def write_report(path, names, rows, depth, gt=None):
    """points.txt: per frame and in total the four counts, the coverage (kept pixels / pixels) and, where ground-truth depth exists,
    the mean absolute relative error of the kept pixels against it where both are valid"""
    px = int(np.prod(depth.shape[1:]))
    IO.write_rows_report(path, names, rows, '%s coverage%s' % (' '.join(ROW_NAMES), '' if gt is None else ' absrel'),
                         lambda sel, r, n: ' %.6f%s' % (r[2] / (px * n), '' if gt is None else ' %.6f' % absrel(depth[sel], gt[sel], depth[sel] > 0)))


def _write_frames(out_dir, names, depth, std, scale):
    """depth and std (scene units) as 16-bit PNGs of metres x 256 in out_dir and out_dir + '_std'"""
    for d in (out_dir, out_dir + '_std'):
        os.makedirs(d, exist_ok=True)
    for i, name in enumerate(names):
        kept = depth[i] > 0
        _write_png16(os.path.join(out_dir, name), encode(depth[i].astype(np.float64) / scale, kept))
        _write_png16(os.path.join(out_dir + '_std', name), encode(std[i].astype(np.float64) / scale, kept))


# --------------------------------------------------------------------------------------------------------------- CLI
def run_colmap(args, device):
    """The COLMAP layout: all frames of the scene together -> depths{sfx}_points/, depths{sfx}_points_std/, points.txt"""
    from . import mip360_data as D
    cfg = D.parse_gin(args.gin_configs, list(args.gin_bindings) + ['Config.data_dir = %r' % args.data_dir,
                                                                   "Config.depth_sup_type = 'gt'", "Config.depth_loss_type = 'mse'"])
    for k in ('depth_cons_views', 'depth_acc_views', 'depth_comp_iters', 'depth_mvs_views'):
        cfg[k] = 0
    cfg['depth_align_anchor'] = cfg['depth_points_vis'] = ''
    scene = D.Scene(cfg)
    prm = check_params(args.vis, **args_params(args, scene.scale, ''))
    idx = np.arange(len(scene.names))
    depth, std, _, rows = splat_scene(scene, idx, device, prm)
    depth, std, rows = depth.cpu().numpy(), std.cpu().numpy(), rows.cpu().numpy()
    sfx = IO.colmap_suffix(cfg)
    gt_dir = os.path.join(args.data_dir, 'depths_gt' + sfx)
    to_gt = dict(zip(D._listdir(os.path.join(args.data_dir, 'images')), D._listdir(gt_dir)))
    out_dir = os.path.join(args.data_dir, 'depths%s_points' % sfx)
    _write_frames(out_dir, [to_gt[n] for n in scene.names], depth, std, scene.scale)
    report = os.path.join(args.data_dir, 'points.txt')
    write_report(report, scene.names, rows, depth, scene.depths_gt)
    print(totals_line(rows, args.vis), flush=True)
    print('wrote %s, %s_std and %s' % (out_dir, out_dir, report), flush=True)
    return rows


def _pose_centres(split_dir, stems):
    """float64 [F, 3, 4] camera-to-world of {split}/pose/{stem}.txt"""
    out = []
    for s in stems:
        with open(os.path.join(split_dir, 'pose', s + '.txt')) as f:
            out.append(np.array([float(v) for v in f.read().split()], np.float64).reshape(4, 4)[:3])
    return np.stack(out, 0)


def run_nerfpp(args, device):
    """The NeRF++ layout, each of train / test by itself -> {split}/depth_points/, {split}/depth_points_std/, {split}/points.txt.
    Returns {split: (rows, fitted scale)}."""
    if not args.points_model:
        raise DepthPointsError('--datadir holds pose files and no reconstruction: name the COLMAP model with --points_model')
    done = {}
    for split, split_dir, files, samplers in IO.nerfpp_splits(args, 'pose', ['*.txt'], '{split}: no frames in {split_dir}',
                                                               try_load_min_depth=False):
        stems = [os.path.splitext(os.path.basename(p))[0] for p in files]
        H, W, scale = samplers[0].H, samplers[0].W, float(samplers[0].depth_scale or 1.0)
        vis, host, call = _split(check_params(args.vis, **args_params(args, scale, '')))
        c2w = _pose_centres(split_dir, stems)                        # (float64: the samplers hold the pose files rounded to float32)
        cams = pack_cams(np.stack([np.asarray(s.intrinsics, np.float64)[:3, :3] for s in samplers], 0), c2w, split_dir)
        points, obs, s_fit = model_points(args.points_model, stems, c2w[:, :, 3], **host)
        depth, std, _, rows = splat_priors(cams, points, obs if vis == 'track' else None, (len(stems), H, W), device, **call)
        depth, std, rows = depth.cpu().numpy(), std.cpu().numpy(), rows.cpu().numpy()
        names = [s + '.png' for s in stems]
        out_dir = os.path.join(split_dir, 'depth_points')
        _write_frames(out_dir, names, depth, std, scale)
        report = os.path.join(split_dir, 'points.txt')
        write_report(report, names, rows, depth, IO.stack_gt(samplers))
        print('%s: fitted scale %.12g; %s' % (split, s_fit, totals_line(rows, vis)), flush=True)
        print('wrote %s, %s_std and %s' % (out_dir, out_dir, report), flush=True)
        done[split] = (rows, s_fit)
    if not done:
        raise DepthPointsError('no frames under %s' % os.path.join(args.datadir, args.scene))
    return done


def make_parser():
    p = IO.base_parser('python -m outdoor_nerf_depth_amd.depth_points', __doc__)
    p.add_argument('--points_model', default='', help='with --datadir: the COLMAP model directory (cameras, images, points3D) the scene\'s '
                   'pose files are a shifted, scaled copy of')
    p.add_argument('--vis', default='track', choices=MODES, help='track: a point goes into the frames that observed it; all: into every '
                   'frame that holds it, behind the visibility window (default track)')
    add_flags(p, '')
    IO.add_device_flag(p)
    return p


def main(argv=None):
    import torch
    args = make_parser().parse_args(argv)
    run = {'colmap': run_colmap, 'nerfpp': run_nerfpp}[IO.pick_layout(args, ' and --points_model')]
    return run(args, torch.device(args.device))


if __name__ == '__main__':
    main()

"""Multi-view consistency check of depth priors on the device: the depth-map filter of multi-view stereo applied to the priors
before training.  ctypes binding of libdepthcons_hip.so (include/depthcons_hip.h), the adapters of both front ends, and the CLI

    python -m outdoor_nerf_depth_amd.depth_consistency --data_dir SCENE --depth_sup_type T [--gin_bindings ...]      (COLMAP layout)
    python -m outdoor_nerf_depth_amd.depth_consistency --datadir DIR --scene SCENE --depth_sup_type T                (NeRF++ layout)

Every valid prior pixel of every posed frame is taken into its `views` nearest frames and back.  It is kept when at least
`min_views` of them agree (reprojection within `pix_tol` pixels, depth within `rel_tol` of its own), and the spread of what they
say is its standard deviation: the per-pixel input the 'gnll' depth loss needs.  A pixel fewer than `min_views` neighbours can
see is kept or dropped by `keep_unverified` (kept by default: a sparse LiDAR prior has almost no evidence in a neighbour).  The
definition is DESIGN.md 8.7 (restated as code in tests/depth_consistency_reference.py).

The check applies to priors that are metric in the scene's frame (LiDAR, completion, stereo, aligned monocular depth).  Relative
priors -- what the 'ssi' loss is for -- do not reproject and are out of scope.  It is pinhole-only.

The CLI writes, next to the prior, the folder the loaders already find under `--depth_sup_type T_cons` and its `_std` twin, which
'gnll' already finds, plus consistency_T.txt with the counts.  The load-time flags (Config.depth_cons_views,
--depth_cons_views) run the same call when a training run loads its frames instead.  For COLMAP scenes the CLI checks all frames
together while the flag checks the training split, so the neighbour sets (and with them a few decisions) can differ.

Everything is enqueued on torch's current stream and nothing synchronises until the numbers are read.  torch only allocates.
There is no host path: without libdepthcons_hip.so and a device every call raises.
"""
import ctypes as C
import os

import numpy as np

from . import _ctypes_util as U
from . import depth_prior_io as IO

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get('DEPTHCONS_HIP_LIB') or os.path.join(_HERE, 'libdepthcons_hip.so')
OK = 0
ABI_VERSION = 1
MAX_FRAMES = 65535
MAX_VIEWS = 16
CAM = 16                          # fx fy cx cy + the 3 x 4 camera-to-world, row-major
ROW_NAMES = ('n_valid', 'n_verifiable', 'n_kept', 'n_dropped')
ORTHO_TOL = 1e-6
# the five parameters: name -> (default, help)
PARAMS = {
    'min_views': (2, 'neighbours that must agree with a prior pixel to keep it, and that must see it to judge it at all'),
    'pix_tol': (1.0, 'largest reprojection error, in pixels, of a neighbour that agrees'),
    'rel_tol': (0.01, 'largest depth difference, relative to the pixel\'s own depth, of a neighbour that agrees'),
    'keep_unverified': (True, 'keep (1) or drop (0) the prior pixels that fewer than min_views neighbours can see'),
    'std_floor': (0.0, 'smallest standard deviation reported, in metres; give a positive one when the spread feeds gnll at load time: neighbours '
                       'that agree exactly report 0, which gnll reads as no standard deviation (the CLI\'s folders hold at least 2 / 256 m)'),
}
VIEWS_HELP = ('check the depth prior of the training frames against each frame\'s N nearest frames on the device when they are loaded, '
              'drop the pixels their neighbours contradict and, for a depth loss that needs the standard deviation and finds neither '
              'a folder nor a constant, use the spread of what the neighbours say (0 = off; 1 .. %d)' % MAX_VIEWS)

_fp = C.c_void_p
# every symbol include/depthcons_hip.h declares: name -> (restype, argtypes)
SYMBOLS = {
    'depthcons_last_error': (C.c_char_p, []),
    'depthcons_abi_version': (C.c_int, []),
    'depthcons_workspace_bytes': (C.c_int64, [C.c_int, C.c_int, C.c_int]),
    'depthcons_check': (C.c_int, [_fp, C.c_int, C.c_int, C.c_int, C.c_int, _fp, _fp, _fp, C.c_double, C.c_double, C.c_int, C.c_int,
                                  C.c_double, _fp, _fp, _fp, _fp, _fp]),
}

_lib = None


class DepthConsError(RuntimeError):
    pass


def lib():
    """The loaded library with typed prototypes.  Raises if it has not been built."""
    global _lib
    if _lib is None:
        _lib = U.load(LIB_PATH, 'libdepthcons_hip.so', SYMBOLS, 'depthcons_abi_version', ABI_VERSION, DepthConsError,
                      ' (hipcc --offload-arch=gfx950). There is no CPU fallback for the consistency check.')
    return _lib


def last_error():
    return lib().depthcons_last_error().decode('utf-8', 'replace')


check = U.checker(lib, 'depthcons_last_error', DepthConsError, 'depthcons call')


def workspace_bytes(n_frames, height, width):
    """Size of the scratch buffer of a call on n_frames frames of height x width pixels; raises DepthConsError for sizes the library
    rejects (n_frames outside 1 .. 65535, height * width outside 1 .. 2^28).  Needs no GPU."""
    return U.size(lib().depthcons_workspace_bytes(int(n_frames), int(height), int(width)), last_error, DepthConsError)


_workspaces = U.Workspaces(workspace_bytes, 2, 'int32')


# ------------------------------------------------------------------------------------------------------ host side
def neighbours(centres, k):
    """int32 [F, k]: the k nearest OTHER frames of every frame by camera-centre distance in float64, ordered by (distance, index)
    -- ties go to the lower index -- and padded with -1 when there are fewer than k others."""
    c = np.asarray(centres, np.float64)
    if c.ndim != 2 or c.shape[1] != 3:
        raise DepthConsError('centres: expected [F, 3], got %s' % (tuple(c.shape),))
    k = int(k)
    if not 0 <= k <= MAX_VIEWS:
        raise DepthConsError('k = %d neighbours: expected 0 .. %d' % (k, MAX_VIEWS))
    F = c.shape[0]
    out = np.full((F, k), -1, np.int32)
    for i in range(F):
        d = c - c[i]
        dist2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
        order = [j for j in np.lexsort((np.arange(F), dist2)) if j != i][:k]      # sorted by dist2, then by index
        out[i, :len(order)] = order
    return out


def pack_cams(K, c2w, name='cams'):
    """float64 [F, 16] of K [3, 3] or [F, 3, 3] (nonzero skew is refused) and camera-to-world c2w [F, 3 or 4, 4], OpenCV axes"""
    c2w = np.asarray(c2w, np.float64)
    if c2w.ndim != 3 or c2w.shape[1] not in (3, 4) or c2w.shape[2] != 4:
        raise DepthConsError('%s: camera-to-world [F, 3 or 4, 4], got %s' % (name, tuple(c2w.shape)))
    F = c2w.shape[0]
    K = np.broadcast_to(np.asarray(K, np.float64).reshape(-1, 3, 3), (F, 3, 3))
    skew = np.abs(K[:, 0, 1])
    if np.any(skew != 0):
        raise DepthConsError('%s: frame %d has skew %g in its intrinsics: the check is for pinhole cameras without skew'
                             % (name, int(np.argmax(skew != 0)), float(K[int(np.argmax(skew != 0)), 0, 1])))
    out = np.empty((F, CAM), np.float64)
    out[:, 0], out[:, 1], out[:, 2], out[:, 3] = K[:, 0, 0], K[:, 1, 1], K[:, 0, 2], K[:, 1, 2]
    out[:, 4:] = c2w[:, :3, :4].reshape(F, 12)
    return out


def validate(cams, nbr):
    """(cams float64 [F, 16], nbr int32 [F, K]) checked on the host before upload: intrinsics positive, rotations orthonormal to
    1e-6, no neighbour equal to its own frame, none repeated, all below F (-1 = no neighbour)."""
    cams = np.ascontiguousarray(cams, np.float64)
    if cams.ndim != 2 or cams.shape[1] != CAM:
        raise DepthConsError('cams: expected float64 [F, %d], got %s' % (CAM, tuple(cams.shape)))
    F = cams.shape[0]
    if not np.all(np.isfinite(cams)):
        raise DepthConsError('cams: frame %d has a value that is not finite' % int(np.argmax(~np.isfinite(cams).all(1))))
    bad = ~(cams[:, :2] > 0).all(1)
    if bad.any():
        raise DepthConsError('cams: frame %d has focal lengths fx = %g, fy = %g: the intrinsics must be positive'
                             % (int(np.argmax(bad)), cams[int(np.argmax(bad)), 0], cams[int(np.argmax(bad)), 1]))
    R = cams[:, 4:].reshape(F, 3, 4)[:, :, :3]
    err = np.abs(np.einsum('fki,fkj->fij', R, R) - np.eye(3)).reshape(F, -1).max(1)
    if (err > ORTHO_TOL).any():
        raise DepthConsError('cams: the rotation of frame %d is not orthonormal (|R^T R - I| = %.3g > %g): the check inverts it by '
                             'transposition' % (int(np.argmax(err > ORTHO_TOL)), float(err.max()), ORTHO_TOL))
    nbr = np.asarray(nbr)
    if nbr.dtype.kind not in 'iu':
        raise DepthConsError('nbr: expected an integer array, got %s' % nbr.dtype)
    if nbr.ndim != 2 or nbr.shape[0] != F:
        raise DepthConsError('nbr: expected [%d, K], got %s' % (F, tuple(nbr.shape)))
    if nbr.shape[1] > MAX_VIEWS:
        raise DepthConsError('nbr: %d neighbours per frame, at most %d' % (nbr.shape[1], MAX_VIEWS))
    nbr = np.ascontiguousarray(nbr, np.int32)
    for i in range(F):
        row = nbr[i][nbr[i] >= 0]
        if (row >= F).any():
            raise DepthConsError('nbr: frame %d lists frame %d, but there are %d frames' % (i, int(row.max()), F))
        if (row == i).any():
            raise DepthConsError('nbr: frame %d lists itself as a neighbour' % i)
        if len(set(row.tolist())) != len(row):
            raise DepthConsError('nbr: frame %d lists a neighbour twice (%s)' % (i, row.tolist()))
    return cams, nbr


def check_params(min_views=2, pix_tol=1.0, rel_tol=0.01, keep_unverified=True, std_floor=0.0):
    """The five parameters as the call takes them; std_floor in the units of the depth"""
    p = dict(min_views=int(min_views), pix_tol=float(pix_tol), rel_tol=float(rel_tol), keep_unverified=bool(keep_unverified),
             std_floor=float(std_floor))
    if p['min_views'] < 1:
        raise DepthConsError('min_views = %d: at least 1' % p['min_views'])
    for key in ('pix_tol', 'rel_tol', 'std_floor'):
        if not (np.isfinite(p[key]) and p[key] >= 0):
            raise DepthConsError('%s = %r: expected a finite number >= 0' % (key, p[key]))
    return p


# ---------------------------------------------------------------------------------------------------- the call
NO_CPU = '%s: expected a CUDA/HIP float32 tensor (the consistency check has no CPU path)'


def _frames(t, name):
    """t checked as a contiguous float32 [F, H, W] tensor.  These few lines are the binding's own: where t lives is asked last
    (_outputs_ok), so that a host without a device gets every other answer, and one frame is not granted a batch axis."""
    import torch
    if not isinstance(t, torch.Tensor):
        raise DepthConsError(NO_CPU % name)
    if t.dtype != torch.float32:
        raise DepthConsError('%s: expected torch.float32, got %s' % (name, t.dtype))
    if t.dim() != 3:
        raise DepthConsError('%s: expected [F, H, W], got %s' % (name, tuple(t.shape)))
    return U.contiguous(t, name, DepthConsError)


_overlaps = IO.overlaps


def _outputs_ok(depth, depth_out):
    """depth (and depth_out, when given) checked: dtype, shape, contiguity, aliasing, then the device"""
    depth = _frames(depth, 'depth')
    if depth_out is not None:
        depth_out = _frames(depth_out, 'depth_out')
        if depth_out.shape != depth.shape or depth_out.device != depth.device:
            raise DepthConsError('depth_out %s on %s: expected the shape %s and device %s of depth'
                                 % (tuple(depth_out.shape), depth_out.device, tuple(depth.shape), depth.device))
        if _overlaps(depth_out, depth):
            raise DepthConsError('depth_out overlaps depth: the neighbours of a pixel read depth, so the check cannot run in place')
    if not depth.is_cuda:
        raise DepthConsError(NO_CPU % 'depth')
    return depth, depth_out


def upload(cams, nbr, device):
    """(cams float64 [F, 16], nbr int32 [F, K] or None for K = 0, K) on the device, after validate()"""
    return _upload(*validate(cams, nbr), device)


def _upload(cams_h, nbr_h, device):
    import torch
    return torch.from_numpy(cams_h).to(device), torch.from_numpy(nbr_h).to(device) if nbr_h.shape[1] > 0 else None, int(nbr_h.shape[1])


def enqueue(depth, cams_d, nbr_d, n_views, prm, std=True, counts=False, rows=True, depth_out=None, out=None):
    """The library call alone, on cameras and neighbour lists that upload() put on the device: Pending.  prm: check_params().  out:
    the `.tensors` of an earlier call of the same shape and outputs, to write into again instead of allocating.  `.tensors`:
    'depth' (float32 [F, H, W]) and, when asked, 'std' (float32 [F, H, W]), 'counts' (uint8 [F, H, W, 2] = (n_seen, n_ok)) and
    'rows' (int64 [F, 4] in ROW_NAMES' order); `.get()`: the same as numpy arrays."""
    import torch
    depth, depth_out = _outputs_ok(depth, depth_out)
    F, H, W = (int(v) for v in depth.shape)
    if tuple(cams_d.shape) != (F, CAM):
        raise DepthConsError('cams: %d cameras for %d frames of depth' % (cams_d.shape[0], F))
    dev = depth.device
    with torch.cuda.device(dev):
        ws = _workspaces.buffer(dev, F, H, W) if rows else None
        if out is None:
            out = {'depth': depth_out if depth_out is not None else torch.empty_like(depth)}
            if std:
                out['std'] = torch.empty((F, H, W), dtype=torch.float32, device=dev)
            if counts:
                out['counts'] = torch.empty((F, H, W, 2), dtype=torch.uint8, device=dev)
            if rows:
                out['rows'] = torch.empty((F, len(ROW_NAMES)), dtype=torch.int64, device=dev)
        check(lib().depthcons_check(U.stream(), F, H, W, n_views, U.p(depth), U.p(cams_d), U.p(nbr_d), prm['pix_tol'],
                                    prm['rel_tol'], prm['min_views'], int(prm['keep_unverified']), prm['std_floor'], U.p(ws),
                                    U.p(out['depth']), U.p(out.get('std')), U.p(out.get('counts')), U.p(out.get('rows'))),
              'depthcons_check')
    return U.Pending(out, (depth, cams_d, nbr_d, ws))


def check_async(depth, cams, nbr, min_views=2, pix_tol=1.0, rel_tol=0.01, keep_unverified=True, std_floor=0.0, std=True,
                counts=False, rows=True, depth_out=None):
    """Pending of the check of the float32 device tensor depth [F, H, W] (z-depth, valid iff > 0) with the host arrays cams
    float64 [F, 16] (pack_cams) and nbr int [F, K] (neighbours); std_floor in the units of depth.  depth_out: a float32 device
    tensor of depth's shape to write the filtered prior to (it must not overlap depth).  Everything is checked on the host
    first; then two small uploads and the library call.  Enqueue only."""
    depth, depth_out = _outputs_ok(depth, depth_out)
    prm = check_params(min_views, pix_tol, rel_tol, keep_unverified, std_floor)
    cams_h, nbr_h = validate(cams, nbr)
    if cams_h.shape[0] != depth.shape[0]:
        raise DepthConsError('cams: %d cameras for %d frames of depth' % (cams_h.shape[0], depth.shape[0]))
    cams_d, nbr_d, n_views = _upload(cams_h, nbr_h, depth.device)
    return enqueue(depth, cams_d, nbr_d, n_views, prm, std, counts, rows, depth_out)


def filter_priors(depth, cams, views=4, nbr=None, **params):
    """(filtered prior float32 [F, H, W], standard deviation float32 [F, H, W], rows int64 [F, 4]) on depth's device: the check of
    depth against each frame's `views` nearest frames (or the lists nbr).  params: the five of check_async.  Enqueue only."""
    cams = np.asarray(cams, np.float64)
    if nbr is None:
        nbr = neighbours(cams.reshape(len(cams), -1)[:, [7, 11, 15]], check_views(views, 'views'))
    t = check_async(depth, cams, nbr, std=True, counts=False, rows=True, **params).tensors
    return t['depth'], t['std'], t['rows']


def totals_line(rows, views):
    """The one log line of a load-time check; rows: int64 [F, 4] (host)"""
    rows = np.asarray(rows, np.int64)
    tot = rows.sum(0)
    emptied = int(((rows[:, 0] > 0) & (rows[:, 2] == 0)).sum())
    return ('depth consistency check (%d views): %d frames, %d valid prior pixels, %d verifiable, %d kept, %d dropped%s'
            % (views, len(rows), tot[0], tot[1], tot[2], tot[3],
               '' if emptied == 0 else ' -- %d frames are left without a prior pixel: is the prior metric in the scene\'s frame?' % emptied))


# -------------------------------------------------------------------------------------------------------- adapters
def cams_from_samplers(samplers):
    """cams float64 [F, 16] of NeRF++ ray samplers: intrinsics[:3, :3] and c2w_mat (OpenCV axes already)"""
    return pack_cams(np.stack([np.asarray(s.intrinsics, np.float64)[:3, :3] for s in samplers], 0),
                     np.stack([np.asarray(s.c2w_mat, np.float64) for s in samplers], 0), 'ray samplers')


def cams_from_scene(scene, idx=None):
    """cams float64 [len(idx), 16] of a MipNeRF-360 Scene: K from the inverse of pixtocam, poses @ diag(1, -1, -1) back to OpenCV
    axes.  A scene with lens distortion is a ConfigError: the check is pinhole-only."""
    from .mip360_data import ConfigError, camera_model_name
    if scene.distortion is not None:
        raise ConfigError('the depth consistency check is pinhole-only (SIMPLE_PINHOLE, PINHOLE), but the scene\'s camera is %s: '
                          'undistort the frames first' % camera_model_name(scene.sparse_dir))
    poses = np.asarray(scene.poses, np.float64)
    if idx is not None:
        poses = poses[np.asarray(idx)]
    c2w = poses.copy()
    c2w[:, :3, :3] = poses[:, :3, :3] * np.array([1., -1., -1.])                  # columns: right, up, back -> right, down, forward
    return pack_cams(np.linalg.inv(np.asarray(scene.pixtocam, np.float64)), c2w, 'scene')


def scene_params(cfg, scale):
    """The call's parameters of a Config dict; Config.depth_cons_std_floor is in metres, the call's in scene units"""
    return dict(min_views=int(cfg.get('depth_cons_min_views', 2)), pix_tol=float(cfg.get('depth_cons_pix_tol', 1.0)),
                rel_tol=float(cfg.get('depth_cons_rel_tol', 0.01)), keep_unverified=bool(cfg.get('depth_cons_keep_unverified', True)),
                std_floor=float(cfg.get('depth_cons_std_floor', 0.0)) * float(scale))


def check_views(views, what):
    views = int(views)
    if not 0 <= views <= MAX_VIEWS:
        raise DepthConsError('%s = %d: expected 0 (off) .. %d' % (what, views, MAX_VIEWS))
    return views


def add_flags(parser, prefix='depth_cons_'):
    """--depth_cons_views and the five parameters on an argparse parser (ddp_train_nerf); the CLI adds the five without prefix"""
    if prefix:
        parser.add_argument('--%sviews' % prefix, type=int, default=0, help=VIEWS_HELP)
    for name, (default, text) in PARAMS.items():
        parser.add_argument('--%s%s' % (prefix, name), type=type(default) if not isinstance(default, bool) else int,
                            default=default if not isinstance(default, bool) else int(default), help='%s (default %s)' % (text, default))


def args_params(args, scale, prefix='depth_cons_'):
    """The call's parameters of parsed flags; --*std_floor is in metres, the call's in scene units"""
    g = lambda name: getattr(args, prefix + name)
    return dict(min_views=g('min_views'), pix_tol=g('pix_tol'), rel_tol=g('rel_tol'), keep_unverified=bool(g('keep_unverified')),
                std_floor=float(g('std_floor')) * float(scale))


def filter_samplers(samplers, device, views, want_std=False, **params):
    """The load-time check of the NeRF++ path: the priors of the ray samplers (one frame each, all of one size) are checked together
    and written back (IO.write_back; with want_std the spread too).  Returns the rows int64 [F, 4] (host).  Every rank computes the
    same bits; nothing is communicated."""
    import torch
    views = check_views(views, '--depth_cons_views')
    depth = torch.from_numpy(IO.stack_priors(samplers, '--depth_cons_views', 'check', 'check', DepthConsError)).to(device)
    out, std, rows = filter_priors(depth, cams_from_samplers(samplers), views, **params)
    IO.write_back(samplers, out.cpu().numpy(), std.cpu().numpy() if want_std else None)
    return rows.cpu().numpy()


# ------------------------------------------------------------------------------------------------------ PNG encoding
def encode_prior(raw, dropped):
    """uint16 PNG values of the filtered prior: the input's own 16-bit value where it is not dropped, 0 where it is"""
    raw = np.asarray(raw)
    return np.where(np.asarray(dropped, bool), 0, raw).astype(np.uint16)


# the standard deviation's PNG: IO.encode_metres of the metres where the prior is kept
encode_std, _write_png16, absrel = IO.encode_metres, IO.write_png16, IO.absrel


def write_report(path, names, rows, prior=None, gt=None, valid=None, kept=None):
    """consistency_T.txt: per frame and in total the four counts and, where ground-truth depth exists, AbsRel of the raw prior
    over the kept and over the dropped pixels"""
    if gt is None:
        return IO.write_rows_report(path, names, rows, ' '.join(ROW_NAMES))
    IO.write_rows_report(path, names, rows, ' '.join(ROW_NAMES) + ' absrel_kept absrel_dropped', lambda sel, r, n: ' %.6f %.6f' % (
        absrel(prior[sel], gt[sel], valid[sel] & kept[sel]), absrel(prior[sel], gt[sel], valid[sel] & ~kept[sel])))


# --------------------------------------------------------------------------------------------------------------- CLI
def run_colmap(args, device):
    """The COLMAP layout: all frames of the scene together -> depths{sfx}_{T}_cons/, depths{sfx}_{T}_cons_std/, consistency_T.txt"""
    import torch
    from PIL import Image
    from . import mip360_data as D
    T = args.depth_sup_type
    cfg = D.parse_gin(args.gin_configs, list(args.gin_bindings) + ['Config.data_dir = %r' % args.data_dir,
                                                                   'Config.depth_sup_type = %r' % T, "Config.depth_loss_type = 'mse'"])
    cfg['depth_cons_views'] = 0
    scene = D.Scene(cfg)
    cams = cams_from_scene(scene)
    depth = torch.from_numpy(scene.depths_sup).to(device)
    out, std, rows = filter_priors(depth, cams, check_views(args.views, '--views'), **args_params(args, scene.scale, ''))
    out, std, rows = out.cpu().numpy(), std.cpu().numpy(), rows.cpu().numpy()
    valid = scene.depths_sup > 0
    kept = valid & (out > 0)
    sup_dir = os.path.join(args.data_dir, 'depths%s_%s' % (IO.colmap_suffix(cfg), T))
    to_sup = dict(zip(D._listdir(os.path.join(args.data_dir, 'images')), D._listdir(sup_dir)))
    out_dir, std_dir = sup_dir + '_cons', sup_dir + '_cons_std'
    for d in (out_dir, std_dir):
        os.makedirs(d, exist_ok=True)
    for i, name in enumerate(scene.names):
        raw = np.asarray(Image.open(os.path.join(sup_dir, to_sup[name])))
        _write_png16(os.path.join(out_dir, to_sup[name]), encode_prior(raw, valid[i] & ~kept[i]))
        _write_png16(os.path.join(std_dir, to_sup[name]), encode_std(std[i] / scene.scale, kept[i]))
    report = os.path.join(args.data_dir, 'consistency_%s.txt' % T)
    write_report(report, scene.names, rows, scene.depths_sup, scene.depths_gt, valid, kept)
    print(totals_line(rows, args.views), flush=True)
    print('wrote %s, %s and %s' % (out_dir, std_dir, report), flush=True)
    return rows


def run_nerfpp(args, device):
    """The NeRF++ layout, each of train / test by itself -> {split}/depth_{T}_cons/, {split}/depth_{T}_cons_std/,
    {split}/consistency_T.txt"""
    import torch
    from .data_loader_split import _imread
    T = args.depth_sup_type
    done = {}
    for split, split_dir, files, samplers in IO.nerfpp_splits(args, 'depth' + ('_' + T if T != 'gt' else ''), ['*.png', '*.jpg'],
                                                               depth_sup_type=T):
        if any(s.depth_sup is None for s in samplers):
            raise DepthConsError('%s: the prior needs ground-truth depth/ and the scene\'s scale file to be read in scene units' % split_dir)
        scale = float(samplers[0].depth_scale)
        prior = IO.stack_frames(samplers, 'depth_sup', '%s: the frames differ in size; the check takes frames of one size' % split_dir,
                                DepthConsError)
        out, std, rows = filter_priors(torch.from_numpy(prior).to(device), cams_from_samplers(samplers),
                                       check_views(args.views, '--views'), **args_params(args, scale, ''))
        out, std, rows = out.cpu().numpy(), std.cpu().numpy(), rows.cpu().numpy()
        valid = prior > 0
        kept = valid & (out > 0)
        out_dir, std_dir = os.path.join(split_dir, 'depth_%s_cons' % T), os.path.join(split_dir, 'depth_%s_cons_std' % T)
        for d in (out_dir, std_dir):
            os.makedirs(d, exist_ok=True)
        names = IO.png_names(files)
        for i, p in enumerate(files):
            _write_png16(os.path.join(out_dir, names[i]), encode_prior(_imread(p), valid[i] & ~kept[i]))
            _write_png16(os.path.join(std_dir, names[i]), encode_std(std[i] / scale, kept[i]))
        report = os.path.join(split_dir, 'consistency_%s.txt' % T)
        write_report(report, names, rows, prior, IO.stack_gt(samplers), valid, kept)
        print('%s: %s' % (split, totals_line(rows, args.views)), flush=True)
        print('wrote %s, %s and %s' % (out_dir, std_dir, report), flush=True)
        done[split] = rows
    if not done:
        raise DepthConsError('no prior of type %r under %s' % (T, os.path.join(args.datadir, args.scene)))
    return done


def make_parser():
    p = IO.base_parser('python -m outdoor_nerf_depth_amd.depth_consistency', __doc__, verb='checked')
    p.add_argument('--depth_sup_type', required=True, help='the prior to check: T of depths_T/ or {split}/depth_T/; the result is found '
                   'under --depth_sup_type T_cons')
    p.add_argument('--views', type=int, default=4, help='nearest frames every frame is checked against (1 .. %d; default 4)' % MAX_VIEWS)
    add_flags(p, '')
    IO.add_device_flag(p)
    return p


def main(argv=None):
    import torch
    args = make_parser().parse_args(argv)
    run = {'colmap': run_colmap, 'nerfpp': run_nerfpp}[IO.pick_layout(args)]
    if args.views < 1:
        raise SystemExit('--views = %d: at least 1' % args.views)
    return run(args, torch.device(args.device))


if __name__ == '__main__':
    main()

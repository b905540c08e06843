"""Completing sparse depth priors by image-guided filtering on the device: the classical, weight-free stand-in for the paper's
depth-completion prior.  ctypes binding of libdepthcomp_hip.so (include/depthcomp_hip.h), the adapters of both front ends, and the CLI

    python -m outdoor_nerf_depth_amd.depth_complete --data_dir SCENE --depth_sup_type T [--gin_bindings ...]      (COLMAP layout)
    python -m outdoor_nerf_depth_amd.depth_complete --datadir DIR --scene SCENE --depth_sup_type T                (NeRF++ layout)

Joint-bilateral normalised convolution, guided by each frame's own colour image: a pixel without a measurement takes the
confidence-weighted mean of the measured depths within `radius` pixels, each weighted by a Gaussian of its distance in the image
(`sigma_space`) and of its colour difference |dR| + |dG| + |dB| (`sigma_colour`), so that the fill stops at object boundaries.  A
window whose depths spread by more than `max_rel_spread` of their mean straddles two surfaces and is refused.  `iters` passes carry
the fill outwards, each with `decay` times the confidence of what it read.  The frame's own pixels are never changed.  The
definition is DESIGN.md 8.10 (restated as code in tests/depth_complete_reference.py).

Out of scope: learned completion, extrapolation beyond iters * radius pixels from a measurement (the sky stays empty), and a guide
other than the frame's own image.

The CLI writes, next to the prior, the folders the loaders already find under `--depth_sup_type T_comp` (the prior and its `_std`
twin for the 'gnll' loss), plus complete_T.txt with the counts.  The load-time flags (Config.depth_comp_iters, --depth_comp_iters)
run the same call when a training run loads its frames instead, after alignment, accumulation and the consistency check; they use
the float32 value, which the CLI's folders round to the PNG's 1 / 256 m.  For COLMAP scenes the CLI takes all frames together while
the flag takes the training split.

Everything is enqueued on torch's current stream and nothing synchronises until the numbers are read.  torch only allocates.
There is no host path: without libdepthcomp_hip.so and a device every call raises.
"""
import ctypes as C
import os

import numpy as np

from . import _ctypes_util as U
from . import depth_prior_io as IO
from .depth_prior_io import overlaps as _overlaps, write_png16 as _write_png16, absrel, encode_metres as encode_std   # noqa: F401

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get('DEPTHCOMP_HIP_LIB') or os.path.join(_HERE, 'libdepthcomp_hip.so')
ABI_VERSION = 1
MAX_FRAMES = 65535
MAX_RADIUS, MAX_ITERS, MAX_POINTS, N_COLOUR = 8, 16, 289, 766
ROW_NAMES = ('n_own', 'n_filled', 'n_refused', 'n_none')
ORIGIN_NONE, ORIGIN_OWN, ORIGIN_FILLED, ORIGIN_REFUSED = 0, 1, 2, 3
# the parameters: name -> (default, help).  The defaults are those of the numpy prototype on the analytic box scene.
PARAMS = {
    'radius': (4, 'half width, in pixels, of the window a pixel is filled from (1 .. %d)' % MAX_RADIUS),
    'sigma_space': (2.0, 'standard deviation, in pixels, of the Gaussian weight of a tap\'s distance in the image'),
    'sigma_colour': (20.0, 'standard deviation, in 8-bit levels of |dR| + |dG| + |dB|, of the Gaussian weight of a tap\'s colour difference'),
    'min_conf': (0.02, 'a pixel is filled only where the confidence-weighted share of its window that carries depth reaches this (0 .. 1)'),
    'min_points': (2, 'a pixel is filled only from at least this many taps that carry depth (1 .. %d)' % MAX_POINTS),
    'max_rel_spread': (0.1, 'a window whose depths spread (weighted standard deviation) by more than this, relative to their mean, '
                            'straddles two surfaces and fills nothing (inf = no gate)'),
    'decay': (0.5, 'a filled pixel carries this times the confidence of its window into the next pass (0 < decay <= 1)'),
}
STD_FLOOR_HELP = 'lower bound, in metres, of the standard deviation the completion writes for the gnll depth loss'
ITERS_HELP = ('complete each training frame\'s depth prior on the device when the frames are loaded, guided by the frame\'s own image: N '
              'passes of joint-bilateral normalised convolution, after alignment, accumulation and the consistency check (0 = off; '
              '1 .. %d)' % MAX_ITERS)

_fp = C.c_void_p
# every symbol include/depthcomp_hip.h declares: name -> (restype, argtypes)
SYMBOLS = {
    'depthcomp_last_error': (C.c_char_p, []),
    'depthcomp_abi_version': (C.c_int, []),
    'depthcomp_workspace_bytes': (C.c_int64, [C.c_int, C.c_int, C.c_int]),
    'depthcomp_complete': (C.c_int, [_fp, C.c_int, C.c_int, C.c_int, _fp, _fp, _fp, _fp, _fp, C.c_int, C.c_int, C.c_int, C.c_double,
                                     C.c_double, C.c_double, _fp, _fp, _fp, _fp, _fp, _fp, _fp]),
}

_lib = None


class DepthCompError(RuntimeError):
    pass


def lib():
    """The loaded library with typed prototypes.  Raises if it has not been built."""
    global _lib
    if _lib is None:
        _lib = U.load(LIB_PATH, 'libdepthcomp_hip.so', SYMBOLS, 'depthcomp_abi_version', ABI_VERSION, DepthCompError,
                      ' (hipcc --offload-arch=gfx950). There is no CPU fallback for the completion of depth priors.')
    return _lib


def last_error():
    return lib().depthcomp_last_error().decode('utf-8', 'replace')


check = U.checker(lib, 'depthcomp_last_error', DepthCompError, 'depthcomp call')


def workspace_bytes(n_frames, height, width):
    """Size of the scratch buffer of a call on n_frames frames of height x width pixels; raises DepthCompError for sizes the library
    rejects (n_frames outside 1 .. 65535, height * width outside 1 .. 2^28).  Needs no GPU."""
    return U.size(lib().depthcomp_workspace_bytes(int(n_frames), int(height), int(width)), last_error, DepthCompError)


_workspaces = U.Workspaces(workspace_bytes, 2, 'float64')


def check_iters(iters, what='iters'):
    if isinstance(iters, bool) or int(iters) != iters or not 1 <= int(iters) <= MAX_ITERS:
        raise DepthCompError('%s = %r: expected an integer 1 .. %d' % (what, iters, MAX_ITERS))
    return int(iters)


def check_params(radius=4, sigma_space=2.0, sigma_colour=20.0, iters=3, min_conf=0.02, min_points=2, max_rel_spread=0.1, decay=0.5,
                 std_floor=0.0):
    """The parameters as the call takes them"""
    p = dict(radius=int(radius), sigma_space=float(sigma_space), sigma_colour=float(sigma_colour), iters=check_iters(iters),
             min_conf=float(min_conf), min_points=int(min_points), max_rel_spread=float(max_rel_spread), decay=float(decay),
             std_floor=float(std_floor))
    if not 1 <= p['radius'] <= MAX_RADIUS or p['radius'] != radius:
        raise DepthCompError('radius = %r: expected an integer 1 .. %d' % (radius, MAX_RADIUS))
    for name in ('sigma_space', 'sigma_colour'):
        if not (np.isfinite(p[name]) and p[name] > 0):
            raise DepthCompError('%s = %r: expected a finite number > 0' % (name, p[name]))
    if not 0 <= p['min_conf'] <= 1:
        raise DepthCompError('min_conf = %r: expected a number in [0, 1]' % p['min_conf'])
    if not 1 <= p['min_points'] <= MAX_POINTS or p['min_points'] != min_points:
        raise DepthCompError('min_points = %r: expected an integer 1 .. %d' % (min_points, MAX_POINTS))
    if not p['max_rel_spread'] >= 0:
        raise DepthCompError('max_rel_spread = %r: expected a number >= 0 (inf = no gate)' % p['max_rel_spread'])
    if not 0 < p['decay'] <= 1:
        raise DepthCompError('decay = %r: expected a number in (0, 1]' % p['decay'])
    if not (np.isfinite(p['std_floor']) and p['std_floor'] >= 0):
        raise DepthCompError('std_floor = %r: expected a finite number >= 0' % p['std_floor'])
    return p


def tables(radius, sigma_space, sigma_colour):
    """(w_space float64 [(2 r + 1)^2] row-major over (dy, dx), w_colour float64 [766] indexed by |dR| + |dG| + |dB|): the two
    Gaussians, evaluated with numpy on the host so that no exp on the device has to agree with it"""
    d = np.arange(-radius, radius + 1, dtype=np.float64)
    w_space = np.exp(-(d[:, None] * d[:, None] + d[None, :] * d[None, :]) / (2.0 * sigma_space * sigma_space)).reshape(-1)
    s = np.arange(N_COLOUR, dtype=np.float64)
    return w_space, np.exp(-(s * s) / (2.0 * sigma_colour * sigma_colour))


def check_tables(w_space, w_colour, radius):
    """The caller's tables as contiguous float64 host arrays: the sizes of `radius`, every entry finite and >= 0"""
    out = []
    for name, t, n in (('w_space', w_space, (2 * radius + 1) ** 2), ('w_colour', w_colour, N_COLOUR)):
        t = np.ascontiguousarray(np.asarray(t, np.float64).reshape(-1))
        if t.size != n:
            raise DepthCompError('%s: %d entries, expected %d%s' % (name, t.size, n, ' ((2 * radius + 1)^2)' if name == 'w_space' else ''))
        if not (np.isfinite(t).all() and (t >= 0).all()):
            raise DepthCompError('%s: every entry must be finite and >= 0' % name)
        out.append(t)
    return out


# ---------------------------------------------------------------------------------------------------- the call
NO_CPU = '%s: expected a CUDA/HIP %s tensor (the completion of depth priors has no CPU path)'


def _frames(t, name, dtype='float32', trailing=()):
    """t checked as a contiguous [F, H, W] (+ trailing) tensor of dtype; where it lives is asked last (_tensors_ok)"""
    import torch
    if not isinstance(t, torch.Tensor):
        raise DepthCompError(NO_CPU % (name, dtype))
    if t.dtype != getattr(torch, dtype):
        raise DepthCompError('%s: expected torch.%s, got %s' % (name, dtype, t.dtype))
    if t.dim() != 3 + len(trailing) or tuple(t.shape[3:]) != tuple(trailing):
        raise DepthCompError('%s: expected [F, H, W%s], got %s' % (name, ''.join(', %d' % n for n in trailing), tuple(t.shape)))
    return U.contiguous(t, name, DepthCompError)


def _tensors_ok(depth, rgb, std_in, depth_out):
    """The tensors of a call checked: dtype, shape, contiguity, aliasing, then the device"""
    depth = _frames(depth, 'depth')
    rgb = _frames(rgb, 'rgb', 'uint8', (3,))
    if tuple(rgb.shape[:3]) != tuple(depth.shape):
        raise DepthCompError('rgb %s: expected the frames %s of depth' % (tuple(rgb.shape), tuple(depth.shape)))
    others = [('rgb', rgb)]
    if std_in is not None:
        std_in = _frames(std_in, 'std_in')
        others.append(('std_in', std_in))
    if depth_out is not None:
        depth_out = _frames(depth_out, 'depth_out')
        others.append(('depth_out', depth_out))
    for name, t in others[1:]:
        if t.shape != depth.shape:
            raise DepthCompError('%s %s: expected the shape %s of depth' % (name, tuple(t.shape), tuple(depth.shape)))
    for name, t in others:
        if t.device != depth.device:
            raise DepthCompError('%s on %s: expected the device %s of depth' % (name, t.device, depth.device))
    if depth_out is not None:
        for name, t in (('depth', depth), ('rgb', rgb), ('std_in', std_in)):
            if t is not None and _overlaps(depth_out, t):
                raise DepthCompError('depth_out overlaps %s: a pass reads the window of a pixel, so the call cannot run in place' % name)
    if not depth.is_cuda:
        raise DepthCompError(NO_CPU % ('depth', 'float32'))
    return depth, rgb, std_in, depth_out


def enqueue(depth, rgb, std_in, w_space_d, w_colour_d, prm, conf=True, passes=True, rows=True, depth_out=None, out=None):
    """The library call alone, on weight tables that are on the device already (float64, check_tables' sizes): Pending.  prm:
    check_params().  out: the `.tensors` of an earlier call of the same shape and outputs, to write into again instead of
    allocating.  `.tensors`: 'depth', 'std' (float32 [F, H, W]), 'origin' (uint8: 0 none, 1 own, 2 filled, 3 refused) and, when
    asked, 'conf' (float32), 'pass' (uint8) and 'rows' (int64 [F, 4] in ROW_NAMES' order); `.get()`: the same as numpy arrays."""
    import torch
    depth, rgb, std_in, depth_out = _tensors_ok(depth, rgb, std_in, depth_out)
    F, H, W = (int(v) for v in depth.shape)
    side = 2 * prm['radius'] + 1
    for name, t, n in (('w_space', w_space_d, side * side), ('w_colour', w_colour_d, N_COLOUR)):
        if not (isinstance(t, torch.Tensor) and t.dtype == torch.float64 and t.numel() == n and t.is_contiguous() and t.device == depth.device):
            raise DepthCompError('%s: expected a contiguous float64 tensor of %d entries on %s' % (name, n, depth.device))
    dev = depth.device
    with torch.cuda.device(dev):
        ws = _workspaces.buffer(dev, F, H, W)
        if out is None:
            out = {'depth': depth_out if depth_out is not None else torch.empty_like(depth), 'std': torch.empty_like(depth),
                   'origin': torch.empty((F, H, W), dtype=torch.uint8, device=dev)}
            if conf:
                out['conf'] = torch.empty_like(depth)
            if passes:
                out['pass'] = torch.empty((F, H, W), dtype=torch.uint8, device=dev)
            if rows:
                out['rows'] = torch.empty((F, len(ROW_NAMES)), dtype=torch.int64, device=dev)
        check(lib().depthcomp_complete(U.stream(), F, H, W, U.p(depth), U.p(rgb), U.p(std_in), U.p(w_space_d), U.p(w_colour_d),
                                       prm['radius'], prm['iters'], prm['min_points'], prm['min_conf'], prm['max_rel_spread'],
                                       prm['decay'], U.p(ws), U.p(out['depth']), U.p(out['std']), U.p(out.get('conf')),
                                       U.p(out['origin']), U.p(out.get('pass')), U.p(out.get('rows'))), 'depthcomp_complete')
    return U.Pending(out, (depth, rgb, std_in, w_space_d, w_colour_d, ws))


def complete_async(depth, rgb, std_in=None, w_space=None, w_colour=None, conf=True, passes=True, rows=True, depth_out=None, **params):
    """Pending of the completion of the float32 device tensor depth [F, H, W] (z-depth, valid iff > 0) guided by the uint8 device
    tensor rgb [F, H, W, 3]; std_in: the float32 standard deviation of depth's own measurements, or None.  w_space, w_colour: host
    tables to use instead of the Gaussians of sigma_space and sigma_colour (check_tables).  depth_out: a float32 device tensor of
    depth's shape to write the completed prior to (it must not overlap an input).  params: those of check_params.  Everything is
    checked on the host first; then two small uploads and the library call.  Enqueue only."""
    import torch
    depth, rgb, std_in, depth_out = _tensors_ok(depth, rgb, std_in, depth_out)
    prm = check_params(**params)
    g_space, g_colour = tables(prm['radius'], prm['sigma_space'], prm['sigma_colour'])
    ws_h, wc_h = check_tables(g_space if w_space is None else w_space, g_colour if w_colour is None else w_colour, prm['radius'])
    return enqueue(depth, rgb, std_in, torch.from_numpy(ws_h).to(depth.device), torch.from_numpy(wc_h).to(depth.device), prm, conf,
                   passes, rows, depth_out)


def complete_priors(depth, rgb, std_in=None, **params):
    """(completed prior float32 [F, H, W], its standard deviation float32 [F, H, W] floored at std_floor where the prior is valid,
    origin uint8 [F, H, W], rows int64 [F, 4]) on depth's device.  params: those of check_params.  Enqueue only."""
    floor = check_params(**params)['std_floor']
    t = complete_async(depth, rgb, std_in, conf=False, passes=False, rows=True, **params).tensors
    std = t['std']
    if floor > 0:
        std = std.clamp_min(floor) * (t['origin'] == ORIGIN_OWN).logical_or_(t['origin'] == ORIGIN_FILLED)
    return t['depth'], std, t['origin'], t['rows']


def totals_line(rows, iters):
    """The one log line of a load-time completion; rows: int64 [F, 4] (host)"""
    rows = np.asarray(rows, np.int64)
    tot = rows.sum(0)
    px = max(int(tot.sum()), 1)
    return ('depth completion (%d passes): %d frames, %d own prior pixels, %d filled, %d refused, %d left empty (coverage %.1f %% -> %.1f %%)'
            % (iters, len(rows), tot[0], tot[1], tot[2], tot[3], 100.0 * tot[0] / px, 100.0 * (tot[0] + tot[1]) / px))


# -------------------------------------------------------------------------------------------------------- adapters
def scene_params(cfg, scale=1.0):
    """The call's parameters of a Config dict (std_floor: metres -> scene units)"""
    p = {name: cfg.get('depth_comp_' + name, default) for name, (default, _) in PARAMS.items()}
    p['iters'] = cfg.get('depth_comp_iters', 3)
    p['std_floor'] = float(cfg.get('depth_comp_std_floor', 0.0)) * float(scale)
    return p


def add_flags(parser, prefix='depth_comp_'):
    """--depth_comp_iters, the parameters and --depth_comp_std_floor on an argparse parser (ddp_train_nerf); the CLI adds them
    without prefix, with its own --iters"""
    if prefix:
        parser.add_argument('--%siters' % prefix, type=int, default=0, help=ITERS_HELP)
    for name, (default, text) in PARAMS.items():
        parser.add_argument('--%s%s' % (prefix, name), type=type(default), default=default, help='%s (default %s)' % (text, default))
    parser.add_argument('--%sstd_floor' % prefix, type=float, default=0.0, help='%s (default 0)' % STD_FLOOR_HELP)


def args_params(args, scale=1.0, prefix='depth_comp_'):
    """The call's parameters of parsed flags (std_floor: metres -> scene units)"""
    p = {name: getattr(args, prefix + name) for name in PARAMS}
    p['iters'] = getattr(args, prefix + 'iters')
    p['std_floor'] = float(getattr(args, prefix + 'std_floor')) * float(scale)
    return p


def guide_u8(img):
    """A sampler's image (float32 in [0, 1], bytes / 255) back as its bytes"""
    return np.clip(np.rint(np.asarray(img, np.float64) * 255.0), 0, 255).astype(np.uint8)


def _stack(samplers, what):
    if any(s.depth_sup is None for s in samplers):
        raise DepthCompError('%s: the training frames carry no depth prior to complete' % what)
    if any(s.img is None for s in samplers):
        raise DepthCompError('%s: the training frames carry no image to guide the completion' % what)
    differ = '%s: the frames differ in size; the completion takes frames of one size' % what
    depth = IO.stack_frames(samplers, 'depth_sup', differ, DepthCompError)
    rgb = np.stack([guide_u8(s.img).reshape(s.H, s.W, 3) for s in samplers], 0)
    std = None
    if all(s.depth_std is not None for s in samplers):
        std = IO.stack_frames(samplers, 'depth_std', differ, DepthCompError)
    return depth, rgb, std


def complete_samplers(samplers, device, want_std=False, **params):
    """The load-time completion of the NeRF++ path: the priors of the ray samplers (one frame each, all of one size) are completed
    together, each guided by its own image, and written back (IO.write_back).  With want_std the standard deviation the samplers
    carry (a constant one is materialised) goes in as std_in and the completion's, floored at std_floor, replaces it.  Returns the
    rows int64 [F, 4] (host).  Every rank computes the same bits; nothing is communicated."""
    import torch
    depth, rgb, std = _stack(samplers, '--depth_comp_iters')
    T = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(device)
    out, std_out, _, rows = complete_priors(T(depth), T(rgb), T(std) if want_std else None, **params)
    IO.write_back(samplers, out.cpu().numpy(), std_out.cpu().numpy() if want_std else None, replace_std=True)
    return rows.cpu().numpy()


# ------------------------------------------------------------------------------------------------------ PNG encoding
def encode_prior(raw, metres, filled):
    """uint16 PNG values of the completed prior: the input's own 16-bit value where nothing is filled, rint(metres * 256) clamped to
    [2, 65535] (the loaders read raw values below 2 as invalid) where something is"""
    return np.where(np.asarray(filled, bool), IO.encode_metres(metres, filled), np.asarray(raw)).astype(np.uint16)


def write_report(path, names, rows, origin, out=None, gt=None):
    """complete_T.txt: per frame and in total the four counts, the coverage (valid pixels / pixels) before and after and, where
    ground-truth depth exists, AbsRel of the filled pixels against it"""
    have_gt = gt is not None
    px = int(np.prod(origin.shape[1:]))
    IO.write_rows_report(path, names, rows, '%s coverage_before coverage_after%s' % (' '.join(ROW_NAMES), ' absrel_filled' if have_gt else ''),
                         lambda sel, r, n: ' %.6f %.6f%s' % (r[0] / (px * n), (r[0] + r[1]) / (px * n), ' %.6f' % absrel(
                             out[sel], gt[sel], origin[sel] == ORIGIN_FILLED) if have_gt else ''))


# --------------------------------------------------------------------------------------------------------------- CLI
def _run(prior, rgb, device, params):
    """(out, std, origin, rows) on the host"""
    import torch
    out, std, origin, rows = complete_priors(torch.from_numpy(np.ascontiguousarray(prior)).to(device),
                                             torch.from_numpy(np.ascontiguousarray(rgb)).to(device), **params)
    return out.cpu().numpy(), std.cpu().numpy(), origin.cpu().numpy(), rows.cpu().numpy()


def run_colmap(args, device):
    """The COLMAP layout: all frames of the scene together -> depths{sfx}_{T}_comp/, depths{sfx}_{T}_comp_std/, complete_T.txt"""
    from PIL import Image
    from . import mip360_data as D
    T = args.depth_sup_type
    cfg = D.parse_gin(args.gin_configs, list(args.gin_bindings) + ['Config.data_dir = %r' % args.data_dir,
                                                                   'Config.depth_sup_type = %r' % T, "Config.depth_loss_type = 'mse'"])
    cfg['depth_cons_views'] = cfg['depth_acc_views'] = cfg['depth_comp_iters'] = 0
    scene = D.Scene(cfg)
    out, std, origin, rows = _run(scene.depths_sup, scene.images, device, args_params(args, scene.scale, ''))
    sup_dir = os.path.join(args.data_dir, 'depths%s_%s' % (IO.colmap_suffix(cfg), T))
    to_sup = dict(zip(D._listdir(os.path.join(args.data_dir, 'images')), D._listdir(sup_dir)))
    out_dir, std_dir = sup_dir + '_comp', sup_dir + '_comp_std'
    for d in (out_dir, std_dir):
        os.makedirs(d, exist_ok=True)
    for i, name in enumerate(scene.names):
        raw = np.asarray(Image.open(os.path.join(sup_dir, to_sup[name])))
        _write_png16(os.path.join(out_dir, to_sup[name]), encode_prior(raw, out[i].astype(np.float64) / scene.scale, origin[i] == ORIGIN_FILLED))
        _write_png16(os.path.join(std_dir, to_sup[name]), encode_std(std[i] / scene.scale, (origin[i] == ORIGIN_OWN) | (origin[i] == ORIGIN_FILLED)))
    report = os.path.join(args.data_dir, 'complete_%s.txt' % T)
    write_report(report, scene.names, rows, origin, out, scene.depths_gt)
    print(totals_line(rows, args.iters), flush=True)
    print('wrote %s, %s and %s' % (out_dir, std_dir, report), flush=True)
    return rows


def run_nerfpp(args, device):
    """The NeRF++ layout, each of train / test by itself -> {split}/depth_{T}_comp/, {split}/depth_{T}_comp_std/,
    {split}/complete_T.txt"""
    from .data_loader_split import _imread
    T = args.depth_sup_type
    done = {}
    for split, split_dir, files, samplers in IO.nerfpp_splits(args, 'depth' + ('_' + T if T != 'gt' else ''), ['*.png', '*.jpg'],
                                                               depth_sup_type=T):
        if any(s.depth_sup is None for s in samplers):
            raise DepthCompError('%s: the prior needs ground-truth depth/ and the scene\'s scale file to be read in scene units' % split_dir)
        scale = float(samplers[0].depth_scale)
        prior, rgb, _ = _stack(samplers, split_dir)
        out, std, origin, rows = _run(prior, rgb, device, args_params(args, scale, ''))
        out_dir, std_dir = os.path.join(split_dir, 'depth_%s_comp' % T), os.path.join(split_dir, 'depth_%s_comp_std' % T)
        for d in (out_dir, std_dir):
            os.makedirs(d, exist_ok=True)
        names = IO.png_names(files)
        for i, p in enumerate(files):
            _write_png16(os.path.join(out_dir, names[i]), encode_prior(_imread(p), out[i].astype(np.float64) / scale, origin[i] == ORIGIN_FILLED))
            _write_png16(os.path.join(std_dir, names[i]), encode_std(std[i] / scale, (origin[i] == ORIGIN_OWN) | (origin[i] == ORIGIN_FILLED)))
        report = os.path.join(split_dir, 'complete_%s.txt' % T)
        write_report(report, names, rows, origin, out, IO.stack_gt(samplers))
        print('%s: %s' % (split, totals_line(rows, args.iters)), flush=True)
        print('wrote %s, %s and %s' % (out_dir, std_dir, report), flush=True)
        done[split] = rows
    if not done:
        raise DepthCompError('no prior of type %r under %s' % (T, os.path.join(args.datadir, args.scene)))
    return done


def make_parser():
    p = IO.base_parser('python -m outdoor_nerf_depth_amd.depth_complete', __doc__)
    p.add_argument('--depth_sup_type', required=True, help='the prior to complete: T of depths_T/ or {split}/depth_T/; the result is found '
                   'under --depth_sup_type T_comp')
    p.add_argument('--iters', type=int, default=3, help='passes (1 .. %d; default 3)' % MAX_ITERS)
    add_flags(p, '')
    IO.add_device_flag(p)
    return p


def main(argv=None):
    import torch
    args = make_parser().parse_args(argv)
    run = {'colmap': run_colmap, 'nerfpp': run_nerfpp}[IO.pick_layout(args)]
    try:
        check_params(**args_params(args, 1.0, ''))
    except DepthCompError as e:
        raise SystemExit(str(e))
    return run(args, torch.device(args.device))


if __name__ == '__main__':
    main()

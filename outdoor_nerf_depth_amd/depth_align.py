"""Aligning relative depth priors to sparse metric depth on the device, before training.  ctypes binding of libdepthalign_hip.so
(include/depthalign_hip.h), the adapters of both front ends, and the CLI

    python -m outdoor_nerf_depth_amd.depth_align --data_dir SCENE --depth_sup_type T --anchor_sup_type A [--space disparity]   (COLMAP layout)
    python -m outdoor_nerf_depth_amd.depth_align --datadir DIR --scene SCENE --depth_sup_type T --anchor_sup_type A           (NeRF++ layout)

A monocular depth prior is known up to one scale and one shift per image.  Each frame's (s, b) is fitted once, robustly (reweighted
least squares with Cauchy weights), against the few metric measurements the frame has -- the anchor: a LiDAR sweep, COLMAP's sparse
points rendered to depth maps -- and applied to every pixel of the prior: z = s p + b in `depth` space, 1 / z = s p + b in `disparity`
space (relative inverse depth, as MiDaS and Depth-Anything give).  The residual spread of the fit is the standard deviation the
'gnll' loss asks for.  The definition is DESIGN.md 8.9 (restated as code in tests/depth_align_reference.py).

Out of scope: spatially varying alignment, sky masks.  The anchor may be the reconstruction's own 3D points: depth_points.py draws them
into the frames (`--anchor_sup_type points` after its CLI, or Config.depth_points_vis / --depth_points_model at load time).

The CLI writes, next to the prior, the folders the loaders already find under `--depth_sup_type T_aligned` (and its `_std` twin,
which 'gnll' reads), plus align_T.txt with every frame's row.  The load-time flags (Config.depth_align_anchor, --depth_align_anchor)
run the same call when a training run loads its frames instead, before the accumulation and the consistency check when those are on;
they use the float32 value, which the CLI's folders round to the PNG's 1 / 256 m.

Everything is enqueued on torch's current stream and nothing synchronises until the numbers are read.  torch only allocates.
There is no host path: without libdepthalign_hip.so and a device every call raises.
"""
import ctypes as C
import os

import numpy as np

from . import _ctypes_util as U
from . import depth_prior_io as IO

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get('DEPTHALIGN_HIP_LIB') or os.path.join(_HERE, 'libdepthalign_hip.so')
ABI_VERSION = 1
MAX_FRAMES = 65535
MAX_ITERS = 32
SPACES = ('depth', 'disparity')
ROW_NAMES = ('s', 'b', 'sigma', 'n_pairs', 'n_inliers', 'status', 'iterations', 'rms')
STATUS_FITTED, STATUS_FEW, STATUS_DEGENERATE, STATUS_INVERTED = 0, 1, 2, 3
STATUS_NAMES = ('fitted', 'too few pairs', 'degenerate', 'inverted or non-finite')
# the parameters: name -> (default, help)
PARAMS = {
    'space': ('depth', 'what the prior is linear in: depth (z = s p + b) or disparity (1 / z = s p + b: relative inverse depth, as MiDaS '
                       'and Depth-Anything give)'),
    'iters': (10, 'reweighted solves after the least-squares one (0 .. %d; 0 = plain least squares)' % MAX_ITERS),
    'c': (1.0, 'the Cauchy weights\' scale, in units of the residuals\' robust standard deviation'),
    'min_points': (16, 'a frame with fewer pixels where prior and anchor are both valid is not fitted and loses its prior (>= 2)'),
    'max_depth': (float('inf'), 'aligned depths beyond this many metres are invalid'),
    'keep_anchor': (False, 'a pixel the anchor measured takes the anchor\'s own value: a completed sparse prior'),
}
ANCHOR_HELP = ('fit each training frame\'s depth prior to the metric prior of this type (one scale and one shift per frame, robustly) on the '
               'device when the frames are loaded, and train on the aligned prior: what makes a monocular prior usable by the absolute '
               'depth losses (\'\' = off)')

_fp = C.c_void_p
# every symbol include/depthalign_hip.h declares: name -> (restype, argtypes)
SYMBOLS = {
    'depthalign_last_error': (C.c_char_p, []),
    'depthalign_abi_version': (C.c_int, []),
    'depthalign_workspace_bytes': (C.c_int64, [C.c_int, C.c_int, C.c_int]),
    'depthalign_fit_apply': (C.c_int, [_fp, C.c_int, C.c_int, C.c_int, _fp, _fp, C.c_int, C.c_int, C.c_double, C.c_int, C.c_double, C.c_int,
                                       C.c_double, _fp, _fp, _fp, _fp]),
}

_lib = None


class DepthAlignError(RuntimeError):
    pass


def lib():
    """The loaded library with typed prototypes.  Raises if it has not been built."""
    global _lib
    if _lib is None:
        _lib = U.load(LIB_PATH, 'libdepthalign_hip.so', SYMBOLS, 'depthalign_abi_version', ABI_VERSION, DepthAlignError,
                      ' (hipcc --offload-arch=gfx950). There is no CPU fallback for the alignment of depth priors.')
    return _lib


def last_error():
    return lib().depthalign_last_error().decode('utf-8', 'replace')


check = U.checker(lib, 'depthalign_last_error', DepthAlignError, 'depthalign call')


def workspace_bytes(n_frames, height, width):
    """Size of the scratch buffer of a call on n_frames frames of height x width pixels (the 12-byte pair of every pixel, the tiles'
    counts and offsets, the frames' pair counts); raises DepthAlignError for sizes the library rejects (n_frames outside 1 .. 65535,
    height * width outside 1 .. 2^28).  Needs no GPU."""
    return U.size(lib().depthalign_workspace_bytes(int(n_frames), int(height), int(width)), last_error, DepthAlignError)


_workspaces = U.Workspaces(workspace_bytes, 2, 'float64')


def check_params(space='depth', iters=10, c=1.0, min_points=16, max_depth=float('inf'), keep_anchor=False, std_floor=0.0):
    """The parameters as the call takes them (max_depth and std_floor in the units of the maps)"""
    if space not in SPACES:
        raise DepthAlignError('space = %r: expected one of %s' % (space, ', '.join(SPACES)))
    try:
        p = dict(space=space, iters=int(iters), c=float(c), min_points=int(min_points), max_depth=float(max_depth),
                 keep_anchor=bool(keep_anchor), std_floor=float(std_floor))
    except (TypeError, ValueError):
        raise DepthAlignError('iters = %r, c = %r, min_points = %r, max_depth = %r, std_floor = %r: expected numbers'
                              % (iters, c, min_points, max_depth, std_floor)) from None
    if not 0 <= p['iters'] <= MAX_ITERS or p['iters'] != iters:
        raise DepthAlignError('iters = %r: expected an integer 0 .. %d' % (iters, MAX_ITERS))
    if not (np.isfinite(p['c']) and p['c'] > 0):
        raise DepthAlignError('c = %r: expected a finite number > 0' % p['c'])
    if p['min_points'] < 2 or p['min_points'] != min_points or p['min_points'] >= 1 << 31:
        raise DepthAlignError('min_points = %r: expected an integer >= 2' % (min_points,))
    if not p['max_depth'] > 0:
        raise DepthAlignError('max_depth = %r: expected a number > 0 (inf = no limit)' % p['max_depth'])
    if not (np.isfinite(p['std_floor']) and p['std_floor'] >= 0):
        raise DepthAlignError('std_floor = %r: expected a finite number >= 0' % p['std_floor'])
    return p


# ---------------------------------------------------------------------------------------------------- the call
NO_CPU = '%s: expected a CUDA/HIP float32 tensor (the alignment of depth priors has no CPU path)'


def _frames(t, name):
    """t checked as a contiguous float32 [F, H, W] tensor; where it lives is asked last (_inputs_ok)"""
    import torch
    if not isinstance(t, torch.Tensor):
        raise DepthAlignError(NO_CPU % name)
    if t.dtype != torch.float32:
        raise DepthAlignError('%s: expected torch.float32, got %s' % (name, t.dtype))
    if t.dim() != 3:
        raise DepthAlignError('%s: expected [F, H, W], got %s' % (name, tuple(t.shape)))
    return U.contiguous(t, name, DepthAlignError)


def _inputs_ok(prior, anchor):
    """prior and anchor checked: dtype, rank, contiguity, one shape, one device, then that it is a GPU"""
    prior, anchor = _frames(prior, 'prior'), _frames(anchor, 'anchor')
    U.same_frames(prior, 'prior', anchor, 'anchor', DepthAlignError)
    if not prior.is_cuda:
        raise DepthAlignError(NO_CPU % 'prior')
    return prior, anchor


def enqueue(prior, anchor, prm, std=True, out=None):
    """The library call alone: Pending.  prm: check_params().  out: the `.tensors` of an earlier call of the same shape and outputs,
    to write into again instead of allocating.  `.tensors`: 'depth' (float32 [F, H, W]), 'std' (float32 [F, H, W], when asked) and
    'rows' (float64 [F, 8] in ROW_NAMES' order); `.get()`: the same as numpy arrays."""
    import torch
    prior, anchor = _inputs_ok(prior, anchor)
    F, H, W = (int(v) for v in prior.shape)
    dev = prior.device
    with torch.cuda.device(dev):
        ws = _workspaces.buffer(dev, F, H, W)
        if out is None:
            out = {'depth': torch.empty_like(prior)}
            if std:
                out['std'] = torch.empty_like(prior)
            out['rows'] = torch.empty((F, len(ROW_NAMES)), dtype=torch.float64, device=dev)
        check(lib().depthalign_fit_apply(U.stream(), F, H, W, U.p(prior), U.p(anchor), SPACES.index(prm['space']), prm['iters'], prm['c'],
                                         prm['min_points'], prm['max_depth'], int(prm['keep_anchor']), prm['std_floor'], U.p(ws),
                                         U.p(out['depth']), U.p(out.get('std')), U.p(out['rows'])), 'depthalign_fit_apply')
    return U.Pending(out, (prior, anchor, ws))


def align_async(prior, anchor, std=True, **params):
    """Pending of the alignment of the float32 device tensor prior [F, H, W] to anchor [F, H, W] (both valid iff > 0).  Everything is
    checked on the host first; then the library call.  Enqueue only."""
    prior, anchor = _inputs_ok(prior, anchor)
    return enqueue(prior, anchor, check_params(**params), std)


def align_priors(prior, anchor, **params):
    """(aligned prior float32 [F, H, W], its standard deviation float32 [F, H, W], rows float64 [F, 8]) on prior's device.  params:
    those of check_params.  Enqueue only."""
    t = align_async(prior, anchor, std=True, **params).tensors
    return t['depth'], t['std'], t['rows']


def totals_line(rows, anchor=''):
    """The one log line of an alignment; rows: float64 [F, 8] (host)"""
    rows = np.asarray(rows, np.float64).reshape(-1, len(ROW_NAMES))
    st = rows[:, 5].astype(np.int64)
    ok = st == STATUS_FITTED
    pairs, inl = rows[ok, 3].sum(), rows[ok, 4].sum()
    return ('depth alignment%s: %d frames, %d fitted, %d too few pairs, %d degenerate, %d inverted; %d pairs, %.1f %% within 3 sigma, '
            'median sigma %.6g' % (' (anchor %s)' % anchor if anchor else '', len(rows), ok.sum(), (st == 1).sum(), (st == 2).sum(),
                                   (st == 3).sum(), pairs, 100.0 * inl / max(pairs, 1.0), np.median(rows[ok, 2]) if ok.any() else 0.0))


# -------------------------------------------------------------------------------------------------------- adapters
def check_anchor(anchor, sup_type, what):
    """The anchor's type name of a flag surface: '' (off) or a type other than the prior's"""
    anchor = anchor or ''
    if not isinstance(anchor, str):
        raise DepthAlignError('%s = %r: expected the type name of a metric prior' % (what, anchor))
    if anchor and anchor == sup_type:
        raise DepthAlignError('%s = %r is the prior itself (depth_sup_type): a prior is aligned to another, metric one' % (what, anchor))
    return anchor


def scene_params(cfg, scale=1.0):
    """The call's parameters of a Config dict; max_depth is metres there, scene units here"""
    g = lambda k: cfg.get('depth_align_' + k, PARAMS[k][0])
    return dict(space=g('space'), iters=g('iters'), c=g('c'), min_points=g('min_points'), max_depth=float(g('max_depth')) * float(scale),
                keep_anchor=g('keep_anchor'))


def add_flags(parser, prefix='depth_align_'):
    """--depth_align_anchor and the parameters on an argparse parser (ddp_train_nerf); the CLI adds them without prefix"""
    if prefix:
        parser.add_argument('--%sanchor' % prefix, default='', help=ANCHOR_HELP)
    for name, (default, text) in PARAMS.items():
        if isinstance(default, bool):
            parser.add_argument('--%s%s' % (prefix, name), action='store_true', help=text)
        elif name == 'space':
            parser.add_argument('--%s%s' % (prefix, name), choices=SPACES, default=default, help='%s (default %s)' % (text, default))
        else:
            parser.add_argument('--%s%s' % (prefix, name), type=type(default), default=default, help='%s (default %s)' % (text, default))


def args_params(args, scale=1.0, prefix='depth_align_'):
    """The call's parameters of parsed flags; max_depth (and the CLI's std_floor) are metres there, scene units here"""
    p = {k: getattr(args, prefix + k) for k in PARAMS}
    p['max_depth'] = float(p['max_depth']) * float(scale)
    if hasattr(args, prefix + 'std_floor'):
        p['std_floor'] = float(getattr(args, prefix + 'std_floor')) * float(scale)
    return p


def _stack(samplers, what):
    if any(s.depth_sup is None for s in samplers):
        raise DepthAlignError('--depth_align_anchor: the training frames carry no %s' % what)
    return IO.stack_frames(samplers, 'depth_sup', '--depth_align_anchor: the frames differ in size; the alignment takes frames of one size',
                           DepthAlignError)


def align_samplers(samplers, anchors, device, want_std=False, **params):
    """The load-time alignment of the NeRF++ path: the priors of the ray samplers (one frame each, all of one size) are fitted to the
    priors of `anchors` (the same frames loaded under the anchor's type) and the aligned ones written back (IO.write_back; with
    want_std the fit's standard deviation too).  A frame that is not fitted loses its prior.  Returns the rows float64 [F, 8]
    (host).  Every rank computes the same bits."""
    import torch
    prior, anchor = _stack(samplers, 'depth prior to align'), _stack(anchors, 'anchor prior')
    if prior.shape != anchor.shape:
        raise DepthAlignError('--depth_align_anchor: %d frames of %s to align against %d of %s' % (prior.shape[:1] + (prior.shape[1:],)
                                                                                                   + anchor.shape[:1] + (anchor.shape[1:],)))
    out, std, rows = align_priors(torch.from_numpy(prior).to(device), torch.from_numpy(anchor).to(device), **params)
    IO.write_back(samplers, out.cpu().numpy(), std.cpu().numpy() if want_std else None)
    return rows.cpu().numpy()


# ------------------------------------------------------------------------------------------------------ PNG encoding
def encode_depth(metres, valid):
    """uint16 PNG values: IO.encode_metres where valid; a fit can give NaN and inf, which are sanitised"""
    return IO.encode_metres(metres, valid, sanitise=True)


_write_png16, absrel = IO.write_png16, IO.absrel


def write_report(path, names, rows, prior=None, out=None, gt=None):
    """align_T.txt: per frame the row and, where ground-truth depth exists, AbsRel of the prior before and after over its valid
    pixels; then the frames that are not fitted, by name"""
    have_gt = gt is not None
    rows = np.asarray(rows, np.float64)
    fmt = lambda r: '%.12g %.12g %.12g %d %d %d %d %.12g' % (r[0], r[1], r[2], r[3], r[4], r[5], r[6], r[7])
    with open(path, 'w') as f:
        f.write('# frame %s%s\n' % (' '.join(ROW_NAMES), ' absrel_before absrel_after' if have_gt else ''))
        for i, name in enumerate(names):
            tail = ' %.6f %.6f' % (absrel(prior[i], gt[i], prior[i] > 0), absrel(out[i], gt[i], out[i] > 0)) if have_gt else ''
            f.write('%s %s%s\n' % (name, fmt(rows[i]), tail))
        tail = ' %.6f %.6f' % (absrel(prior, gt, prior > 0), absrel(out, gt, out > 0)) if have_gt else ''
        f.write('total %d fitted of %d%s\n' % ((rows[:, 5] == STATUS_FITTED).sum(), len(rows), tail))
        for i, name in enumerate(names):
            if rows[i, 5] != STATUS_FITTED:
                f.write('not fitted: %s (%s)\n' % (name, STATUS_NAMES[int(rows[i, 5])]))


# --------------------------------------------------------------------------------------------------------------- CLI
def _run(prior, anchor, device, params):
    import torch
    with np.errstate(invalid='ignore'):
        out, std, rows = align_priors(torch.from_numpy(np.ascontiguousarray(prior, np.float32)).to(device),
                                      torch.from_numpy(np.ascontiguousarray(anchor, np.float32)).to(device), **params)
    return out.cpu().numpy(), std.cpu().numpy(), rows.cpu().numpy()


def run_colmap(args, device):
    """The COLMAP layout: all frames of the scene -> depths{sfx}_{T}_aligned/, depths{sfx}_{T}_aligned_std/, align_T.txt"""
    from . import mip360_data as D
    T, A = args.depth_sup_type, check_anchor(args.anchor_sup_type, args.depth_sup_type, '--anchor_sup_type')
    scenes = []
    for kind in (T, A):
        cfg = D.parse_gin(args.gin_configs, list(args.gin_bindings) + ['Config.data_dir = %r' % args.data_dir,
                                                                       'Config.depth_sup_type = %r' % kind, "Config.depth_loss_type = 'mse'"])
        cfg['depth_cons_views'] = cfg['depth_acc_views'] = 0
        cfg['depth_align_anchor'] = ''
        scenes.append(D.Scene(cfg))
    scene, anchor = scenes
    out, std, rows = _run(scene.depths_sup, anchor.depths_sup, device, args_params(args, scene.scale, ''))
    sup_dir = os.path.join(args.data_dir, 'depths%s_%s' % (IO.colmap_suffix(cfg), T))
    to_sup = dict(zip(D._listdir(os.path.join(args.data_dir, 'images')), D._listdir(sup_dir)))
    out_dir, std_dir = sup_dir + '_aligned', sup_dir + '_aligned_std'
    for d in (out_dir, std_dir):
        os.makedirs(d, exist_ok=True)
    for i, name in enumerate(scene.names):
        png = os.path.splitext(to_sup[name])[0] + '.png'
        _write_png16(os.path.join(out_dir, png), encode_depth(out[i].astype(np.float64) / scene.scale, out[i] > 0))
        _write_png16(os.path.join(std_dir, png), encode_depth(std[i].astype(np.float64) / scene.scale, out[i] > 0))
    report = os.path.join(args.data_dir, 'align_%s.txt' % T)
    write_report(report, scene.names, rows, scene.depths_sup, out, scene.depths_gt)
    print(totals_line(rows, A), flush=True)
    print('wrote %s, %s and %s' % (out_dir, std_dir, report), flush=True)
    return rows


def run_nerfpp(args, device):
    """The NeRF++ layout, each of train / test by itself -> {split}/depth_{T}_aligned/, {split}/depth_{T}_aligned_std/,
    {split}/align_T.txt"""
    from .data_loader_split import load_data_split
    T, A = args.depth_sup_type, check_anchor(args.anchor_sup_type, args.depth_sup_type, '--anchor_sup_type')
    done = {}
    for split, split_dir, files, samplers in IO.nerfpp_splits(args, 'depth' + ('_' + T if T != 'gt' else ''), ['*.png', '*.jpg'],
                                                               depth_sup_type=T):
        anchors = load_data_split(args.datadir, args.scene, split, depth_sup_type=A)
        if any(s.depth_sup is None for s in samplers + anchors):
            raise DepthAlignError('%s: prior and anchor need ground-truth depth/ and the scene\'s scale file to be read in scene units' % split_dir)
        scale = float(samplers[0].depth_scale)
        prior, anchor = _stack(samplers, 'depth prior to align'), _stack(anchors, 'anchor prior')
        if prior.shape != anchor.shape:
            raise DepthAlignError('%s: prior %s and anchor %s differ in shape' % (split_dir, prior.shape, anchor.shape))
        out, std, rows = _run(prior, anchor, device, args_params(args, scale, ''))
        out_dir, std_dir = os.path.join(split_dir, 'depth_%s_aligned' % T), os.path.join(split_dir, 'depth_%s_aligned_std' % T)
        for d in (out_dir, std_dir):
            os.makedirs(d, exist_ok=True)
        names = IO.png_names(files)
        for i in range(len(files)):
            _write_png16(os.path.join(out_dir, names[i]), encode_depth(out[i].astype(np.float64) / scale, out[i] > 0))
            _write_png16(os.path.join(std_dir, names[i]), encode_depth(std[i].astype(np.float64) / scale, out[i] > 0))
        report = os.path.join(split_dir, 'align_%s.txt' % T)
        write_report(report, names, rows, prior, out, IO.stack_gt(samplers))
        print('%s: %s' % (split, totals_line(rows, A)), flush=True)
        print('wrote %s, %s and %s' % (out_dir, std_dir, report), flush=True)
        done[split] = rows
    if not done:
        raise DepthAlignError('no prior of type %r under %s' % (T, os.path.join(args.datadir, args.scene)))
    return done


def make_parser():
    p = IO.base_parser('python -m outdoor_nerf_depth_amd.depth_align', __doc__, together=False)
    p.add_argument('--depth_sup_type', required=True, help='the prior to align: T of depths_T/ or {split}/depth_T/; the result is found '
                   'under --depth_sup_type T_aligned')
    p.add_argument('--anchor_sup_type', required=True, help='the metric prior to align it to: A of depths_A/ or {split}/depth_A/')
    add_flags(p, '')
    p.add_argument('--std_floor', type=float, default=0.0, help='the least standard deviation written, in metres (default 0)')
    IO.add_device_flag(p)
    return p


def main(argv=None):
    import torch
    args = make_parser().parse_args(argv)
    run = {'colmap': run_colmap, 'nerfpp': run_nerfpp}[IO.pick_layout(args)]
    return run(args, torch.device(args.device))


if __name__ == '__main__':
    main()

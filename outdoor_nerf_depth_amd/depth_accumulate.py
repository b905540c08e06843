"""Densifying sparse depth priors from neighbouring frames on the device: multi-sweep accumulation, as KITTI's own annotated depth
is built, applied to the priors before training.  ctypes binding of libdepthacc_hip.so (include/depthacc_hip.h), the adapters of
both front ends, and the CLI

    python -m outdoor_nerf_depth_amd.depth_accumulate --data_dir SCENE --depth_sup_type T [--gin_bindings ...]      (COLMAP layout)
    python -m outdoor_nerf_depth_amd.depth_accumulate --datadir DIR --scene SCENE --depth_sup_type T                (NeRF++ layout)

Every valid prior pixel of a frame's `views` nearest frames is taken into the frame.  Where the frame has no measurement of its own,
the nearest of what arrived is added -- unless a surface nearer by more than `occl_tol` (relative) lies within `occl_radius` pixels
of it: a sparse source shows the background "through" a foreground the target did not measure, and that filter is what keeps it out.
The frame's own pixels are never changed.  The definition is DESIGN.md 8.8 (restated as code in
tests/depth_accumulate_reference.py).

Out of scope: moving objects (a car measured in frame j is pasted where it was), lens distortion and skew (refused by name),
relative priors (what the 'ssi' loss is for; they do not reproject), and splats wider than one pixel.

The CLI writes, next to the prior, the folder the loaders already find under `--depth_sup_type T_acc`, plus accumulate_T.txt with
the counts.  The load-time flags (Config.depth_acc_views, --depth_acc_views) run the same call when a training run loads its frames
instead, before the consistency check when both are on; they use the float32 value, which the CLI's folders round to the PNG's
1 / 256 m.  For COLMAP scenes the CLI takes all frames together while the flag takes the training split.

Everything is enqueued on torch's current stream and nothing synchronises until the numbers are read.  torch only allocates.
There is no host path: without libdepthacc_hip.so and a device every call raises.
"""
import ctypes as C
import os

import numpy as np

from . import _ctypes_util as U
from . import depth_prior_io as IO
from .depth_consistency import (pack_cams, neighbours, validate, upload, cams_from_scene, cams_from_samplers, check_views,   # noqa: F401
                                DepthConsError, MAX_VIEWS, CAM, _upload)
from .depth_prior_io import overlaps as _overlaps, write_png16 as _write_png16, absrel   # noqa: F401

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get('DEPTHACC_HIP_LIB') or os.path.join(_HERE, 'libdepthacc_hip.so')
ABI_VERSION = 1
MAX_FRAMES = 65535
MAX_RADIUS = 8
ROW_NAMES = ('n_own', 'n_candidates', 'n_added', 'n_hidden')
ORIGIN_NONE, ORIGIN_OWN, ORIGIN_ADDED, ORIGIN_HIDDEN = 0, 1, 2, 3
# the two parameters: name -> (default, help)
PARAMS = {
    'occl_radius': (2, 'half width, in pixels, of the window in which a nearer surface hides a neighbour\'s measurement (0 .. %d; 0 = the '
                       'pixel alone: no visibility filter)' % MAX_RADIUS),
    'occl_tol': (0.05, 'a neighbour\'s measurement is hidden when it lies behind the nearest surface of its window by more than this, '
                       'relative to that surface'),
}
VIEWS_HELP = ('take the depth prior of each training frame\'s N nearest frames into the frame on the device when the frames are loaded, '
              'and add it where the frame has no measurement of its own and no nearer surface hides it: a sparse prior becomes several '
              'times denser (0 = off; 1 .. %d)' % MAX_VIEWS)

_fp = C.c_void_p
# every symbol include/depthacc_hip.h declares: name -> (restype, argtypes)
SYMBOLS = {
    'depthacc_last_error': (C.c_char_p, []),
    'depthacc_abi_version': (C.c_int, []),
    'depthacc_workspace_bytes': (C.c_int64, [C.c_int, C.c_int, C.c_int]),
    'depthacc_accumulate': (C.c_int, [_fp, C.c_int, C.c_int, C.c_int, C.c_int, _fp, _fp, _fp, C.c_int, C.c_double, _fp, _fp, _fp, _fp, _fp]),
}

_lib = None


class DepthAccError(DepthConsError):
    pass


def _shared(fn, *args):
    """fn(*args) of depth_consistency's host side, its refusals raised as this module's error"""
    try:
        return fn(*args)
    except DepthAccError:
        raise
    except DepthConsError as e:
        raise DepthAccError(str(e)) from None


def lib():
    """The loaded library with typed prototypes.  Raises if it has not been built."""
    global _lib
    if _lib is None:
        _lib = U.load(LIB_PATH, 'libdepthacc_hip.so', SYMBOLS, 'depthacc_abi_version', ABI_VERSION, DepthAccError,
                      ' (hipcc --offload-arch=gfx950). There is no CPU fallback for the accumulation of depth priors.')
    return _lib


def last_error():
    return lib().depthacc_last_error().decode('utf-8', 'replace')


check = U.checker(lib, 'depthacc_last_error', DepthAccError, 'depthacc call')


def workspace_bytes(n_frames, height, width):
    """Size of the scratch buffer of a call on n_frames frames of height x width pixels (the 8-byte z-buffer and the row partials);
    raises DepthAccError for sizes the library rejects (n_frames outside 1 .. 65535, height * width outside 1 .. 2^28).  Needs no GPU."""
    return U.size(lib().depthacc_workspace_bytes(int(n_frames), int(height), int(width)), last_error, DepthAccError)


_workspaces = U.Workspaces(workspace_bytes, 2, 'float64')


def check_params(occl_radius=2, occl_tol=0.05):
    """The two parameters as the call takes them"""
    p = dict(occl_radius=int(occl_radius), occl_tol=float(occl_tol))
    if not 0 <= p['occl_radius'] <= MAX_RADIUS or p['occl_radius'] != occl_radius:
        raise DepthAccError('occl_radius = %r: expected an integer 0 .. %d' % (occl_radius, MAX_RADIUS))
    if not (np.isfinite(p['occl_tol']) and p['occl_tol'] >= 0):
        raise DepthAccError('occl_tol = %r: expected a finite number >= 0' % p['occl_tol'])
    return p


# ---------------------------------------------------------------------------------------------------- the call
NO_CPU = '%s: expected a CUDA/HIP float32 tensor (the accumulation of depth priors has no CPU path)'


def _frames(t, name):
    """t checked as a contiguous float32 [F, H, W] tensor; where it lives is asked last (_outputs_ok)"""
    import torch
    if not isinstance(t, torch.Tensor):
        raise DepthAccError(NO_CPU % name)
    if t.dtype != torch.float32:
        raise DepthAccError('%s: expected torch.float32, got %s' % (name, t.dtype))
    if t.dim() != 3:
        raise DepthAccError('%s: expected [F, H, W], got %s' % (name, tuple(t.shape)))
    return U.contiguous(t, name, DepthAccError)


def _outputs_ok(depth, depth_out):
    """depth (and depth_out, when given) checked: dtype, shape, contiguity, aliasing, then the device"""
    depth = _frames(depth, 'depth')
    if depth_out is not None:
        depth_out = _frames(depth_out, 'depth_out')
        if depth_out.shape != depth.shape or depth_out.device != depth.device:
            raise DepthAccError('depth_out %s on %s: expected the shape %s and device %s of depth'
                                % (tuple(depth_out.shape), depth_out.device, tuple(depth.shape), depth.device))
        if _overlaps(depth_out, depth):
            raise DepthAccError('depth_out overlaps depth: the resolve pass reads the neighbours of a pixel, so the call cannot run in place')
    if not depth.is_cuda:
        raise DepthAccError(NO_CPU % 'depth')
    return depth, depth_out


def enqueue(depth, cams_d, nbr_d, n_views, prm, origin=True, src=False, rows=True, depth_out=None, out=None):
    """The library call alone, on cameras and neighbour lists that upload() put on the device: Pending.  prm: check_params().  out:
    the `.tensors` of an earlier call of the same shape and outputs, to write into again instead of allocating.  `.tensors`:
    'depth' (float32 [F, H, W]) and, when asked, 'origin' (uint8 [F, H, W]: 0 nothing, 1 own, 2 added, 3 hidden), 'src' (int32
    [F, H, W]: (slot << 28) | source pixel where origin is 2 or 3, else -1) and 'rows' (int64 [F, 4] in ROW_NAMES' order);
    `.get()`: the same as numpy arrays."""
    import torch
    depth, depth_out = _outputs_ok(depth, depth_out)
    F, H, W = (int(v) for v in depth.shape)
    if tuple(cams_d.shape) != (F, CAM):
        raise DepthAccError('cams: %d cameras for %d frames of depth' % (cams_d.shape[0], F))
    dev = depth.device
    with torch.cuda.device(dev):
        ws = _workspaces.buffer(dev, F, H, W)
        if out is None:
            out = {'depth': depth_out if depth_out is not None else torch.empty_like(depth)}
            if origin:
                out['origin'] = torch.empty((F, H, W), dtype=torch.uint8, device=dev)
            if src:
                out['src'] = torch.empty((F, H, W), dtype=torch.int32, device=dev)
            if rows:
                out['rows'] = torch.empty((F, len(ROW_NAMES)), dtype=torch.int64, device=dev)
        check(lib().depthacc_accumulate(U.stream(), F, H, W, n_views, U.p(depth), U.p(cams_d), U.p(nbr_d), prm['occl_radius'],
                                        prm['occl_tol'], U.p(ws), U.p(out['depth']), U.p(out.get('origin')), U.p(out.get('src')),
                                        U.p(out.get('rows'))), 'depthacc_accumulate')
    return U.Pending(out, (depth, cams_d, nbr_d, ws))


def accumulate_async(depth, cams, nbr, occl_radius=2, occl_tol=0.05, origin=True, src=False, rows=True, depth_out=None):
    """Pending of the accumulation into the float32 device tensor depth [F, H, W] (z-depth, valid iff > 0) with the host arrays cams
    float64 [F, 16] (pack_cams) and nbr int [F, V] (neighbours).  depth_out: a float32 device tensor of depth's shape to write the
    denser prior to (it must not overlap depth).  Everything is checked on the host first; then two small uploads and the library
    call.  Enqueue only."""
    depth, depth_out = _outputs_ok(depth, depth_out)
    prm = check_params(occl_radius, occl_tol)
    cams_h, nbr_h = _shared(validate, cams, nbr)
    if cams_h.shape[0] != depth.shape[0]:
        raise DepthAccError('cams: %d cameras for %d frames of depth' % (cams_h.shape[0], depth.shape[0]))
    cams_d, nbr_d, n_views = _upload(cams_h, nbr_h, depth.device)
    return enqueue(depth, cams_d, nbr_d, n_views, prm, origin, src, rows, depth_out)


def accumulate_priors(depth, cams, views=4, nbr=None, **params):
    """(denser prior float32 [F, H, W], origin uint8 [F, H, W], rows int64 [F, 4]) on depth's device: the accumulation of each
    frame's `views` nearest frames (or the lists nbr) into it.  params: the two of accumulate_async.  Enqueue only."""
    cams = np.asarray(cams, np.float64)
    if nbr is None:
        nbr = _shared(neighbours, cams.reshape(len(cams), -1)[:, [7, 11, 15]], _shared(check_views, views, 'views'))
    t = accumulate_async(depth, cams, nbr, origin=True, src=False, rows=True, **params).tensors
    return t['depth'], t['origin'], t['rows']


def totals_line(rows, views):
    """The one log line of a load-time accumulation; rows: int64 [F, 4] (host)"""
    tot = np.asarray(rows, np.int64).sum(0)
    return ('depth accumulation (%d views): %d frames, %d own prior pixels, %d reached by a neighbour, %d added, %d hidden (x %.2f)'
            % (views, len(rows), tot[0], tot[1], tot[2], tot[3], (tot[0] + tot[2]) / max(int(tot[0]), 1)))


# -------------------------------------------------------------------------------------------------------- adapters
def scene_params(cfg):
    """The call's parameters of a Config dict"""
    return dict(occl_radius=int(cfg.get('depth_acc_occl_radius', 2)), occl_tol=float(cfg.get('depth_acc_occl_tol', 0.05)))


def add_flags(parser, prefix='depth_acc_'):
    """--depth_acc_views and the two parameters on an argparse parser (ddp_train_nerf); the CLI adds the two without prefix"""
    if prefix:
        parser.add_argument('--%sviews' % prefix, type=int, default=0, help=VIEWS_HELP)
    for name, (default, text) in PARAMS.items():
        parser.add_argument('--%s%s' % (prefix, name), type=type(default), default=default, help='%s (default %s)' % (text, default))


def args_params(args, prefix='depth_acc_'):
    """The call's parameters of parsed flags"""
    return dict(occl_radius=getattr(args, prefix + 'occl_radius'), occl_tol=getattr(args, prefix + 'occl_tol'))


def accumulate_samplers(samplers, device, views, **params):
    """The load-time accumulation of the NeRF++ path: the priors of the ray samplers (one frame each, all of one size) are taken
    together and the denser ones written back (IO.write_back).  Returns the rows int64 [F, 4] (host).  Every rank computes the same
    bits; nothing is communicated."""
    import torch
    views = _shared(check_views, views, '--depth_acc_views')
    depth = torch.from_numpy(IO.stack_priors(samplers, '--depth_acc_views', 'accumulate', 'accumulation', DepthAccError)).to(device)
    out, _, rows = accumulate_priors(depth, _shared(cams_from_samplers, samplers), views, **params)
    IO.write_back(samplers, out.cpu().numpy())
    return rows.cpu().numpy()


# ------------------------------------------------------------------------------------------------------ PNG encoding
def encode_prior(raw, metres, added):
    """uint16 PNG values of the denser prior: the input's own 16-bit value where nothing is added, rint(metres * 256) clamped to
    [2, 65535] (the loaders read raw values below 2 as invalid) where something is"""
    return np.where(np.asarray(added, bool), IO.encode_metres(metres, added), np.asarray(raw)).astype(np.uint16)


def write_report(path, names, rows, origin, out=None, gt=None, hidden_z=None):
    """accumulate_T.txt: per frame and in total the four counts, the coverage (valid pixels / pixels) before and after and, where
    ground-truth depth exists, AbsRel of the added pixels and of the hidden candidates against it"""
    have_gt = gt is not None
    px = int(np.prod(origin.shape[1:]))

    def tail(sel, r, n):
        t = ' %.6f %.6f' % (r[0] / (px * n), (r[0] + r[2]) / (px * n))
        if have_gt:
            t += ' %.6f %.6f' % (absrel(out[sel], gt[sel], origin[sel] == ORIGIN_ADDED), absrel(hidden_z[sel], gt[sel], origin[sel] == ORIGIN_HIDDEN))
        return t
    IO.write_rows_report(path, names, rows, '%s coverage_before coverage_after%s' % (' '.join(ROW_NAMES), ' absrel_added absrel_hidden' if have_gt else ''),
                         tail)


# --------------------------------------------------------------------------------------------------------------- CLI
def _run(prior_d, cams, views, params):
    """(out, origin, rows, every) on the host: the call, and for the report's AbsRel of the hidden candidates the call once more with
    the window of the pixel alone, which hides nothing: `every` holds the z of every candidate, the hidden ones among them"""
    out, origin, rows = accumulate_priors(prior_d, cams, views, **params)
    every, _, _ = accumulate_priors(prior_d, cams, views, occl_radius=0, occl_tol=0.0)
    return out.cpu().numpy(), origin.cpu().numpy(), rows.cpu().numpy(), every.cpu().numpy()


def run_colmap(args, device):
    """The COLMAP layout: all frames of the scene together -> depths{sfx}_{T}_acc/, accumulate_T.txt"""
    import torch
    from PIL import Image
    from . import mip360_data as D
    T = args.depth_sup_type
    cfg = D.parse_gin(args.gin_configs, list(args.gin_bindings) + ['Config.data_dir = %r' % args.data_dir,
                                                                   'Config.depth_sup_type = %r' % T, "Config.depth_loss_type = 'mse'"])
    cfg['depth_cons_views'] = cfg['depth_acc_views'] = 0
    scene = D.Scene(cfg)
    out, origin, rows, every = _run(torch.from_numpy(scene.depths_sup).to(device), cams_from_scene(scene),
                                    check_views(args.views, '--views'), args_params(args, ''))
    sup_dir = os.path.join(args.data_dir, 'depths%s_%s' % (IO.colmap_suffix(cfg), T))
    to_sup = dict(zip(D._listdir(os.path.join(args.data_dir, 'images')), D._listdir(sup_dir)))
    out_dir = sup_dir + '_acc'
    os.makedirs(out_dir, exist_ok=True)
    for i, name in enumerate(scene.names):
        raw = np.asarray(Image.open(os.path.join(sup_dir, to_sup[name])))
        _write_png16(os.path.join(out_dir, to_sup[name]), encode_prior(raw, out[i].astype(np.float64) / scene.scale, origin[i] == ORIGIN_ADDED))
    report = os.path.join(args.data_dir, 'accumulate_%s.txt' % T)
    write_report(report, scene.names, rows, origin, out, scene.depths_gt, every)
    print(totals_line(rows, args.views), flush=True)
    print('wrote %s and %s' % (out_dir, report), flush=True)
    return rows


def run_nerfpp(args, device):
    """The NeRF++ layout, each of train / test by itself -> {split}/depth_{T}_acc/, {split}/accumulate_T.txt"""
    import torch
    from .data_loader_split import _imread
    T = args.depth_sup_type
    done = {}
    for split, split_dir, files, samplers in IO.nerfpp_splits(args, 'depth' + ('_' + T if T != 'gt' else ''), ['*.png', '*.jpg'],
                                                               depth_sup_type=T):
        if any(s.depth_sup is None for s in samplers):
            raise DepthAccError('%s: the prior needs ground-truth depth/ and the scene\'s scale file to be read in scene units' % split_dir)
        scale = float(samplers[0].depth_scale)
        prior = IO.stack_frames(samplers, 'depth_sup', '%s: the frames differ in size; the accumulation takes frames of one size' % split_dir,
                                DepthAccError)
        out, origin, rows, every = _run(torch.from_numpy(prior).to(device), cams_from_samplers(samplers),
                                        check_views(args.views, '--views'), args_params(args, ''))
        out_dir = os.path.join(split_dir, 'depth_%s_acc' % T)
        os.makedirs(out_dir, exist_ok=True)
        names = IO.png_names(files)
        for i, p in enumerate(files):
            _write_png16(os.path.join(out_dir, names[i]), encode_prior(_imread(p), out[i].astype(np.float64) / scale, origin[i] == ORIGIN_ADDED))
        report = os.path.join(split_dir, 'accumulate_%s.txt' % T)
        write_report(report, names, rows, origin, out, IO.stack_gt(samplers), every)
        print('%s: %s' % (split, totals_line(rows, args.views)), flush=True)
        print('wrote %s and %s' % (out_dir, report), flush=True)
        done[split] = rows
    if not done:
        raise DepthAccError('no prior of type %r under %s' % (T, os.path.join(args.datadir, args.scene)))
    return done


def make_parser():
    p = IO.base_parser('python -m outdoor_nerf_depth_amd.depth_accumulate', __doc__)
    p.add_argument('--depth_sup_type', required=True, help='the prior to densify: T of depths_T/ or {split}/depth_T/; the result is found '
                   'under --depth_sup_type T_acc')
    p.add_argument('--views', type=int, default=4, help='nearest frames taken into every frame (1 .. %d; default 4)' % MAX_VIEWS)
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

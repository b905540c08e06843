"""What the command lines of the six depth-prior tools share (depth_consistency, depth_accumulate, depth_align, depth_complete,
depth_mvs, depth_points): the 16-bit PNG conventions, AbsRel, the parser head, the choice between the two scene
layouts, the walk over a NeRF++ scene's splits and the per-frame-then-total report.  Functions only; nothing here touches a
device or a library."""
import os

import numpy as np


# ------------------------------------------------------------------------------------------------------ PNG encoding
def write_png16(path, a):
    from PIL import Image
    Image.fromarray(np.ascontiguousarray(a, np.uint16)).save(path)


def encode_metres(metres, mask, sanitise=False):
    """uint16 PNG values: rint(metres * 256) clamped to [2, 65535] where mask holds (the loaders read raw values below 2 as
    invalid), 0 elsewhere.  sanitise: a NaN under the mask becomes 2 and +inf 65535 without a warning (a fit can produce either)"""
    v = np.asarray(metres, np.float64)
    if sanitise:
        with np.errstate(invalid='ignore'):
            v = np.clip(np.rint(np.nan_to_num(v, nan=0.0, posinf=65535.0) * 256.0), 2, 65535)
    else:
        v = np.clip(np.rint(v * 256.0), 2, 65535)
    return np.where(np.asarray(mask, bool), v, 0).astype(np.uint16)


def absrel(depth, gt, mask):
    """mean |depth - gt| / gt over mask and gt > 0 (float64), NaN over no pixel"""
    m = np.asarray(mask, bool) & (gt > 0)
    if not m.any():
        return float('nan')
    p, g = depth[m].astype(np.float64), gt[m].astype(np.float64)
    return float(np.mean(np.abs(p - g) / g))


def overlaps(a, b):
    """do the tensors a and b share a byte?"""
    pa, pb = a.data_ptr(), b.data_ptr()
    return pa < pb + b.numel() * b.element_size() and pb < pa + a.numel() * a.element_size()


# ------------------------------------------------------------------------------------------------------------ reports
def write_rows_report(path, names, rows, header, tail=None):
    """path: '# frame ' + header, one line per frame -- its name and its row of counts -- and the line 'total' with their sums.
    tail(sel, r, n): what follows the counts of a line (the coverage, the ground-truth columns), for sel = the frame's index or
    slice(None) for the total, r = the line's counts and n = the frames it covers."""
    rows = np.asarray(rows, np.int64)
    lines = [(i, name, rows[i], 1) for i, name in enumerate(names)] + [(slice(None), 'total', rows.sum(0), len(names))]
    with open(path, 'w') as f:
        f.write('# frame %s\n' % header)
        for sel, name, r, n in lines:
            f.write('%s %s%s\n' % (name, ' '.join(str(int(v)) for v in r), tail(sel, r, n) if tail else ''))


# ---------------------------------------------------------------------------------------------------------------- CLI
def base_parser(prog, doc, verb='taken', together=True):
    """The parser head of a tool: --data_dir, the gin flags, --datadir, --scene; doc: the module's docstring"""
    import argparse
    from .mip360_data import add_gin_flags
    p = argparse.ArgumentParser(prog=prog, description=doc.split('\n\n')[2], formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument('--data_dir', default=None, help='a COLMAP-format scene (the MipNeRF-360 layout)'
                   + ('; all of its frames are %s together' % verb if together else ''))
    add_gin_flags(p)
    p.add_argument('--datadir', default=None, help='the folder of NeRF++-format scenes')
    p.add_argument('--scene', default=None, help='the NeRF++-format scene under --datadir; train and test are %s each by itself' % verb)
    return p


def add_device_flag(parser):
    parser.add_argument('--device', default='cuda:0')


def pick_layout(args, hint=''):
    """'colmap' or 'nerfpp' of parsed flags: exactly one of --data_dir and --datadir, the latter with --scene"""
    if (args.data_dir is None) == (args.datadir is None):
        raise SystemExit('give either --data_dir (COLMAP layout) or --datadir with --scene%s (NeRF++ layout)' % hint)
    if args.datadir is not None and not args.scene:
        raise SystemExit('--datadir needs --scene')
    return 'colmap' if args.data_dir is not None else 'nerfpp'


def colmap_suffix(cfg):
    """'_4' of Config.factor = 4: the suffix of a COLMAP scene's downsampled folders ('' at full size)"""
    factor = int(cfg['factor'])
    return '_%d' % factor if factor > 0 else ''


def nerfpp_splits(args, subdir, exts, empty='{split}: no prior in {folder}', **load_kw):
    """(split, split_dir, files, samplers) of train and test of the NeRF++ scene args.datadir / args.scene: files = what {split}/subdir
    holds with the extensions exts; samplers = load_data_split(..., **load_kw).  A split without files prints `empty` and is left out;
    a caller that gets nothing says so in its own words."""
    from .data_loader_split import load_data_split, find_files
    for split in ('train', 'test'):
        split_dir = os.path.join(args.datadir.rstrip('/'), args.scene, split)
        folder = os.path.join(split_dir, subdir)
        files = find_files(folder, exts=exts)
        if not files:
            print(empty.format(split=split, folder=folder, split_dir=split_dir), flush=True)
            continue
        yield split, split_dir, files, load_data_split(args.datadir, args.scene, split, **load_kw)


def png_names(files):
    return [os.path.splitext(os.path.basename(p))[0] + '.png' for p in files]


def one_size(samplers, what, error):
    """(H, W) of samplers that all have one size, or error(what)"""
    if len(set((s.H, s.W) for s in samplers)) != 1:
        raise error(what)
    return samplers[0].H, samplers[0].W


def stack_frames(samplers, attr, what, error):
    """float32 [F, H, W] of every sampler's attr (one flat frame each); frames of different sizes are error(what)"""
    H, W = one_size(samplers, what, error)
    return np.stack([np.asarray(getattr(s, attr), np.float32).reshape(H, W) for s in samplers], 0)


def stack_priors(samplers, what, verb, noun, error):
    """float32 [F, H, W] of the samplers' depth prior for the stage `what` (its switch), which is to `verb` it: its `noun` takes
    frames of one size that all carry a prior, else error(...)"""
    if any(s.depth_sup is None for s in samplers):
        raise error('%s: the training frames carry no depth prior to %s' % (what, verb))
    return stack_frames(samplers, 'depth_sup', '%s: the frames differ in size; the %s takes frames of one size' % (what, noun), error)


def write_back(samplers, depth, std=None, replace_std=False):
    """A stage's result into the samplers it read: depth[i] into every depth_sup and, where std is given, std[i] into depth_std -- of
    the samplers that carry none or, with replace_std, of all.  Host sampling and the device sampler both read them from there."""
    for i, s in enumerate(samplers):
        s.depth_sup = depth[i].reshape(-1)
        if std is not None and (replace_std or s.depth_std is None):
            s.depth_std = std[i].reshape(-1)


def stack_gt(samplers):
    """[F, H, W] of the samplers' ground-truth depth, None unless every one carries it"""
    if not all(s.depth_gt is not None for s in samplers):
        return None
    return np.stack([s.depth_gt.reshape(s.H, s.W) for s in samplers], 0)

#!/usr/bin/env python3
"""Does the MipNeRF-360 host path of two checkouts make the same library calls?  The check a refactor of mip360.py stands on;
needs a GPU and both checkouts built.

    python tools/mip360_launch_trace.py <checkout>                  # print the trace
    python tools/mip360_launch_trace.py <checkout A> <checkout B>   # one child process per checkout; exit status 1 if they differ

Every kernel launch goes through mip360.lib().<symbol>.  The functions of the loaded handle are wrapped to print, per call, the
symbol and its integer and float arguments (int arrays element by element); a pointer argument prints as * or, when null, 0 --
never its value.  Traced: one Mip360Trainer.train_step with num_glo_features 0 and 4 and one Mip360Model.from_trainer(...).forward
each, at 8 rays (512 / 256 rows: the fm and fused kernels) and at 5 rays (320 / 160 rows: the row-major fallback), with the
module's defaults and then with each USE_* switch turned off in turn.
"""
import argparse
import ctypes as C
import difflib
import os
import subprocess
import sys

SWITCHES = ('USE_FM', 'USE_BATCH_PACK', 'USE_FUSED_PROP', 'USE_DEFER_DW', 'USE_MULTI_DW', 'USE_FUSED_VIEW')
NUMBERS = (C.c_int, C.c_int32, C.c_int64, C.c_uint64, C.c_float, C.c_double)


def show(argtype, v):
    if argtype in NUMBERS:
        return repr(v)
    if argtype is C.POINTER(C.c_int) and isinstance(v, C.Array):
        return repr(list(v))
    null = v is None or v == 0 or (isinstance(v, C.c_void_p) and not v.value)
    return '0' if null else '*'


def show_args(name, argtypes, args):
    return ', '.join(show(t, v) for t, v in zip(argtypes, args))


def wrap(M, out, show_args=show_args):
    """Every function of M.lib() that M.SYMBOLS names writes a line to `out` before it runs: the symbol and
    show_args(symbol, argtypes, args)"""
    h = M.lib()
    for name, (_, argtypes) in M.SYMBOLS.items():
        def traced(*args, _fn=getattr(h, name), _name=name, _types=argtypes):
            out.write('%s(%s)\n' % (_name, show_args(_name, _types, args)))
            return _fn(*args)
        setattr(h, name, traced)


def sections(text):
    """{'==== ' header line: the lines under it}, in order"""
    out, key = {}, None
    for line in text:
        if line.startswith('==== '):
            key = line
        out.setdefault(key, []).append(line)
    return out


def compare(script, checkouts, n_show, timeout=600, per_section=False):
    """`script <checkout>` in one child process per checkout, each under its own timeout, the next only after the last one exited 0
    (check=True raises otherwise).  Prints the first n_show differing lines and a verdict -- with per_section one per '==== ' header
    before it; returns the exit status."""
    texts = [subprocess.run([sys.executable, os.path.abspath(script), c], check=True, stdout=subprocess.PIPE, text=True,
                            timeout=timeout).stdout.splitlines(True) for c in checkouts]
    diff = [d for d in difflib.unified_diff(texts[0], texts[1], 'a', 'b', n=0) if d[0] in '+-' and d[:3] not in ('+++', '---')]
    if per_section:
        a, b = sections(texts[0]), sections(texts[1])
        for key in list(a) + [k for k in b if k not in a]:
            print('%s: %s' % ('identical' if a.get(key) == b.get(key) else 'DIFFERS', (key or '(before the first section)').strip()))
    sys.stdout.writelines(diff[:n_show])
    print('%s: %d and %d calls traced' % ('DIFFERS (%d lines)' % len(diff) if diff else 'identical', *[
        sum(not t.startswith(('-- ', '==== ')) for t in text) for text in texts]))
    return 1 if diff else 0


def trace(checkout, out):
    sys.path.insert(0, os.path.abspath(checkout))
    import numpy as np
    import torch
    from outdoor_nerf_depth_amd import mip360 as M
    dev = torch.device('cuda:0')
    wrap(M, out)

    def run(n, G):
        rs = np.random.RandomState(0)
        he = lambda shapes: [(rs.uniform(-np.sqrt(6.0 / i), np.sqrt(6.0 / i), (i, o)).astype(np.float32), np.zeros(o, np.float32))
                             for i, o in shapes]
        T = lambda x: torch.from_numpy(x).to(dev)
        d = rs.randn(n, 3).astype(np.float32)
        d /= np.linalg.norm(d, axis=-1, keepdims=True)
        rays = dict(origins=T((rs.randn(n, 3) * 0.3).astype(np.float32)), directions=T(d), viewdirs=T(d.copy()),
                    radii=T(np.full((n, 1), 2e-3, np.float32)), near=T(np.full((n, 1), 0.2, np.float32)),
                    far=T(np.full((n, 1), 30., np.float32)))
        gt, sup = T(rs.rand(n, 3).astype(np.float32)), T(rs.uniform(1, 6, n).astype(np.float32))
        jit = [T(rs.rand(n).astype(np.float32)) for _ in range(3)]
        out.write('-- construct\n')
        tr = M.Mip360Trainer(he(M.mlp_shapes(M.PROP_CFG)), he(M.mlp_shapes(M.NERF_CFG, G)), dev, max_steps=1000, num_glo_features=G,
                             num_glo_embeddings=4)
        out.write('-- train_step\n')
        tr.train_step(rays, gt, sup, jitter01=jit, cam_idx=T((np.arange(n) % 4).astype(np.int32)) if G else None)
        out.write('-- from_trainer\n')
        model = M.Mip360Model.from_trainer(tr)
        out.write('-- forward\n')
        model.forward(rays, 0.5, None)
        torch.cuda.synchronize(dev)

    for off in (None,) + SWITCHES:
        if off is not None:
            setattr(M, off, False)
        for n in (8, 5):
            for G in (0, 4):
                out.write('==== %s, %d rays, num_glo_features %d\n' % ('defaults' if off is None else off + ' off', n, G))
                run(n, G)
        if off is not None:
            setattr(M, off, True)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('a')
    ap.add_argument('b', nargs='?')
    ap.add_argument('--show', type=int, default=20, help='print the first N lines of a unified diff where the traces differ')
    args = ap.parse_args()
    if args.b is None:
        trace(args.a, sys.stdout)
        return 0
    return compare(__file__, (args.a, args.b), args.show)


if __name__ == '__main__':
    sys.exit(main())

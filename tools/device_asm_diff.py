#!/usr/bin/env python3
"""Is the device code of two checkouts the same?  The check a refactor of the kernels stands on; needs no GPU.

    python tools/device_asm_diff.py <checkout A> <checkout B> [--only mip360_] [--show N]

Every source of every library in csrc/build.py's table (this checkout's table: the list and the flags are not restated
here) is compiled in both checkouts with that file's flags plus --offload-device-only -S, and the two assembly texts are
compared after dropping the lines that contain __hip_cuid_ (a hash of the input path, the only thing that differs between
two compilations of the same text).  Prints one line per translation unit; exit status 1 if any differs or fails.
"""
import argparse
import difflib
import importlib.util
import os
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join('outdoor_nerf_depth_amd', 'csrc')


def load_build():
    spec = importlib.util.spec_from_file_location('nerfpp_csrc_build', os.path.join(ROOT, CSRC, 'build.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def device_asm(B, checkout, src, flags, out):
    path = os.path.join(checkout, CSRC, src)
    if not os.path.exists(path):
        return None
    subprocess.check_call([B.HIPCC] + B.COMMON + flags + ['--offload-device-only', '-S', path, '-o', out],
                          stderr=subprocess.DEVNULL)
    with open(out) as f:
        return [line for line in f if '__hip_cuid_' not in line]


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('a')
    ap.add_argument('b')
    ap.add_argument('--only', default='', help='compare only the sources whose file name contains this')
    ap.add_argument('--show', type=int, default=0, help='print the first N lines of a unified diff where they differ')
    args = ap.parse_args()
    B = load_build()
    units = [(lib, src, flags) for lib, sources, _ in B.LIBRARIES for src, flags in sources.items()
             if args.only in B.split_source(src)[0]]
    with tempfile.TemporaryDirectory() as tmp, \
            ThreadPoolExecutor(max_workers=int(os.environ.get('NERFPP_BUILD_JOBS', '8'))) as ex:
        jobs = [[ex.submit(device_asm, B, os.path.abspath(c), B.split_source(src)[0], flags, os.path.join(tmp, '%d%s.s' % (i, side)))
                 for c, side in ((args.a, 'a'), (args.b, 'b'))] for i, (_, src, flags) in enumerate(units)]
        bad = 0
        for (lib, src, flags), (ja, jb) in zip(units, jobs):
            try:
                ta, tb = ja.result(), jb.result()
            except subprocess.CalledProcessError:
                ta = tb = None
            diff = []
            if ta is None or tb is None:
                verdict = 'MISSING OR DOES NOT COMPILE'
            elif ta == tb:
                verdict = 'identical (%d lines)' % len(ta)
            else:
                diff = [d for d in difflib.unified_diff(ta, tb, 'a', 'b', n=0) if d[0] in '+-' and d[:3] not in ('+++', '---')]
                verdict = 'DIFFERS (%d lines)' % len(diff)
            bad += not verdict.startswith('identical')
            print('%-28s %-18s %-20s %s' % (verdict, lib, B.split_source(src)[0], ' '.join(flags)), flush=True)
            sys.stdout.writelines(diff[:args.show])
    print('%d of %d translation units differ' % (bad, len(units)))
    return 1 if bad else 0


if __name__ == '__main__':
    sys.exit(main())

#!/usr/bin/env python
"""Golden vectors for the 'gnll' depth loss (tests/golden/depth_gnll.npz): depth_gaussian_log_likelihood of the upstream NeRF++
depth_loss module, computed by that module itself in float64, with torch autograd's gradients for depth_map and weights.

    python tests/golden/make_golden_depth_gnll.py <path to nerf-methods/nerfplusplus>

Upstream's function names an `nn` it never imports; the module gets `nn = torch.nn` after the import, nothing else is changed.  Only
inputs and outputs are stored; no upstream code is copied.  The cases are those of tests/depth_gnll_reference.draw (positions, no
limit -- upstream has none): n = 7 and n = 257 rays of 64 samples, with clamped gated rays, rays the gate holds back and invalid rays.
The samples lie in 0.5 .. 2 and the priors about 0.02 off the rendering: a clamped ray's gradient is 0.5 (D - p)^2 / 1e-6 (x - D)^2 / n,
and the tests compare gradients to 1e-12 absolute, which float64 can only meet for gradients of a few hundred.
"""
import importlib.util
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from tests import depth_gnll_reference as R  # noqa: E402

CASES = {'n7': (20233, 7), 'n257': (20232, 257)}
S = 64


def main(src):
    spec = importlib.util.spec_from_file_location('upstream_depth_loss', os.path.join(src, 'depth_loss.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    mod.nn = torch.nn
    out = {}
    for name, (seed, n) in CASES.items():
        c = R.draw(seed, n, [S], far=2.0, offset=0.02)
        w, x, d, p, sigma = c['w'][0], c['x'][0], c['d'][0], c['p'], c['sigma']
        t64 = lambda a: torch.from_numpy(a.astype(np.float64))
        depth_map, weights = t64(d).requires_grad_(), t64(w).requires_grad_()
        target = torch.stack([t64(p), t64(sigma)], -1)
        valid = torch.from_numpy((p > 0) & (sigma > 0))
        value = mod.depth_gaussian_log_likelihood(depth_map, t64(x), weights, target, valid)
        value.backward()
        ref = R.gnll(w, x, d, p, sigma)
        print('%s: value %.17g, stats %s (supervised, gated, clamped), ungated %d' % (name, float(value.detach()), ref['stats'], (ref['sup'] & ~ref['gated']).sum()))
        assert ref['stats'][2] >= 2 and (ref['sup'] & ~ref['gated']).any() and (~ref['sup']).any()
        out.update({name + '_w': w, name + '_x': x, name + '_d': d, name + '_p': p, name + '_sigma': sigma,
                    name + '_value': np.float64(float(value.detach())), name + '_g_d': depth_map.grad.numpy(), name + '_g_w': weights.grad.numpy()})
    np.savez_compressed(os.path.join(ROOT, 'tests', 'golden', 'depth_gnll.npz'), **out)


if __name__ == '__main__':
    main(sys.argv[1])

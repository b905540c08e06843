"""CPU (no GPU): the per-ray 'kl_ray' / 'urf_ray' depth losses of the MipNeRF-360 path -- the numpy reference
(tests/mip360_depth_rays_reference.py) against torch autograd and against upstream's form where the two coincide, the header's
declarations, the bindings, and every argument check of mip360_depth_loss_rays (made before any device call)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from oracle import mip360_oracle as O
from tests import mip360_depth_rays_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIGMA = 0.375                       # exactly representable in float32


def level(rs, n, S, supervised=0.7):
    """One level's inputs, as tests/test_gpu_mip360_round3.py::_level draws them, plus supervision, distance_mean, directions"""
    sd = np.sort(rs.rand(n, S + 1), -1).astype(np.float32)
    td = (0.3 + 5.0 * sd).astype(np.float32)
    w = (O.softmax(rs.randn(n, S) * 2) * rs.uniform(0.5, 1.0, (n, 1))).astype(np.float32)
    sup = np.where(rs.rand(n) < supervised, rs.uniform(0.5, 5, n), 0).astype(np.float32)
    dm = rs.uniform(0.5, 5, n).astype(np.float32)
    dirs = (rs.randn(n, 3) * 1.3).astype(np.float32)
    return w, td, sup, dm, dirs


def _torch_value(kind, w, td, sup, dm, dirs, sigma, near, empty):
    """The definition written with torch float64 ops (near / empty are constants of the inputs)"""
    import torch
    n = w.shape[0]
    m = (sup > 0).double()
    gt = sup[:, None]
    steps = 0.5 * (td[:, :-1] + td[:, 1:])
    if kind == 'kl_ray':
        length = (td[:, 1:] - td[:, :-1]) * dirs.norm(dim=-1, keepdim=True)
        per_ray = (-torch.log(w + 1e-7) * torch.exp(-(steps - gt) ** 2 / (2 * sigma)) * length).sum(-1)
    else:
        us = sigma / 3
        pdf = torch.exp(-(steps - gt) ** 2 / (2 * us ** 2) - np.log(us) - np.log(np.sqrt(2 * np.pi)))
        per_ray = (sup - dm) ** 2 + (near * (w - pdf) ** 2).sum(-1) + (empty * w ** 2).sum(-1)
    return (m * per_ray).sum() / n


@pytest.mark.parametrize('kind', R.KINDS)
@pytest.mark.parametrize('n,S', [(5, 17), (37, 32)])
def test_reference_gradients_match_torch_autograd(kind, n, S):
    torch = pytest.importorskip('torch')
    rs = np.random.RandomState(n * 100 + S)
    w, td, sup, dm, dirs = level(rs, n, S)
    assert (sup > 0).any() and (sup == 0).any()
    near, empty = R.flags(td, sup, SIGMA)
    if kind == 'urf_ray':
        assert near.any() and empty.any()
    t = lambda a: torch.from_numpy(a.astype(np.float64))
    tw, tdm = t(w).requires_grad_(), t(dm).requires_grad_()
    v = _torch_value(kind, tw, t(td), t(sup), tdm, t(dirs), SIGMA, torch.from_numpy(near), torch.from_numpy(empty))
    v.backward()
    value, g_w, g_dm = R.value_and_grads(kind, w, td, sup, dm, dirs, SIGMA)
    np.testing.assert_allclose(value, float(v.detach()), rtol=1e-13)
    np.testing.assert_allclose(g_w, tw.grad.numpy(), rtol=1e-12, atol=1e-15 * np.abs(g_w).max())
    want_dm = tdm.grad.numpy() if tdm.grad is not None else np.zeros(n)
    np.testing.assert_allclose(g_dm, want_dm, rtol=1e-12, atol=1e-18)
    if kind == 'kl_ray':
        assert (g_dm == 0).all()                                          # no gradient to distance_mean
    assert (g_w[sup == 0] == 0).all() and (g_dm[sup == 0] == 0).all()       # unsupervised rays get none at all


@pytest.mark.parametrize('kind', R.KINDS)
def test_equals_upstreams_form_where_both_are_defined(kind):
    """n == S with every ray supervised: upstream's `loss.sum(-2) * mask` then `.mean()` adds up the same n x S terms and divides
    by S = n, so the value and both gradients coincide -- which pins the element expressions to the existing oracle."""
    rs = np.random.RandomState(3)
    n = S = 24
    w, td, sup, dm, dirs = level(rs, n, S, supervised=2.0)
    assert (sup > 0).all()
    f64 = lambda a: a.astype(np.float64)
    up = kind[:-4]
    want = O.depth_loss(f64(w), f64(td), f64(sup), f64(dm), SIGMA, f64(dirs), up)
    gw_o, gd_o = O.depth_loss_grads(f64(w), f64(td), f64(sup), f64(dm), SIGMA, f64(dirs), up)
    value, g_w, g_dm = R.value_and_grads(kind, w, td, sup, dm, dirs, SIGMA)
    np.testing.assert_allclose(value, want, rtol=1e-12)
    np.testing.assert_allclose(g_w, gw_o, rtol=1e-12, atol=1e-12 * np.abs(gw_o).max())
    np.testing.assert_allclose(g_dm, gd_o, rtol=1e-12, atol=1e-18)


def test_one_ray_kl_is_upstreams_times_the_sample_count():
    """n == 1: upstream's mean over the S columns against this form's sum over them"""
    rs = np.random.RandomState(4)
    S = 32
    w, td, sup, dm, dirs = level(rs, 1, S, supervised=2.0)
    f64 = lambda a: a.astype(np.float64)
    want = S * O.depth_loss(f64(w), f64(td), f64(sup), f64(dm), SIGMA, f64(dirs), 'kl')
    np.testing.assert_allclose(R.value_and_grads('kl_ray', w, td, sup, dm, dirs, SIGMA)[0], want, rtol=1e-12)


def test_float32_evaluation_keeps_the_float32_flags():
    """The float32 evaluation differs from the float64 one by rounding only: same near / empty pattern, small errors"""
    rs = np.random.RandomState(5)
    w, td, sup, dm, dirs = level(rs, 37, 32)
    for kind in R.KINDS:
        v64, g64, _ = R.value_and_grads(kind, w, td, sup, dm, dirs, SIGMA)
        v32, g32, _ = R.value_and_grads(kind, w, td, sup, dm, dirs, SIGMA, np.float32)
        assert g32.dtype == np.float32 and ((g32 == 0) == (g64 == 0)).all()
        np.testing.assert_allclose(v32, v64, rtol=2e-6)
        e_w, e_dm = R.float32_errors(kind, w, td, sup, dm, dirs, SIGMA)
        assert 0 < e_w < 1e-5 and e_dm < 1e-6, (kind, e_w, e_dm)


# ------------------------------------------------------------------------------------------------ header and bindings
def test_header_declares_the_entry_points_and_keeps_abi_9():
    text = open(os.path.join(ROOT, 'include', 'mip360_hip.h')).read()
    assert re.search(r'#define MIP360_ABI_VERSION 9\b', text)
    assert re.search(r'#define MIP360_DEPTH_KL_RAY 5\b', text) and re.search(r'#define MIP360_DEPTH_URF_RAY 6\b', text)
    for name in ('mip360_depth_loss_rays', 'mip360_depth_rays_revision'):
        assert re.search(r'\bint %s\(' % name, text), name


def test_bindings_and_depth_types():
    from outdoor_nerf_depth_amd import mip360 as M
    assert {k: M.DEPTH_TYPES[k] for k in (None, 'none', 'mse', 'l1', 'kl', 'urf')} == \
        {None: 0, 'none': 0, 'mse': 1, 'l1': 2, 'kl': 3, 'urf': 4}
    assert M.DEPTH_TYPES['kl_ray'] == 5 and M.DEPTH_TYPES['urf_ray'] == 6 and len(M.DEPTH_TYPES) == 8
    lib = M.lib()
    assert lib.mip360_abi_version() == M.ABI_VERSION == 9
    assert lib.mip360_depth_rays_revision() == M.DEPTH_RAYS_REVISION == 1
    assert 'mip360_depth_loss_rays' in M.SYMBOLS


def test_entry_point_validates_arguments_without_a_gpu():
    from outdoor_nerf_depth_amd import mip360 as M
    lib = M.lib()
    d = 64                                                     # a non-null value no failing call dereferences
    names = ['stream', 'type', 'n_rays', 'n_levels', 'n_samples', 'weights', 'tdist', 'depth_sup', 'distance_mean', 'directions',
             'sigma', 'scale', 'values', 'g_weights', 'g_distance_mean', 'scalars', 'workspace']
    ptrs = lambda *v: (C.c_void_p * 4)(*v)
    four = ptrs(d, d, d, d)
    ok = [None, 6, 16, 3, (C.c_int * 4)(64, 64, 32, 0), four, four, d, four, d, 0.375, (C.c_float * 4)(1, 1, 1, 1), d, four, four,
          None, d]

    def call(**kw):
        a = list(ok)
        for k, v in kw.items():
            a[names.index(k)] = v
        return lib.mip360_depth_loss_rays(*a)
    err = lambda: lib.mip360_last_error()
    for t in (0, 1, 2, 3, 4, 7, -1):
        assert call(type=t) == 1 and b'5 (kl_ray) or 6 (urf_ray)' in err(), t
    for L in (0, 5, -1):
        assert call(n_levels=L) == 1 and b'1 <= n_levels <= 4' in err(), L
    for S in (0, 65, -3):
        for lvl in range(3):
            counts = [64, 64, 32, 0]
            counts[lvl] = S
            assert call(n_samples=(C.c_int * 4)(*counts)) == 1 and b'1 <= n_samples <= 64' in err(), (S, lvl)
    assert call(n_levels=4) == 1 and b'1 <= n_samples <= 64' in err()             # the fourth count above is 0
    assert call(n_rays=0) == 1 and b'n_rays > 0' in err()
    for kind in (5, 6):
        for ptr in ('n_samples', 'weights', 'tdist', 'depth_sup', 'scale', 'values', 'workspace'):
            assert call(type=kind, **{ptr: None}) == 1 and b'non-null' in err(), ptr
        assert call(type=kind, weights=ptrs(d, None, d, d)) == 1 and b'non-null weights and tdist' in err()
        assert call(type=kind, tdist=ptrs(d, d, None, d)) == 1 and b'non-null weights and tdist' in err()
        for s in (0.0, -0.1, float('nan')):
            assert call(type=kind, sigma=s) == 1 and b'sigma > 0' in err(), s
    assert call(type=6, distance_mean=None) == 1 and b'urf_ray needs distance_mean' in err()
    assert call(type=6, distance_mean=ptrs(d, d, None, d)) == 1 and b'urf_ray needs distance_mean' in err()
    assert call(type=5, directions=None) == 1 and b'kl_ray needs the ray directions' in err()

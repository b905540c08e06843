"""CPU checks of tests/mip360_loss_reference.py, the inputs and bounds tests/test_gpu_mip360_loss_edges.py holds the MipNeRF-360 loss
head and compositing kernels to:
  * the generators make what they promise (exact float32 cumulative sums, ties, coinciding edges, enough non-zero gradients --
    conditions on the inputs, so that a device test cannot pass on all-zero gradients);
  * the oracle's closed-form gradients agree with float64 central differences AT ties (tests/test_mip360_oracle.py uses tie-free
    data);
  * the oracle evaluated in float32 stays inside every bound helper: a bound that float32 numpy misses is wrong."""
import numpy as np
import pytest

from oracle import mip360_oracle as O
from tests import mip360_loss_reference as R

N = 257
f32eps = np.float32(O.EPS32)


def _seed(Sn, Sp):
    return 1000 + 67 * Sn + Sp


@pytest.mark.parametrize('Sn,Sp', R.LOSS_SIZES)
def test_dyadic_family_is_what_the_bounds_assume(Sn, Sp):
    rs = np.random.RandomState(_seed(Sn, Sp))
    c = R.loss_case(rs, 'dyadic', N, Sn, Sp, 1)
    sd_n, w_n, sd_p, w_p = c['sd_n'], c['w_n'], c['sd_p'][0], c['w_p'][0]
    for sd, w in ((sd_n, w_n), (sd_p, w_p)):
        assert sd.dtype == np.float32 and w.dtype == np.float32
        assert (np.diff(sd) >= 0).all() and sd.min() >= 0 and sd.max() <= 1
        assert (w >= 0).all() and (w.astype(np.float64).sum(-1) <= 1).all()
        np.testing.assert_array_equal(np.cumsum(w, -1, dtype=np.float32).astype(np.float64), np.cumsum(w.astype(np.float64), -1))
        assert (np.diff(sd) == 0).mean() >= 0.15                         # equal neighbours: zero-width intervals
        assert 0.25 <= (w == 0).mean() <= 0.5 and (w.sum(-1) == 0).any()
        assert (sd[1] == sd[1, 0]).all()                                  # a ray whose edges are all equal
    if min(Sn, Sp) >= 6:
        assert (sd_n[0, :3] == 0).all() and (sd_n[0, -3:] == 1).all() and (sd_p[0, :3] == 0).all() and (sd_p[0, -3:] == 1).all()
    if Sp >= 32:
        assert (sd_n[..., :, None] == sd_p[..., None, :]).any(-1).mean() >= 0.5     # NeRF edges that sit on a proposal edge
    term = O.lossfun_outer(R.f64(sd_n), R.f64(w_n), R.f64(sd_p), R.f64(w_p))
    grad = O.lossfun_outer_grad_w_env(R.f64(sd_n), R.f64(w_n), R.f64(sd_p), R.f64(w_p))
    assert (term != 0).mean() >= 0.25 and (grad != 0).mean() >= 0.25, ((term != 0).mean(), (grad != 0).mean())


@pytest.mark.parametrize('Sn,Sp', [(1, 1), (2, 63), (33, 7), (64, 64)])
def test_closed_form_gradients_hold_at_ties(Sn, Sp):
    """lossfun_outer_grad_w_env and lossfun_distortion_grad_w against float64 central differences on the tie-laden family.  Both
    losses are piecewise quadratic in the weights, so a central difference is exact except for an interval whose hinge
    max(0, w_i - w_outer_i) has its kink inside the step h, where it is off by at most h sup|f''| / 2 = h / (w_i + eps)."""
    rs = np.random.RandomState(_seed(Sn, Sp))
    n, h = 37, 2.0 ** -30
    c = R.loss_case(rs, 'dyadic', n, Sn, Sp, 1)
    sd_n, w_n, sd_p, w_p = [R.f64(c[k] if k[-1] == 'n' else c[k][0]) for k in ('sd_n', 'w_n', 'sd_p', 'w_p')]
    closed = O.lossfun_outer_grad_w_env(sd_n, w_n, sd_p, w_p)
    lo, hi = O.searchsorted(sd_p, sd_n)
    _, w_outer = O.inner_outer(sd_n, sd_p, w_p)
    kink = (np.abs(w_n - w_outer) <= h) / (w_n + O.EPS32)
    assert (kink > 0).any()                                               # the hinge does sit exactly on its kink somewhere
    for j in range(Sp):
        d = np.zeros_like(w_p)
        d[:, j] = h
        fd = (O.lossfun_outer(sd_n, w_n, sd_p, w_p + d).sum(-1) - O.lossfun_outer(sd_n, w_n, sd_p, w_p - d).sum(-1)) / (2 * h)
        cover = (j >= lo[:, :-1]) & (j < hi[:, 1:])
        tol = h * (kink * cover).sum(-1) + 1e-6 * np.abs(closed[:, j]) + 1e-7
        assert (np.abs(fd - closed[:, j]) <= tol).all(), (j, np.abs(fd - closed[:, j]).max())
    closed = O.lossfun_distortion_grad_w(sd_n, w_n)
    for i in range(Sn):
        d = np.zeros_like(w_n)
        d[:, i] = h
        fd = (O.lossfun_distortion(sd_n, w_n + d) - O.lossfun_distortion(sd_n, w_n - d)) / (2 * h)
        np.testing.assert_allclose(fd, closed[:, i], rtol=1e-6, atol=1e-7)


def _float32_loss_head(c):
    """the oracle's loss-head pieces in float32 and float64 on one case"""
    out = []
    for cast, eps in ((np.float32, f32eps), (np.float64, O.EPS32)):
        sd_n, w_n = cast(c['sd_n']), cast(c['w_n'])
        out.append(dict(
            term=[O.lossfun_outer(sd_n, w_n, cast(s), cast(w), eps) for s, w in zip(c['sd_p'], c['w_p'])],
            grad=[O.lossfun_outer_grad_w_env(sd_n, w_n, cast(s), cast(w), eps) for s, w in zip(c['sd_p'], c['w_p'])],
            dist=O.lossfun_distortion(sd_n, w_n), dist_grad=O.lossfun_distortion_grad_w(sd_n, w_n)))
        assert out[-1]['term'][0].dtype == cast and out[-1]['dist_grad'].dtype == cast
    return out


@pytest.mark.parametrize('Sn,Sp', R.LOSS_SIZES)
def test_float32_oracle_is_within_the_dyadic_tolerance(Sn, Sp):
    """On the dyadic family the float32 evaluation is within DYADIC_RTOL = 64 * 2^-24 of float64 everywhere and zero exactly where
    float64 is zero (measured over the seven size pairs at 257 rays: at most 3.0e-7 relative)."""
    c = R.loss_case(np.random.RandomState(_seed(Sn, Sp)), 'dyadic', N, Sn, Sp, 1)
    lo, hi = _float32_loss_head(c)
    worst = 0.0
    for a, b in ((lo['term'][0], hi['term'][0]), (lo['grad'][0], hi['grad'][0]), (lo['dist'], hi['dist']),
                 (lo['dist_grad'], hi['dist_grad'])):
        np.testing.assert_array_equal(a == 0, b == 0)
        np.testing.assert_allclose(a, b, rtol=R.DYADIC_RTOL, atol=0)
        worst = max(worst, float(np.max(np.abs(a - b) / np.where(b == 0, 1, np.abs(b)))))
    print('float32 oracle vs float64, dyadic (%d, %d): %.3g relative' % (Sn, Sp, worst))
    assert worst <= R.DYADIC_RTOL / 4                    # room for another evaluation order and another division


@pytest.mark.parametrize('family', ['dyadic', 'general'])
@pytest.mark.parametrize('Sn,Sp', R.LOSS_SIZES)
def test_float32_oracle_stays_inside_the_loss_head_bounds(family, Sn, Sp):
    c = R.loss_case(np.random.RandomState(_seed(Sn, Sp) + 1), family, N, Sn, Sp, 1)
    lo, hi = _float32_loss_head(c)
    b = R.interlevel_grad_bound(c['sd_n'], c['w_n'], c['sd_p'][0], c['w_p'][0])
    d = R.distortion_grad_bound(c['sd_n'], c['w_n'])
    ratios = {}
    for name, got, want, bound in (('term', lo['term'][0], hi['term'][0], b['term']), ('grad', lo['grad'][0], hi['grad'][0], b['grad']),
                                   ('dist', lo['dist'], hi['dist'], d['loss']), ('dist_grad', lo['dist_grad'], hi['dist_grad'], d['grad'])):
        err = np.abs(got - want)
        assert (err <= bound).all(), (name, float((err / np.maximum(bound, 1e-300)).max()))
        ratios[name] = float((err / np.maximum(bound, 1e-300)).max())
    inter32 = np.float32(np.mean(lo['term'][0], dtype=np.float32))
    assert abs(inter32 - hi['term'][0].mean()) <= R.interlevel_loss_bound(c['sd_n'], c['w_n'], [(c['sd_p'][0], c['w_p'][0])])
    print('float32 oracle / bound, %s (%d, %d): %s' % (family, Sn, Sp, ratios))
    if family == 'general' and Sn > 1:
        nz = hi['grad'][0] != 0                                            # the bounds are not vacuous
        assert np.median(b['grad'][nz] / np.abs(hi['grad'][0][nz])) < 1e-3
        assert np.median(d['grad'] / np.maximum(np.abs(hi['dist_grad']), 1e-300)) < 1e-3


@pytest.mark.parametrize('opaque', [True, False])
@pytest.mark.parametrize('family', R.COMPOSITING_FAMILIES)
@pytest.mark.parametrize('S', [1, 2, 17, 63, 64])
def test_float32_oracle_stays_inside_the_compositing_bound(S, family, opaque):
    """alpha_weights_backward + volumetric_rendering_backward in float32 against float64, for each single gradient and all three."""
    rs = np.random.RandomState(S * 7 + opaque)
    n = 23
    density, rgbs, tdist, dirs = R.compositing_case(rs, family, n, S)
    g = dict(g_weights=rs.randn(n, S).astype(np.float32), g_rgb=rs.randn(n, 3).astype(np.float32),
             g_distance_mean=rs.randn(n).astype(np.float32))
    worst = 0.0
    for keys in (('g_weights',), ('g_rgb',), ('g_distance_mean',), ('g_weights', 'g_rgb', 'g_distance_mean')):
        sel = {k: g[k] for k in keys}
        with np.errstate(all='ignore'):
            got = R.rendering_backward(density, rgbs, tdist, dirs, np.float32(1), opaque, **sel)[0]
            ratio, want, _ = R.rendering_backward_ratio(got, density, rgbs, tdist, dirs, 1.0, opaque, **sel)
        assert got.dtype == np.float32 and np.isfinite(want).all() and np.isfinite(ratio).all()
        assert (ratio <= 1).all(), (keys, float(ratio.max()))
        worst = max(worst, float(ratio.max()))
        if family == 'plain' and keys == ('g_weights',) and S > 1:                # the bound is not vacuous
            bound = R.compositing_grad_bound(density, tdist, dirs, g['g_weights'], opaque)
            assert np.median(bound[:, :-1] / np.maximum(np.abs(want[:, :-1]), 1e-300)) < 1e-3
    print('float32 oracle / compositing bound, S %d %s opaque %d: %.3g' % (S, family, opaque, worst))

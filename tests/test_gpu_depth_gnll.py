"""GPU: the Gaussian negative-log-likelihood depth loss (depthgnll_levels, csrc/depthgnll_kernels.hip) against
tests/depth_gnll_reference.py, in both training paths and through both CLIs.

Gates of the kernel tests.  They follow from the arithmetic contract -- float64 inside, one float32 rounding on the way out: `stats`
exact; a value within 1e-6 * (1 / n) sum |l_r| of the float64 reference (the sum cancels: l_r has either sign); a gradient entry (the
buffers are pre-filled with 0.5 / -0.25 and ACCUMULATED into) within 4 * 2^-24 * max(|fill|, |scale * g|) of fill + scale * g64;
entries of rays the gate does not let through bit-equal to the fill.  The gate and the clamp are discontinuities, so the generator
(depth_gnll_reference.draw) keeps every ray 1e-4 (relative) off them in float64 on the host, and every case with n >= 64 is asserted
to hold a ray of each class.  Every figure is printed before it is asserted.

Measured on an MI355X (test_gnll_uses_the_uncertainty_of_noisy_priors: the float64 mean |distance_mean - true depth| over the rays
with a true depth, per batch, mean over the last 50 of 400 batches +- standard error): gnll 0.251528 +- 0.001411, rgb-only 2.156599 +-
0.005611, mse on the same priors 0.254543 +- 0.001393; rgb-only - gnll = 329 standard errors of the difference (gate: 3).  The worst
gradient entry of the case list sits at 0.48 of its bound.
"""
import logging
import re
import shutil

import numpy as np
import pytest

torch = pytest.importorskip('torch')
pytestmark = pytest.mark.gpu

from oracle import mip360_oracle as O                                    # noqa: E402
from tests import depth_gnll_reference as R                               # noqa: E402
from tests.test_gpu_mip360 import T, N, dev, _rays                        # noqa: E402

FILLS = (0.5, -0.25)                                                      # g_w, g_d
EPS = 2.0 ** -24
# (n, [S_l], edges, limit): S below, at and just over a wave, S not a multiple of 64, n = 1, n off the workgroup's four rays
CASES = [(1, [1], 0, 0), (7, [3], 0, 0), (64, [64], 0, 0), (64, [65], 1, 0), (257, [64, 64, 32], 1, 0), (1024, [192], 0, 1),
         (1024, [193], 0, 0), (4096, [64, 64, 32], 1, 0)]
SCALES = (0.7, 1.3, 0.25)


@pytest.fixture(scope='module')
def G():
    dev()
    from outdoor_nerf_depth_amd import depth_gnll
    return depth_gnll


_drawn = {}


def case(i):
    """case i of CASES, drawn once and shared"""
    if i not in _drawn:
        n, samples, edges, lim = CASES[i]
        _drawn[i] = R.draw(1000 + i, n, samples, bool(edges), bool(lim))
    return _drawn[i]


def call(G, c, scales=None, fills=FILLS, fold=None, grads=True):
    L = len(c['samples'])
    g_w = [torch.full(w.shape, fills[0], device=dev()) for w in c['w']] if grads else None
    g_d = [torch.full((c['n'],), fills[1], device=dev()) for _ in range(L)] if grads else None
    values, stats = G.gnll_loss([T(w) for w in c['w']], [T(x) for x in c['x']], [T(d) for d in c['d']], T(c['p']), T(c['sigma']),
                                None if c['limit'] is None else T(c['limit']), c['edges'], scales, g_w, g_d, fold)
    torch.cuda.synchronize()
    return N(values).astype(np.float64), N(stats).astype(np.float64), g_w, g_d


def refs_of(c):
    return [R.gnll(c['w'][l], c['x'][l], c['d'][l], c['p'], c['sigma'], c['limit'], c['edges']) for l in range(len(c['samples']))]


def check_gradient(got, fill, sg, gated_rows, tag):
    """got float32 against fill + sg (float64), entry by entry; rows of rays that are not gated bit-equal to the fill"""
    want = fill + sg
    bound = 4 * EPS * np.maximum(abs(fill), np.abs(sg))
    ratio = (np.abs(got.astype(np.float64) - want) / bound)[gated_rows]
    print('%s: %d gated rays, worst entry at %.3f of its bound (max |scale g| %.3e)' % (tag, gated_rows.sum(), ratio.max() if ratio.size else 0.0,
                                                                                       np.abs(sg).max()))
    assert (got[~gated_rows].view(np.int32) == np.float32(fill).view(np.int32)).all(), tag
    assert ratio.size == 0 or ratio.max() <= 1.0, tag


# ------------------------------------------------------------------------------------------------ 1. kernel against reference
@pytest.mark.parametrize('i', range(len(CASES)))
def test_values_stats_and_gradients(G, i):
    c = case(i)
    n, L = c['n'], len(c['samples'])
    census = R.census(c)
    print('case %s: %s, %d nudges' % (CASES[i], census, c['nudged']))
    if n >= 64:
        for k in R.CLASSES:
            assert census[k] >= 1 or (k == 'limit' and c['limit'] is None), k
    scales = list(SCALES[:L])
    values, stats, g_w, g_d = call(G, c, scales)
    for l, ref in enumerate(refs_of(c)):
        tag = 'case %s level %d' % (CASES[i], l)
        print('%s: value %.9g, float64 %.9g, (1 / n) sum |l_r| %.9g; stats %s, float64 %s'
              % (tag, values[l], ref['value'], ref['abs_sum'], stats[l].tolist(), ref['stats'].tolist()))
        np.testing.assert_array_equal(stats[l], ref['stats'])
        assert abs(values[l] - ref['value']) <= 1e-6 * ref['abs_sum'], tag
        s32 = float(np.float32(scales[l]))
        check_gradient(N(g_w[l]), FILLS[0], s32 * ref['g_w'], ref['gated'], tag + ' g_w')
        check_gradient(N(g_d[l]), FILLS[1], s32 * ref['g_d'], ref['gated'], tag + ' g_d')


# ------------------------------------------------------------------------------------------------ 2. further kernel tests
def test_same_call_twice_is_bit_identical(G):
    c = case(7)
    a, b = call(G, c, list(SCALES)), call(G, c, list(SCALES))
    for x, y in ((a[0], b[0]), (a[1], b[1])):
        np.testing.assert_array_equal(x, y)
    for k in (2, 3):
        for x, y in zip(a[k], b[k]):
            assert torch.equal(x.view(torch.int32), y.view(torch.int32))


@pytest.mark.parametrize('how', ['p', 'sigma', 'limit'])
def test_every_ray_unsupervised_is_exactly_zero_and_touches_nothing(G, how):
    c = dict(case(4))
    if how == 'p':
        c['p'] = np.zeros_like(c['p'])
    elif how == 'sigma':
        c['sigma'] = -np.abs(c['sigma'])
    else:
        c['limit'] = (c['p'] * np.float32(0.5)).astype(np.float32)
    total = torch.full((1,), 3.0, device=dev())
    values, stats, g_w, g_d = call(G, c, list(SCALES), fold=dict(total=total))
    assert (values == 0).all() and not np.signbit(values).any() and (stats == 0).all() and float(total) == 3.0
    for g, fill in zip(g_w + g_d, [FILLS[0]] * 3 + [FILLS[1]] * 3):
        assert (N(g).view(np.int32) == np.float32(fill).view(np.int32)).all()


def test_null_gradients_and_scale_are_accepted(G):
    c = case(4)
    plain, stats, _, _ = call(G, c, None, grads=False)
    refs = refs_of(c)
    for l, ref in enumerate(refs):
        assert abs(plain[l] - ref['value']) <= 1e-6 * ref['abs_sum']
        np.testing.assert_array_equal(stats[l], ref['stats'])
    g_w = [None, torch.full(c['w'][1].shape, FILLS[0], device=dev()), None]               # single entries may be null as well
    values, _ = G.gnll_loss([T(w) for w in c['w']], [T(x) for x in c['x']], [T(d) for d in c['d']], T(c['p']), T(c['sigma']), None,
                            True, None, g_w, None)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(N(values).astype(np.float64), plain)
    check_gradient(N(g_w[1]), FILLS[0], refs[1]['g_w'], refs[1]['gated'], 'scale None = 1')


def test_folds_match_the_host_arithmetic(G):
    c = case(4)
    fold = {k: torch.full((1,), v, device=dev()) for k, v in (('total', 2.5), ('last', 9.0), ('others', 9.0), ('n_sup', -1.0))}
    values, stats, _, _ = call(G, c, list(SCALES), fold=fold)
    v32 = values.astype(np.float32)
    total = np.float32(0)
    for s, v in zip(SCALES, v32):
        total = np.float32(total + np.float32(np.float32(s) * v))
    got = {k: float(t) for k, t in fold.items()}
    print('folds %s; values %s' % (got, v32.tolist()))
    assert got['total'] == float(np.float32(np.float32(2.5) + total))
    assert got['last'] == float(v32[2]) and got['others'] == float(np.float32(v32[0] + v32[1])) and got['n_sup'] == stats[2, 0]


def test_argument_errors_name_the_tensor(G):
    c = case(2)
    w, x, d, p, s = T(c['w'][0]), T(c['x'][0]), T(c['d'][0]), T(c['p']), T(c['sigma'])
    with pytest.raises(G.DepthGnllError, match=r'x\[0\]: expected a contiguous tensor of shape \(64, 65\)'):
        G.gnll_loss([w], [x], [d], p, s, edges=True)
    with pytest.raises(G.DepthGnllError, match=r'pred_levels\[0\]: expected a contiguous tensor of shape \(64,\)'):
        G.gnll_loss([w], [x], [d[:32]], p, s)
    with pytest.raises(G.DepthGnllError, match=r'prior_std: expected torch.float32'):
        G.gnll_loss([w], [x], [d], p, s.double())
    with pytest.raises(G.DepthGnllError, match=r'prior: expected a CUDA/HIP'):
        G.gnll_loss([w], [x], [d], p.cpu(), s)
    with pytest.raises(G.DepthGnllError, match=r'limit: expected a contiguous tensor of shape \(64,\)'):
        G.gnll_loss([w], [x], [d], p, s, limit=torch.zeros(128, device=dev())[::2])
    with pytest.raises(G.DepthGnllError, match=r'g_weights\[0\]: expected a contiguous tensor'):
        G.gnll_loss([w], [x], [d], p, s, g_weights=[torch.zeros(64, 128, device=dev())[:, ::2]])
    with pytest.raises(G.DepthGnllError, match=r'g_pred: 2 entries for 1 levels'):
        G.gnll_loss([w], [x], [d], p, s, g_pred=[None, None])
    with pytest.raises(G.DepthGnllError, match=r"fold\['mean'\]: the folds are"):
        G.gnll_loss([w], [x], [d], p, s, fold=dict(mean=torch.zeros(1, device=dev())))
    with pytest.raises(G.DepthGnllError, match=r'weights\[0\]: expected .* S in 1 .. 1024'):
        G.gnll_loss([torch.zeros(4, 1025, device=dev())], [torch.zeros(4, 1025, device=dev())], [d[:4]], p[:4], s[:4])
    both = torch.zeros(64, 64, device=dev())
    with pytest.raises(G.DepthGnllError, match=r'g_w\[0\] and g_w\[1\] are the same buffer'):
        G.gnll_loss([w, w], [x, x], [d, d], p, s, g_weights=[both, both])


# ------------------------------------------------------------------------------------------------ 3. the MipNeRF-360 step
class Recorder(object):
    """depth_gnll.gnll_loss, keeping copies of what a call was given and of the `total` fold and the gradient buffers before it ran"""

    def __init__(self, G):
        self.inner, self.calls = G.gnll_loss, []

    def __call__(self, weights, x, pred_levels, prior, prior_std, limit=None, edges=False, scale=None, g_weights=None, g_pred=None,
                 fold=None):
        rec = dict(w=[N(t) for t in weights], x=[N(t) for t in x], d=[N(t) for t in pred_levels], p=N(prior), sigma=N(prior_std),
                   limit=None if limit is None else N(limit), edges=edges, scale=list(scale), fold_keys=sorted(fold),
                   total_before=float(fold['total']), g_w_before=[N(g) for g in g_weights], g_d_before=[N(g) for g in g_pred])
        out = self.inner(weights, x, pred_levels, prior, prior_std, limit, edges, scale, g_weights, g_pred, fold)
        rec['g_w_after'], rec['g_d_after'] = [N(g) for g in g_weights], [N(g) for g in g_pred]
        self.calls.append(rec)
        return out


def check_accumulated(after, before, sg, gated, tag):
    """after = float32(before + sg) entry by entry on the gated rays, the bits of `before` elsewhere"""
    bound = 4 * EPS * np.maximum(np.abs(before), np.abs(sg))
    miss = np.abs(after.astype(np.float64) - (before.astype(np.float64) + sg))[gated]
    worst = (miss / np.maximum(bound[gated], 1e-300)).max() if miss.size else 0.0
    print('%s: %d gated rays, worst entry at %.3f of its bound' % (tag, gated.sum(), worst))
    assert (after[~gated].view(np.int32) == before[~gated].view(np.int32)).all(), tag
    assert (miss <= bound[gated]).all(), tag


def _mip360_inputs(n, seed=31):
    rs = np.random.RandomState(seed)
    rays = {k: T(v) for k, v in _rays(rs, n).items()}
    gt = T(rs.rand(n, 3).astype(np.float32))
    sup = np.where(rs.rand(n) < .7, rs.uniform(1, 4, n), 0).astype(np.float32)
    std = np.where(rs.rand(n) < .9, sup * np.exp(rs.uniform(np.log(0.01), np.log(0.5), n)), 0).astype(np.float32)
    jit = [T(rs.rand(n).astype(np.float32)) for _ in range(3)]
    return rays, gt, T(sup), T(std), jit


def _mip360_params():
    return O.init_mlp_params(O.PROP_CFG, np.random.RandomState(0)), O.init_mlp_params(O.NERF_CFG, np.random.RandomState(1))


def test_mip360_train_step_scalars_match_the_reference(G, monkeypatch):
    """n = 256: scalars [2], [5] and the depth part of [0] against the reference evaluated on the step's own weights, tdist and
    distance_mean of every level, with kl_ray's level weights; the gradients are accumulated onto what mip360_losses left"""
    from outdoor_nerf_depth_amd import mip360 as M
    rec = Recorder(G)
    monkeypatch.setattr(G, 'gnll_loss', rec)
    n, lam = 256, 0.1
    rays, gt, sup, std, jit = _mip360_inputs(n)
    prop0, nerf0 = _mip360_params()
    tr = M.Mip360Trainer(prop0, nerf0, dev(), max_steps=1000, depth_loss_type='gnll', lambda_depth=lam)
    sc = N(tr.train_step(rays, gt, sup, jitter01=jit, depth_std=std)).astype(np.float64)
    tr.flush()
    torch.cuda.synchronize()
    assert len(rec.calls) == 1
    c = rec.calls[0]
    assert [w.shape for w in c['w']] == [(n, 64), (n, 64), (n, 32)] and [x.shape for x in c['x']] == [(n, 65), (n, 65), (n, 33)]
    assert c['edges'] is True and c['limit'] is None and c['fold_keys'] == ['last', 'others', 'total']
    np.testing.assert_allclose(c['scale'], [lam, lam, 2 * lam], rtol=1e-12)             # prop, prop, (1 + (2 - 1)) * lambda
    np.testing.assert_array_equal(c['d'][2], N(tr.last_distance_mean))
    np.testing.assert_array_equal(c['p'], N(sup))
    np.testing.assert_array_equal(c['sigma'], N(std))
    refs = [R.gnll(c['w'][l], c['x'][l], c['d'][l], c['p'], c['sigma'], None, True) for l in range(3)]
    want_total = c['total_before'] + sum(float(np.float32(k)) * r['value'] for k, r in zip(c['scale'], refs))
    weight = sum(k * r['abs_sum'] for k, r in zip(c['scale'], refs))
    print('mip360 step: scalars %s; float64 depth %.9g, proposals %.9g, total %.9g; stats %s'
          % (sc, refs[2]['value'], refs[0]['value'] + refs[1]['value'], want_total, [r['stats'].tolist() for r in refs]))
    assert all(r['stats'][1] >= 16 for r in refs)
    assert abs(sc[2] - refs[2]['value']) <= 1e-6 * refs[2]['abs_sum']
    assert abs(sc[5] - (refs[0]['value'] + refs[1]['value'])) <= 2e-6 * (refs[0]['abs_sum'] + refs[1]['abs_sum'])
    assert abs(sc[0] - want_total) <= 2e-6 * (abs(c['total_before']) + weight)
    for l in range(3):
        s32 = float(np.float32(c['scale'][l]))
        assert not c['g_d_before'][l].any()
        check_accumulated(c['g_w_after'][l], c['g_w_before'][l], s32 * refs[l]['g_w'], refs[l]['gated'], 'mip360 level %d g_w' % l)
        check_accumulated(c['g_d_after'][l], c['g_d_before'][l], s32 * refs[l]['g_d'], refs[l]['gated'], 'mip360 level %d g_dm' % l)
    np.testing.assert_array_equal(N(tr.last_gnll_stats), np.stack([r['stats'] for r in refs]))
    for tm in (tr.prop, tr.nerf):
        assert bool(torch.isfinite(tm.grads).all()) and float(tm.grads.abs().max()) > 0


def test_mip360_trainer_takes_the_bench_batch_and_needs_the_std(G):
    """4096 rays, 64 / 64 / 32 samples: one step, everything finite, the same bits twice; without depth_std the step raises"""
    from outdoor_nerf_depth_amd import mip360 as M
    rays, gt, sup, std, jit = _mip360_inputs(4096)
    prop0, nerf0 = _mip360_params()
    finals = []
    for rep in range(2):
        tr = M.Mip360Trainer(prop0, nerf0, dev(), max_steps=250000, depth_loss_type='gnll')
        sc = N(tr.train_step(rays, gt, sup, jitter01=jit, depth_std=std))
        tr.flush()
        torch.cuda.synchronize()
        stats = N(tr.last_gnll_stats)
        print('gnll at 4096 rays: scalars %s, stats %s' % (sc, stats.tolist()))
        assert np.isfinite(sc).all() and stats[2, 0] == float(((sup > 0) & (std > 0)).sum()) and stats[2, 1] > 0
        for tm in (tr.prop, tr.nerf):
            assert bool(torch.isfinite(tm.grads).all()) and bool(torch.isfinite(tm.flat).all()) and float(tm.grads.abs().max()) > 0
        finals.append((sc, N(tr.prop.flat), N(tr.nerf.flat)))
    for a, b in zip(*finals):
        np.testing.assert_array_equal(a.view(np.int32), b.view(np.int32))
    with pytest.raises(M.Mip360Error, match=r"'gnll': train_step needs the standard deviation of the prior \(depth_std\)"):
        M.Mip360Trainer(prop0, nerf0, dev(), depth_loss_type='gnll').train_step(rays, gt, sup, jitter01=jit)
    with pytest.raises(ValueError, match=r'gnll \(Gaussian negative'):
        M.Mip360Trainer(prop0, nerf0, dev(), depth_loss_type='nll')


# ------------------------------------------------------------------------------------------------ 4. the NeRF++ step
def _nerfpp_batch(n, seed=3, std=True):
    from outdoor_nerf_depth_amd.synthetic import SyntheticKitti
    rs = np.random.RandomState(seed)
    b = SyntheticKitti().random_batch(n, rs)
    b['depth_sup'] = np.where(rs.rand(n) < 0.7, rs.uniform(0.02, 0.2, n), 0).astype(np.float32)
    if std:
        b['depth_std'] = np.where(rs.rand(n) < 0.9, b['depth_sup'] * np.exp(rs.uniform(np.log(0.01), np.log(0.5), n)), 0).astype(np.float32)
    return {k: T(np.asarray(v, np.float32)) for k, v in b.items() if isinstance(v, np.ndarray)}


def test_nerfpp_train_step_scalars_match_the_reference(G, monkeypatch):
    """n = 64, 16 / 16 samples: per level, [2] = the loss of ret['depth'] with the foreground weights at fg_z_vals under the bound
    p < fg_far, [3] = the supervised rays, [0] = the rgb loss + lambda * [2]; g_w starts from zeros"""
    from outdoor_nerf_depth_amd.trainer import NerfppTrainer
    from outdoor_nerf_depth_amd.model import init_level_params
    rec = Recorder(G)
    monkeypatch.setattr(G, 'gnll_loss', rec)
    lam = 0.25
    tr = NerfppTrainer(dev(), precision=2, cascade_samples=(16, 16), use_depth=True, depth_loss_type='gnll', lambda_depth=lam,
                       level_params=init_level_params(2))
    batch = _nerfpp_batch(64)
    scalars = [N(s).astype(np.float64) for s in tr.train_step(batch)]
    tr.flush()
    torch.cuda.synchronize()
    assert len(rec.calls) == 2
    for m, (sc, c) in enumerate(zip(scalars, rec.calls)):
        S = 16 if m == 0 else 32
        assert [w.shape for w in c['w']] == [(64, S)] == [x.shape for x in c['x']] and c['edges'] is False and c['limit'].shape == (64,)
        assert c['fold_keys'] == ['last', 'n_sup', 'total'] and c['scale'] == [lam]
        np.testing.assert_array_equal(c['p'], N(batch['depth_sup']))
        np.testing.assert_array_equal(c['sigma'], N(batch['depth_std']))
        ref = R.gnll(c['w'][0], c['x'][0], c['d'][0], c['p'], c['sigma'], c['limit'], False)
        print('nerf++ level %d: scalars %s; float64 gnll %.9g ((1 / n) sum |l_r| %.9g), stats %s' % (m, sc, ref['value'], ref['abs_sum'], ref['stats']))
        assert ref['stats'][1] >= 8
        assert abs(sc[2] - ref['value']) <= 1e-6 * ref['abs_sum']
        assert sc[3] == ref['stats'][0]
        assert c['total_before'] == np.float32(sc[1])                                    # rgb-only head: loss = rgb_loss
        assert abs(sc[0] - (sc[1] + float(np.float32(lam)) * ref['value'])) <= 2e-6 * (abs(sc[1]) + lam * ref['abs_sum'])
        assert not c['g_w_before'][0].any() and not c['g_d_before'][0].any()
        check_accumulated(c['g_w_after'][0], c['g_w_before'][0], lam * ref['g_w'], ref['gated'], 'nerf++ level %d g_w' % m)
        check_accumulated(c['g_d_after'][0], c['g_d_before'][0], lam * ref['g_d'], ref['gated'], 'nerf++ level %d g_depth' % m)
        np.testing.assert_array_equal(N(tr.last_gnll_stats[m])[0], ref['stats'])
    for g in tr.grads:
        assert bool(torch.isfinite(g).all()) and float(g[:-4].abs().max()) > 0
    from outdoor_nerf_depth_amd import _lib as L
    tr = NerfppTrainer(dev(), precision=2, cascade_samples=(16, 16), use_depth=True, depth_loss_type='gnll', level_params=init_level_params(2))
    with pytest.raises(L.NerfppError, match="'gnll': the batch has no depth_std"):
        tr.train_step(_nerfpp_batch(64, std=False))
    tr.flush()
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ 5. nothing new for the others
def test_other_depth_types_never_load_the_new_library(G, monkeypatch, tmp_path):
    """with the library unloaded and its path pointing nowhere, every other depth type of both trainers still steps; gnll does not"""
    from outdoor_nerf_depth_amd import mip360 as M
    from outdoor_nerf_depth_amd.trainer import NerfppTrainer
    from outdoor_nerf_depth_amd.model import init_level_params
    monkeypatch.setattr(G, '_lib', None)
    monkeypatch.setattr(G, 'LIB_PATH', str(tmp_path / 'libdepthgnll_hip.so'))
    rays, gt, sup, std, jit = _mip360_inputs(32)
    cam = T(np.arange(32, dtype=np.int32) % 4)
    prop0, nerf0 = _mip360_params()
    kw = dict(num_prop_samples=32, num_nerf_samples=32)
    for kind in ('mse', 'l1', 'kl', 'kl_ray', 'urf_ray', 'ssi', None):
        extra = dict(depth_ssi_groups=4, depth_ssi_min_rays=2) if kind == 'ssi' else {}
        tr = M.Mip360Trainer(prop0, nerf0, dev(), max_steps=1000, depth_loss_type=kind, depth_sigma=0.3, **kw, **extra)
        assert np.isfinite(N(tr.train_step(rays, gt, sup, jitter01=jit, cam_idx=cam if kind == 'ssi' else None))).all()
        tr.flush()
    batch = _nerfpp_batch(64)
    for kind in ('mse', 'l1', 'kl', 'ssi'):
        tr = NerfppTrainer(dev(), precision=2, cascade_samples=(16, 16), use_depth=True, depth_loss_type=kind, level_params=init_level_params(2))
        assert all(np.isfinite(N(s)[:2]).all() for s in tr.train_step(batch))
        tr.flush()
    torch.cuda.synchronize()
    assert G._lib is None
    tr = M.Mip360Trainer(prop0, nerf0, dev(), max_steps=1000, depth_loss_type='gnll', **kw)
    with pytest.raises(G.DepthGnllError, match='libdepthgnll_hip.so not found'):
        tr.train_step(rays, gt, sup, jitter01=jit, depth_std=std)
    tr.flush()
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ 6. it does what it is for
@pytest.fixture(scope='module')
def noisy_scene(tmp_path_factory):
    """write_scene's 12-frame scene whose depths_mono_crop PNGs carry per-pixel Gaussian noise of known standard deviation -- 20 % of
    the depth at about a third of the pixels, 1 % at the rest -- with that standard deviation in depths_mono_crop_std (both metres *
    256; the validity masks kept)"""
    from PIL import Image
    from tests.test_mip360_scene import write_scene
    dev()
    root = tmp_path_factory.mktemp('depth_gnll')
    data = root / 'scene'
    write_scene(str(data), n_frames=12, H=32, W=40)
    (data / 'depths_mono_crop_std').mkdir()
    rs = np.random.RandomState(11)
    files = sorted((data / 'depths_mono_crop').iterdir())
    assert len(files) == 12
    for f in files:
        sup = np.asarray(Image.open(str(f))).astype(np.float64)
        share = np.where(rs.rand(*sup.shape) < 1.0 / 3.0, 0.2, 0.01)
        noisy = np.where(sup > 0, np.clip(np.round(sup * (1.0 + share * rs.randn(*sup.shape))), 2, 65535), 0).astype(np.uint16)
        std = np.where(sup > 0, np.clip(np.round(sup * share), 2, 65535), 0).astype(np.uint16)
        assert ((noisy > 0) == (sup > 0)).all()
        Image.fromarray(noisy).save(str(f))
        Image.fromarray(std).save(str(data / 'depths_mono_crop_std' / f.name))
    return root


def _train_400(data, kind):
    """400 steps of 1024 rays from seed 0 -> the float64 mean |last_distance_mean - TRUE depth| over the rays that have a true depth,
    for each of the last 50 batches"""
    from outdoor_nerf_depth_amd import mip360 as M
    from outdoor_nerf_depth_amd import mip360_data as D
    from outdoor_nerf_depth_amd import mip360_train as TR
    b = ["Config.data_dir = '%s'" % data, 'Config.max_steps = 400', 'Config.batch_size = 1024', 'Config.lr_delay_steps = 0',
         "Config.depth_sup_type = 'mono_crop'", 'Config.sample_every = 1', 'Config.compute_disp_metrics = %s' % (kind is not None),
         "Config.depth_loss_type = '%s'" % (kind or 'mse')]
    cfg = D.parse_gin(bindings=b)
    scene = D.Scene(cfg)
    train = scene.device_frames('train', dev())
    tr = TR.make_trainer(cfg, dev(), n_train_frames=train['cams'].shape[0])
    kept = []
    for step in range(400):
        bt = M.sample_batch(train['cams'], train['rgb_u8'], train['depth_sup'], 0, step, 1024, scene.near, scene.far, depth_gt=train['depth_gt'])
        kw = dict(depth_std=TR.batch_depth_std(train['depth_std'], bt['pix'])) if kind == 'gnll' else {}
        tr.train_step(bt['rays'], bt['rgb'], bt['depth_sup'], jitter01=list(bt['jitter01']), **kw)
        if step >= 350:
            kept.append((tr.last_distance_mean, bt['depth_gt']))
    tr.flush()
    torch.cuda.synchronize()
    out = []
    for dm, gt in kept:
        dm, gt = N(dm).astype(np.float64), N(gt).astype(np.float64)
        out.append(np.abs(dm - gt)[gt > 0].mean())
    return np.asarray(out)


def test_gnll_uses_the_uncertainty_of_noisy_priors(G, noisy_scene):
    """Priors with per-pixel noise of known standard deviation (20 % of the depth at a third of the pixels, 1 % elsewhere), the
    standard-deviation maps supplied.  Metric: the float64 mean |distance_mean - depth_gt| over the rays with a true depth, per batch
    over the last 50 of 400 batches.  'gnll' must be lower than rgb-only by more than 3 standard errors of the difference of the two
    means; 'mse' on the same priors is printed, not gated.  Measured on an MI355X: gnll 0.251528 +- 0.001411, rgb-only 2.156599 +-
    0.005611, mse 0.254543 +- 0.001393 (gnll ahead of mse by 1.5 standard errors of that difference: nothing this test resolves)."""
    data = str(noisy_scene / 'scene')
    res = {kind: _train_400(data, kind) for kind in ('gnll', None, 'mse')}
    stat = {k: (e.mean(), e.std(ddof=1) / np.sqrt(len(e))) for k, e in res.items()}
    for k, (mean, se) in stat.items():
        print('%-8s mean |distance_mean - true depth| = %.6f +- %.6f (standard error, 50 batches)' % (k or 'rgb-only', mean, se))
    gap, se = stat[None][0] - stat['gnll'][0], np.hypot(stat[None][1], stat['gnll'][1])
    print('rgb-only - gnll = %.6f = %.1f standard errors' % (gap, gap / se))
    assert gap > 3 * se, (gap, se)


# ------------------------------------------------------------------------------------------------ 7. CLI
def test_mip360_cli_trains_and_resumes_bit_identically(noisy_scene):
    from tests.test_gpu_mip360_app import _run, _bindings, _load_params
    data = noisy_scene / 'scene'
    extra = ["Config.depth_loss_type = 'gnll'", 'Config.batch_size = 256', 'Config.max_steps = 6', 'Config.checkpoint_every = 3',
             'Config.print_every = 3']
    full, resumed = noisy_scene / 'run', noisy_scene / 'resumed'
    out = _run('mip360_train', _bindings(data, full, extra))
    assert 'step 6/6' in out and (full / 'checkpoint_3').is_file() and (full / 'checkpoint_6').is_file()
    depth = [float(x) for x in re.findall(r'depth=([-\d.e+naif]+)', out)]
    gated = [float(x) for x in re.findall(r'gnll_gated=([-\d.e+naif]+)\n', out)]
    print('mip360_train gnll: depth %s, gnll_gated %s' % (depth, gated))
    assert len(depth) == 3 and all(np.isfinite(depth)), out[-2000:]
    assert len(gated) == 3 and all(0 < x <= 1 for x in gated), out[-2000:]
    resumed.mkdir()
    shutil.copy(str(full / 'checkpoint_3'), str(resumed / 'checkpoint_3'))
    out = _run('mip360_train', _bindings(data, resumed, extra))
    assert 'Resuming from' in out
    a, b = _load_params(full / 'checkpoint_6'), _load_params(resumed / 'checkpoint_6')
    assert a['trainer']['step'] == b['trainer']['step'] == 6 and a['counter'] == b['counter']
    for mlp in ('prop', 'nerf'):
        for k in ('params', 'mu', 'nu'):
            assert torch.equal(a['trainer'][mlp][k], b['trainer'][mlp][k]), (mlp, k)


def test_nerfpp_cli_runs_three_steps(tmp_path):
    dev()
    from outdoor_nerf_depth_amd import ddp_train_nerf as T_
    argv = ['--expname', 'gnll', '--basedir', str(tmp_path), '--synthetic', '--synthetic_hw', '24,32', '--synthetic_frames', '20',
            '--cascade_samples', '16,16', '--use_depth', '--depth_loss_type', 'gnll', '--depth_sup_type', 'mono_crop', '--lambda_depth',
            '0.1', '--sample_every', '2', '--world_size', '1', '--N_rand_override', '128', '--i_weights', '100', '--i_test', '100',
            '--i_print', '1', '--N_iters', '3']
    args = T_.config_parser().parse_args(argv)
    T_.validate_args(args)
    args.world_size = 1
    lines = []

    class Keep(logging.Handler):
        def emit(self, record):
            lines.append(record.getMessage())
    handler = Keep()
    T_.logger.addHandler(handler)
    try:
        T_.ddp_train_nerf(0, args)
    finally:
        T_.logger.removeHandler(handler)
    text = '\n'.join(lines)
    assert 'depth_loss_type = gnll' in (tmp_path / 'gnll' / 'args.txt').read_text()
    found = re.findall(r'step: (\d+) .*?level_0/loss_depth: ([-\d.e+naif]+) .*?level_0/rgb_loss: ([-\d.e+naif]+) .*?'
                       r'level_1/loss_depth: ([-\d.e+naif]+) .*?level_1/rgb_loss: ([-\d.e+naif]+) .*? gnll_gated=([\d.]+)$', text, re.M)
    print('ddp_train_nerf gnll: %s' % found)
    assert [int(f[0]) for f in found] == [0, 1, 2], text[-2000:]                # (the loop counts from the checkpoint's step: 0)
    vals = np.asarray([[float(x) for x in f[1:]] for f in found])
    assert np.isfinite(vals).all() and (vals[:, 4] > 0).all() and (vals[:, 4] <= 1).all()

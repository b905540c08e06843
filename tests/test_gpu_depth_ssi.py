"""GPU: the scale-and-shift-invariant depth loss (depthssi_levels, csrc/depthssi_kernels.hip) against
tests/depth_ssi_reference.py, in both training paths and through both CLIs.

Gates of the kernel tests.  They follow from the arithmetic contract -- float64 inside, one float32 rounding on the way out:
`values`, w and q within rtol 1e-6 of the float64 reference; N, `fitted` and `stats` exact; a gradient entry (the buffers are
pre-filled with 0.5 / -0.25 and ACCUMULATED into) within 4 * 2^-24 * max(|fill|, |scale * g|) of fill + scale * g64; entries of rays
that are unsupervised or in a group that is not fitted bit-equal to the fill.  Every multi-group case plants a group under min_rays,
a group whose rendered depth is bit-equal, a few ids outside 0 .. G - 1 and an empty group; G = 3 cannot hold an empty group next to
those two and a fitted one, so that case leaves the empty group out and the added case (257, 5, 1) plants all four.  The fitted
groups' coefficient of variation of d is asserted on the host to be at least 0.1, so the float64 solve is well conditioned and no
case sits on the fitted edge.  Every figure is printed before it is asserted.

Measured on an MI355X (test_ssi_recovers_geometry_from_per_frame_distorted_priors, the float64 loss of distance_mean against the
TRUE depth, fitted per frame, mean over the last 50 of 400 batches +- standard error): ssi 0.003829 +- 0.000049, rgb-only 0.250783 +-
0.001913, mse on the distorted priors 0.152430 +- 0.001323; rgb-only - ssi = 129 standard errors of the difference (gate: 3).  The
worst gradient entry of the case list sits at 0.25 of its bound.
"""
import logging
import re
import shutil

import numpy as np
import pytest

torch = pytest.importorskip('torch')
pytestmark = pytest.mark.gpu

from oracle import mip360_oracle as O                                    # noqa: E402
from tests import depth_ssi_reference as R                                # noqa: E402
from tests.test_gpu_mip360 import T, N, dev, _rays                        # noqa: E402

FILLS = (0.5, -0.25)
EPS = 2.0 ** -24
CASES = [(1, 1, 1, 8), (7, 1, 1, 3), (64, 1, 1, 8), (257, 3, 1, 8), (257, 5, 1, 8), (1024, 1, 3, 8), (4096, 37, 3, 8)]


@pytest.fixture(scope='module')
def S():
    dev()
    from outdoor_nerf_depth_amd import depth_ssi
    return depth_ssi


def make_case(n, G, levels, min_rays, seed=0):
    """dict(d = [levels] float32 [n], p float32 [n] with about 30 % zeros, g int32 [n] or None, roles = {group: planted role})"""
    rs = np.random.RandomState(seed + 1000 * n + G)
    roles = {}
    if G >= 3:
        roles = {1: 'under', 2: 'constant'}
        if G >= 5:
            roles[3] = 'empty'
    normal = [k for k in range(G) if k not in roles]
    g = np.asarray(normal, np.int32)[rs.randint(0, len(normal), n)]
    if G >= 3:
        idx = rs.permutation(n)
        g[idx[:min_rays + 4]] = 1                                          # 'under': supervision is cut to min_rays - 1 rays below
        g[idx[min_rays + 4:min_rays + 4 + 3 * min_rays]] = 2               # 'constant': plenty of rays, one depth
    d = [rs.uniform(1.0, 6.0, n).astype(np.float32) for _ in range(levels)]
    a, b = rs.uniform(0.5, 2.0, G), rs.uniform(-1.0, 1.0, G)
    p = (a[g] * d[0] + b[g] + 0.2 * rs.randn(n)).astype(np.float32)
    p = np.where(p > 0, p, np.float32(0.5)).astype(np.float32)
    if n >= 7:
        off = rs.rand(n) < 0.3
        off[:4] = False                                                    # (n = 7 keeps at least min_rays = 3 supervised rays)
        p[off] = 0
    if G >= 3:
        p[g == 2] = np.where(np.arange((g == 2).sum()) % 4 == 3, 0, np.abs(p[g == 2]) + 0.5)
        under = np.flatnonzero(g == 1)
        p[under] = np.abs(p[under]) + 0.5
        p[under[min_rays - 1:]] = 0
        for l in range(levels):
            d[l][g == 2] = np.float32(3.7 + l)
    if n >= 257:                                                           # a few ids outside 0 .. G - 1, supervised ones among them
        out = np.flatnonzero(np.isin(g, normal))[::41][:6]
        g[out] = np.asarray([-1, G, G + 5, -7, G, -1], np.int32)[:len(out)]
        p[out[:3]] = np.abs(p[out[:3]]) + 0.5
        roles['outside'] = out
    return dict(d=d, p=p, g=None if (n == 64 and G == 1) else g, roles=roles)


def check_case_is_off_the_fitted_edge(c, G, min_rays):
    """host-side: the planted groups are unfitted for the planted reason, every other group is fitted with CV(d) >= 0.1"""
    d, p, g, roles = c['d'], c['p'], c['g'], c['roles']
    for l, dl in enumerate(d):
        ref = R.ssi(dl, p, g, G, min_rays)
        cv = R.coefficient_of_variation(dl, p, g, G)
        for k in range(G):
            role = roles.get(k)
            N_k = ref['fit'][k, 2]
            if role == 'under':
                assert 0 < N_k < min_rays and not ref['fit'][k, 3]
            elif role == 'constant':
                gg = np.zeros(len(p), np.int32) if g is None else g
                vals = dl[(gg == k) & (p > 0)]
                assert N_k >= min_rays and (vals.view(np.int32) == vals.view(np.int32)[0]).all() and not ref['fit'][k, 3]
            elif role == 'empty':
                assert N_k == 0 and not ((g == k).any()) and not ref['fit'][k, 3]
            elif len(p) >= 7:
                assert ref['fit'][k, 3] == 1 and N_k >= min_rays and cv[k] >= 0.1, (l, k, N_k, cv[k])
    if 'outside' in roles:
        out = roles['outside']
        assert ((g[out] < 0) | (g[out] >= G)).all() and (p[out] > 0).any()
    if len(p) >= 64:
        assert 0.15 < (p == 0).mean() < 0.45


def call(S, c, G, min_rays, norm='all', scales=None, fills=None, fold=None):
    """-> (values, fit, stats, [grad buffers]) as numpy"""
    L = len(c['d'])
    fills = fills or [FILLS[l % 2] for l in range(L)]
    bufs = [torch.full((len(c['p']),), f, device=dev()) for f in fills]
    v, fit, stats = S.ssi_loss([T(x) for x in c['d']], T(c['p']), None if c['g'] is None else T(c['g']), G, min_rays, norm, scales,
                               bufs, fold)
    return N(v), N(fit), N(stats), [N(b) for b in bufs]


def check_against_reference(c, G, min_rays, norm, scales, fills, got, tag):
    values, fit, stats, bufs = got
    for l, dl in enumerate(c['d']):
        ref = R.ssi(dl, c['p'], c['g'], G, min_rays, norm)
        rel = abs(float(values[l]) - ref['value']) / max(abs(ref['value']), 1e-300)
        print('%s level %d: value %.9g, float64 %.9g (rel %.2e); supervised %d, in fitted groups %d' % (tag, l, values[l], ref['value'], rel,
                                                                                                     ref['stats'][0], ref['stats'][1]))
        np.testing.assert_allclose(values[l], ref['value'], rtol=1e-6, atol=0)
        on = ref['fit'][:, 3] == 1
        np.testing.assert_array_equal(fit[l][:, 3], ref['fit'][:, 3])
        np.testing.assert_array_equal(fit[l][:, 2], ref['fit'][:, 2])
        np.testing.assert_array_equal(stats[l], ref['stats'])
        if on.any():
            print('%s level %d: max rel error of w %.2e, of q %.2e' % (tag, l, np.abs(fit[l][on, 0] / ref['fit'][on, 0] - 1).max(),
                                                                     np.abs(fit[l][on, 1] / ref['fit'][on, 1] - 1).max()))
        np.testing.assert_allclose(fit[l][on, :2], ref['fit'][on, :2], rtol=1e-6, atol=0)
        assert (fit[l][~on, :2] == 0).all()
        sg = float(np.float32(scales[l])) * ref['grad']
        fill = np.float32(fills[l])
        want = float(fill) + sg
        bound = 4 * EPS * np.maximum(abs(float(fill)), np.abs(sg))
        err = np.abs(bufs[l].astype(np.float64) - want)
        t = ref['touched']
        if t.any():
            print('%s level %d: gradient buffer, worst error / bound = %.3f over %d owned entries' % (tag, l, (err[t] / bound[t]).max(), t.sum()))
            assert (err[t] <= bound[t]).all()
        np.testing.assert_array_equal(bufs[l][~t].view(np.int32), np.full((~t).sum(), fill, np.float32).view(np.int32))


# ------------------------------------------------------------------------------------------------ 1. the case list
@pytest.mark.parametrize('norm', R.NORMS)
@pytest.mark.parametrize('n,G,levels,min_rays', CASES)
def test_values_fit_stats_and_gradients(S, n, G, levels, min_rays, norm):
    c = make_case(n, G, levels, min_rays)
    check_case_is_off_the_fitted_edge(c, G, min_rays)
    scales = [0.37, 1.5, 0.11][:levels]
    for flip in (0, 1):                                                    # both fills on every level
        fills = [FILLS[(l + flip) % 2] for l in range(levels)]
        got = call(S, c, G, min_rays, norm, scales, fills)
        check_against_reference(c, G, min_rays, norm, scales, fills, got, '(%d, %d, %d) %s' % (n, G, levels, norm))
    if n == 1:
        assert got[0][0] == 0 and got[2][0, 0] == 1 and got[2][0, 1] == 0    # one ray is under every min_rays: nothing fitted


def test_no_scale_no_grads_no_group(S):
    """the defaults: scale 1, no gradient buffers, one group without ids"""
    c = make_case(64, 1, 1, 8)
    v, fit, stats = S.ssi_loss([T(c['d'][0])], T(c['p']))
    ref = R.ssi(c['d'][0], c['p'])
    np.testing.assert_allclose(N(v)[0], ref['value'], rtol=1e-6)
    np.testing.assert_array_equal(N(stats)[0], ref['stats'])
    assert tuple(fit.shape) == (1, 1, 4) and tuple(stats.shape) == (1, 2)


def test_group_ids_read_in_place_from_a_pixel_table(S):
    """group = the sampler's pix [n, 3]: the frame column with an element stride of 3"""
    c = make_case(4096, 37, 3, 8)
    pix = np.stack([c['g'], np.arange(4096, dtype=np.int32) % 40, np.arange(4096, dtype=np.int32) % 32], 1).astype(np.int32)
    a = S.ssi_loss([T(x) for x in c['d']], T(c['p']), T(c['g']), 37)
    b = S.ssi_loss([T(x) for x in c['d']], T(c['p']), T(pix), 37)
    for x, y in zip(a, b):
        np.testing.assert_array_equal(N(x).view(np.int32), N(y).view(np.int32))
    assert N(a[0]).min() > 0


# ------------------------------------------------------------------------------------------------ 2. determinism, nothing supervised
def test_same_call_twice_is_bit_identical(S):
    c = make_case(4096, 37, 3, 8)
    a, b = call(S, c, 37, 8, 'all', [0.37, 1.5, 0.11]), call(S, c, 37, 8, 'all', [0.37, 1.5, 0.11])
    for x, y in zip(a[:3] + tuple(a[3]), b[:3] + tuple(b[3])):
        np.testing.assert_array_equal(x.view(np.int32), y.view(np.int32))
    assert np.abs(a[3][0] - FILLS[0]).max() > 0


@pytest.mark.parametrize('norm', R.NORMS)
def test_every_ray_unsupervised_is_exactly_zero_and_touches_nothing(S, norm):
    c = make_case(1024, 1, 3, 8)
    c['p'] = np.zeros_like(c['p'])
    fold = {k: torch.full((1,), 7.0, device=dev()) for k in S.FOLD_KEYS}
    values, fit, stats, bufs = call(S, c, 1, 8, norm, [0.37, 1.5, 0.11], fold=fold)
    assert (values == 0).all() and not np.signbit(values).any() and (stats == 0).all() and (fit == 0).all()
    for l, b in enumerate(bufs):
        np.testing.assert_array_equal(b.view(np.int32), np.full(b.shape, FILLS[l % 2], np.float32).view(np.int32))
    assert [float(fold[k]) for k in S.FOLD_KEYS] == [7.0, 0.0, 0.0, 0.0]


# ------------------------------------------------------------------------------------------------ 3. the folds
@pytest.mark.parametrize('norm', R.NORMS)
def test_folds_match_the_host_arithmetic(S, norm):
    """total += sum_l scale[l] * value[l] (float32, level order, from 0, then added); last; others (float32, level order); N_sup --
    from the values the call returns, bit for bit"""
    c = make_case(4096, 37, 3, 8)
    scales = [0.37, 1.5, 0.11]
    six = torch.tensor([1.25, 9.0, float('nan'), float('nan'), 9.0, float('nan')], device=dev())
    fold = dict(total=six[0:1], last=six[2:3], others=six[5:6], n_sup=six[3:4])       # views into one tensor, as the trainers pass
    values, _, stats, _ = call(S, c, 37, 8, norm, scales, fold=fold)
    f32 = np.float32
    t = f32(0)
    for k, v in zip(scales, values):
        t = f32(t + f32(f32(k) * v))
    want = [f32(f32(1.25) + t), f32(9), values[2], stats[0, 0], f32(9), f32(values[0] + values[1])]
    got = N(six)
    print('folds (%s): %s, host %s' % (norm, got, want))
    np.testing.assert_array_equal(got.view(np.int32), np.asarray(want, f32).view(np.int32))
    assert stats[0, 0] == ((c['p'] > 0) & (c['g'] >= 0) & (c['g'] < 37)).sum()


# ------------------------------------------------------------------------------------------------ 4. argument errors
def test_argument_errors_name_the_tensor(S):
    c = make_case(64, 1, 1, 8)
    d, p = T(c['d'][0]), T(c['p'])
    bad = [(dict(pred_levels=[d.double()]), r'pred_levels\[0\]: expected torch.float32'),
           (dict(pred_levels=[d, d[:32]]), r'pred_levels\[1\]: expected a contiguous tensor of shape \(64,\)'),
           (dict(prior=p[::2].repeat_interleave(2)[::1].double()), 'prior: expected torch.float32'),
           (dict(prior=torch.zeros(128, device=dev())[::2]), 'prior: expected a contiguous'),
           (dict(group=torch.zeros(64, device=dev())), 'group: expected a contiguous torch.int32'),
           (dict(group=torch.zeros(64, 2, dtype=torch.int32, device=dev()), n_groups=2), r'group: expected shape \(64,\) or \(64, 3\)'),
           (dict(n_groups=2), 'n_groups = 2 without `group`'),
           (dict(norm='mean'), "norm 'mean'"),
           (dict(min_rays=0), 'min_rays = 0'),
           (dict(scale=[1, 2]), 'scale: 2 entries for 1 levels'),
           (dict(grads=[torch.zeros(64, device=dev()).double()]), r'grads\[0\]: expected torch.float32'),
           (dict(grads=[None, None]), 'grads: 2 entries for 1 levels'),
           (dict(fold=dict(sum=p[:1])), r"fold\['sum'\]: the folds are total, last, others, n_sup"),
           (dict(fold=dict(total=p[:2])), r"fold\['total'\]: expected a one-element float32")]
    for kw, what in bad:
        args = dict(pred_levels=[d], prior=p)
        args.update(kw)
        with pytest.raises(S.DepthSsiError, match=what):
            S.ssi_loss(**args)


# ------------------------------------------------------------------------------------------------ 5. the MipNeRF-360 step
class Recorder(object):
    """depth_ssi.ssi_loss, keeping copies of what a call was given and of the `total` fold before it ran"""

    def __init__(self, S):
        self.inner, self.calls = S.ssi_loss, []

    def __call__(self, pred_levels, prior, group=None, n_groups=1, min_rays=8, norm='all', scale=None, grads=None, fold=None):
        rec = dict(pred=[N(t) for t in pred_levels], prior=N(prior), group=None if group is None else group.cpu().numpy(), n_groups=n_groups,
                   min_rays=min_rays, norm=norm, scale=list(scale), total_before=float(fold['total']), grads_before=[N(g) for g in grads])
        out = self.inner(pred_levels, prior, group, n_groups, min_rays, norm, scale, grads, fold)
        rec['grads_after'] = [N(g) for g in grads]
        self.calls.append(rec)
        return out


def _mip360_inputs(n, F, seed=31):
    rs = np.random.RandomState(seed)
    rays = {k: T(v) for k, v in _rays(rs, n).items()}
    gt = T(rs.rand(n, 3).astype(np.float32))
    sup = T(np.where(rs.rand(n) < .7, rs.uniform(1, 4, n), 0).astype(np.float32))
    jit = [T(rs.rand(n).astype(np.float32)) for _ in range(3)]
    cam = T(rs.randint(0, F, n).astype(np.int32))
    return rays, gt, sup, jit, cam


def _mip360_params():
    return O.init_mlp_params(O.PROP_CFG, np.random.RandomState(0)), O.init_mlp_params(O.NERF_CFG, np.random.RandomState(1))


def test_mip360_train_step_scalars_match_the_reference(S, monkeypatch):
    """n = 256 over 12 frames: scalars [2], [5] and the depth part of [0] against the reference evaluated on the step's own
    distance_mean of every level, with kl_ray's level weights; the gradients land on the zeros mip360_losses left"""
    from outdoor_nerf_depth_amd import mip360 as M
    rec = Recorder(S)
    monkeypatch.setattr(S, 'ssi_loss', rec)
    n, F, lam = 256, 12, 0.1
    rays, gt, sup, jit, cam = _mip360_inputs(n, F)
    prop0, nerf0 = _mip360_params()
    tr = M.Mip360Trainer(prop0, nerf0, dev(), max_steps=1000, depth_loss_type='ssi', lambda_depth=lam, depth_ssi_groups=F, depth_ssi_min_rays=6)
    sc = N(tr.train_step(rays, gt, sup, jitter01=jit, cam_idx=cam)).astype(np.float64)
    tr.flush()
    torch.cuda.synchronize()
    assert len(rec.calls) == 1
    c = rec.calls[0]
    assert len(c['pred']) == 3 and c['n_groups'] == F and c['min_rays'] == 6 and c['norm'] == 'all'
    np.testing.assert_allclose(c['scale'], [lam, lam, 2 * lam], rtol=1e-12)             # prop, prop, (1 + (2 - 1)) * lambda
    np.testing.assert_array_equal(c['pred'][2], N(tr.last_distance_mean))
    refs = [R.ssi(d, c['prior'], c['group'], F, 6, 'all') for d in c['pred']]
    want_total = c['total_before'] + sum(k * r['value'] for k, r in zip(c['scale'], refs))
    print('mip360 step: scalars %s; float64 depth %.9g, proposals %.9g, total %.9g; fitted frames %s'
          % (sc, refs[2]['value'], refs[0]['value'] + refs[1]['value'], want_total, [int(r['fit'][:, 3].sum()) for r in refs]))
    assert all(r['fit'][:, 3].sum() >= F // 2 for r in refs) and refs[2]['value'] > 0
    np.testing.assert_allclose(sc[2], refs[2]['value'], rtol=1e-6)
    np.testing.assert_allclose(sc[5], refs[0]['value'] + refs[1]['value'], rtol=2e-6)
    np.testing.assert_allclose(sc[0], want_total, rtol=2e-6)
    for l in range(3):
        assert not c['grads_before'][l].any()
        sg = float(np.float32(c['scale'][l])) * refs[l]['grad']
        np.testing.assert_allclose(c['grads_after'][l], sg, rtol=0, atol=4 * EPS * np.abs(sg).max())
    np.testing.assert_array_equal(N(tr.last_ssi_stats), np.stack([r['stats'] for r in refs]))
    for tm in (tr.prop, tr.nerf):
        assert bool(torch.isfinite(tm.grads).all()) and float(tm.grads.abs().max()) > 0


def test_mip360_trainer_takes_the_bench_batch(S):
    """4096 rays, 64 / 64 / 32 samples, 37 frames: one step, everything finite, the depth scalars present, the same bits twice"""
    from outdoor_nerf_depth_amd import mip360 as M
    rays, gt, sup, jit, cam = _mip360_inputs(4096, 37)
    pix = torch.stack([cam, cam * 0 + 3, cam * 0 + 5], 1).contiguous()       # the sampler's table: (frame, x, y)
    prop0, nerf0 = _mip360_params()
    finals = []
    for rep in range(2):
        tr = M.Mip360Trainer(prop0, nerf0, dev(), max_steps=250000, depth_loss_type='ssi', depth_ssi_groups=37)
        sc = N(tr.train_step(rays, gt, sup, jitter01=jit, cam_idx=pix))
        tr.flush()
        torch.cuda.synchronize()
        stats = N(tr.last_ssi_stats)
        print('ssi at 4096 rays: scalars %s, stats %s' % (sc, stats.tolist()))
        assert np.isfinite(sc).all() and sc[2] > 0 and sc[5] > 0 and stats[2, 0] == float((sup > 0).sum()) and stats[2, 1] > 0
        for tm in (tr.prop, tr.nerf):
            assert bool(torch.isfinite(tm.grads).all()) and bool(torch.isfinite(tm.flat).all()) and float(tm.grads.abs().max()) > 0
        finals.append((sc, N(tr.prop.flat), N(tr.nerf.flat)))
    for a, b in zip(*finals):
        np.testing.assert_array_equal(a.view(np.int32), b.view(np.int32))


def test_mip360_step_needs_the_frame_indices(S):
    from outdoor_nerf_depth_amd import mip360 as M
    rays, gt, sup, jit, cam = _mip360_inputs(32, 4)
    prop0, nerf0 = _mip360_params()
    with pytest.raises(M.Mip360Error, match=r"'ssi': train_step needs the rays' frame indices \(cam_idx\)"):
        M.Mip360Trainer(prop0, nerf0, dev(), depth_loss_type='ssi', depth_ssi_groups=4).train_step(rays, gt, sup, jitter01=jit)
    with pytest.raises(M.Mip360Error, match='built without depth_ssi_groups'):
        M.Mip360Trainer(prop0, nerf0, dev(), depth_loss_type='ssi').train_step(rays, gt, sup, jitter01=jit, cam_idx=cam)
    with pytest.raises(M.Mip360Error, match='depth_ssi_groups = the number of training frames'):
        M.Mip360Trainer(prop0, nerf0, dev(), depth_loss_type='ssi', depth_ssi_groups=0)
    with pytest.raises(ValueError, match='or ssi'):
        M.Mip360Trainer(prop0, nerf0, dev(), depth_loss_type='huber')


# ------------------------------------------------------------------------------------------------ 6. the NeRF++ step
def _nerfpp_batch(n, seed=3):
    from outdoor_nerf_depth_amd.synthetic import SyntheticKitti
    rs = np.random.RandomState(seed)
    b = SyntheticKitti().random_batch(n, rs)
    b['depth_sup'] = np.where(rs.rand(n) < 0.7, rs.uniform(0.02, 0.2, n), 0).astype(np.float32)
    return {k: T(np.asarray(v, np.float32)) for k, v in b.items() if isinstance(v, np.ndarray)}


def test_nerfpp_train_step_scalars_match_the_reference(S, monkeypatch):
    """n = 64, 16 / 16 samples: per level, [2] = the loss of ret['depth'] (one group, mean over the supervised rays), [3] = the
    supervised rays, [0] = the rgb loss + lambda * [2]"""
    from outdoor_nerf_depth_amd.trainer import NerfppTrainer
    from outdoor_nerf_depth_amd.model import init_level_params
    rec = Recorder(S)
    monkeypatch.setattr(S, 'ssi_loss', rec)
    lam = 0.25
    tr = NerfppTrainer(dev(), precision=2, cascade_samples=(16, 16), use_depth=True, depth_loss_type='ssi', lambda_depth=lam,
                       level_params=init_level_params(2), depth_ssi_min_rays=5)
    batch = _nerfpp_batch(64)
    scalars = [N(s).astype(np.float64) for s in tr.train_step(batch)]
    tr.flush()
    torch.cuda.synchronize()
    assert len(rec.calls) == 2
    for m, (sc, c) in enumerate(zip(scalars, rec.calls)):
        assert len(c['pred']) == 1 and c['group'] is None and c['n_groups'] == 1 and c['min_rays'] == 5 and c['norm'] == 'supervised'
        ref = R.ssi(c['pred'][0], c['prior'], None, 1, 5, 'supervised')
        print('nerf++ level %d: scalars %s; float64 ssi %.9g on %d supervised rays (w %.6g, q %.6g)'
              % (m, sc, ref['value'], ref['stats'][0], ref['fit'][0, 0], ref['fit'][0, 1]))
        cv = R.coefficient_of_variation(c['pred'][0], c['prior'])[0]
        print('nerf++ level %d: coefficient of variation of the rendered depth %.4f (not fitted below 1e-4)' % (m, cv))
        assert ref['fit'][0, 3] == 1 and ref['value'] > 0 and cv >= 1e-3
        np.testing.assert_allclose(sc[2], ref['value'], rtol=1e-6)
        assert sc[3] == ref['stats'][0] == float((N(batch['depth_sup']) > 0).sum())
        assert c['total_before'] == np.float32(sc[1])                                    # rgb-only head: loss = rgb_loss
        np.testing.assert_allclose(sc[0], sc[1] + float(np.float32(lam)) * ref['value'], rtol=2e-6)
        assert not c['grads_before'][0].any()
        sg = lam * ref['grad']
        np.testing.assert_allclose(c['grads_after'][0], sg, rtol=0, atol=4 * EPS * np.abs(sg).max())
    for g in tr.grads:
        assert bool(torch.isfinite(g).all()) and float(g[:-4].abs().max()) > 0


# ------------------------------------------------------------------------------------------------ 7. nothing new for the others
def test_other_depth_types_never_load_the_new_library(S, monkeypatch, tmp_path):
    """with the library unloaded and its path pointing nowhere, every other depth type of both trainers still steps; ssi does not"""
    from outdoor_nerf_depth_amd import mip360 as M
    from outdoor_nerf_depth_amd.trainer import NerfppTrainer
    from outdoor_nerf_depth_amd.model import init_level_params
    monkeypatch.setattr(S, '_lib', None)
    monkeypatch.setattr(S, 'LIB_PATH', str(tmp_path / 'libdepthssi_hip.so'))
    rays, gt, sup, jit, cam = _mip360_inputs(32, 4)
    prop0, nerf0 = _mip360_params()
    kw = dict(num_prop_samples=32, num_nerf_samples=32)
    for kind in ('mse', 'l1', 'kl', 'kl_ray', 'urf_ray', None):
        tr = M.Mip360Trainer(prop0, nerf0, dev(), max_steps=1000, depth_loss_type=kind, depth_sigma=0.3, **kw)
        assert np.isfinite(N(tr.train_step(rays, gt, sup, jitter01=jit))).all()
        tr.flush()
    batch = _nerfpp_batch(64)
    for kind in ('mse', 'l1', 'kl'):
        tr = NerfppTrainer(dev(), precision=2, cascade_samples=(16, 16), use_depth=True, depth_loss_type=kind, level_params=init_level_params(2))
        assert all(np.isfinite(N(s)[:2]).all() for s in tr.train_step(batch))
        tr.flush()
    torch.cuda.synchronize()
    assert S._lib is None
    tr = M.Mip360Trainer(prop0, nerf0, dev(), max_steps=1000, depth_loss_type='ssi', depth_ssi_groups=4, **kw)
    with pytest.raises(S.DepthSsiError, match='libdepthssi_hip.so not found'):
        tr.train_step(rays, gt, sup, jitter01=jit, cam_idx=cam)
    tr.flush()
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ 8. it does what it is for
@pytest.fixture(scope='module')
def distorted_scene(tmp_path_factory):
    """write_scene's 12-frame scene whose depths_mono_crop PNGs are a_f * depth + b_f per frame: a_f in [0.5, 2], b_f in [-1, 1] m
    (the PNGs hold metres * 256), the validity masks kept"""
    from PIL import Image
    from tests.test_mip360_scene import write_scene
    dev()
    root = tmp_path_factory.mktemp('depth_ssi')
    data = root / 'scene'
    write_scene(str(data), n_frames=12, H=32, W=40)
    rs = np.random.RandomState(7)
    files = sorted((data / 'depths_mono_crop').iterdir())
    assert len(files) == 12
    for f in files:
        a, b = rs.uniform(0.5, 2.0), rs.uniform(-1.0, 1.0)
        sup = np.asarray(Image.open(str(f))).astype(np.float64)
        new = np.where(sup > 0, np.clip(np.round(a * sup + b * 256.0), 1, 65535), 0).astype(np.uint16)
        assert ((new > 0) == (sup > 0)).all()
        Image.fromarray(new).save(str(f))
    return root


def _train_400(data, kind):
    """400 steps of 1024 rays from seed 0 -> the float64 reference's loss of last_distance_mean against the TRUE depth, one scale and
    shift per frame, for each of the last 50 batches"""
    from outdoor_nerf_depth_amd import mip360 as M
    from outdoor_nerf_depth_amd import mip360_data as D
    from outdoor_nerf_depth_amd import mip360_train as TR
    b = ["Config.data_dir = '%s'" % data, 'Config.max_steps = 400', 'Config.batch_size = 1024', 'Config.lr_delay_steps = 0',
         "Config.depth_sup_type = 'mono_crop'", 'Config.sample_every = 1', 'Config.compute_disp_metrics = %s' % (kind is not None),
         "Config.depth_loss_type = '%s'" % (kind or 'mse')]
    cfg = D.parse_gin(bindings=b)
    scene = D.Scene(cfg)
    train = scene.device_frames('train', dev())
    F = train['cams'].shape[0]
    tr = TR.make_trainer(cfg, dev(), n_train_frames=F)
    kept = []
    for step in range(400):
        bt = M.sample_batch(train['cams'], train['rgb_u8'], train['depth_sup'], 0, step, 1024, scene.near, scene.far, depth_gt=train['depth_gt'])
        tr.train_step(bt['rays'], bt['rgb'], bt['depth_sup'], jitter01=list(bt['jitter01']), cam_idx=bt['pix'] if kind == 'ssi' else None)
        if step >= 350:
            kept.append((tr.last_distance_mean, bt['depth_gt'], bt['pix'][:, 0]))
    tr.flush()
    torch.cuda.synchronize()
    return np.asarray([R.ssi(N(dm), N(gt), g.cpu().numpy(), F, 8, 'all')['value'] for dm, gt, g in kept])


def test_ssi_recovers_geometry_from_per_frame_distorted_priors(S, distorted_scene):
    """Priors that are right only up to a scale and a shift per frame.  Metric: the loss itself, in float64, of the rendered
    distance_mean against the TRUE depth_gt (grouped by frame), per batch over the last 50 of 400 batches.  'ssi' must be lower than
    rgb-only by more than 3 standard errors of the difference of the two means; 'mse' on the distorted priors is printed, not gated."""
    data = str(distorted_scene / 'scene')
    res = {kind: _train_400(data, kind) for kind in ('ssi', None, 'mse')}
    stat = {k: (e.mean(), e.std(ddof=1) / np.sqrt(len(e))) for k, e in res.items()}
    for k, (mean, se) in stat.items():
        print('%-8s ssi(distance_mean; true depth) = %.6f +- %.6f (standard error, 50 batches)' % (k or 'rgb-only', mean, se))
    gap, se = stat[None][0] - stat['ssi'][0], np.hypot(stat[None][1], stat['ssi'][1])
    print('rgb-only - ssi = %.6f = %.1f standard errors' % (gap, gap / se))
    assert gap > 3 * se, (gap, se)


# ------------------------------------------------------------------------------------------------ 9. CLI
def test_mip360_cli_trains_and_resumes_bit_identically(distorted_scene):
    from tests.test_gpu_mip360_app import _run, _bindings, _load_params
    data = distorted_scene / 'scene'
    extra = ["Config.depth_loss_type = 'ssi'", 'Config.depth_ssi_min_rays = 6', 'Config.batch_size = 256', 'Config.max_steps = 6',
             'Config.checkpoint_every = 3', 'Config.print_every = 3']
    full, resumed = distorted_scene / 'run', distorted_scene / 'resumed'
    out = _run('mip360_train', _bindings(data, full, extra))
    assert 'step 6/6' in out and (full / 'checkpoint_3').is_file() and (full / 'checkpoint_6').is_file()
    depth = [float(x) for x in re.findall(r'depth=([-\d.e+naif]+)', out)]
    fit = [float(x) for x in re.findall(r'ssi_fit=([-\d.e+naif]+)', out)]
    print('mip360_train ssi: depth %s, ssi_fit %s' % (depth, fit))
    assert len(depth) == 3 and all(np.isfinite(depth)) and min(depth) >= 0 and max(depth) > 0, out[-2000:]
    assert len(fit) == 3 and all(0 < x <= 1 for x in fit), out[-2000:]
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
    from outdoor_nerf_depth_amd import ddp_train_nerf as T
    argv = ['--expname', 'ssi', '--basedir', str(tmp_path), '--synthetic', '--synthetic_hw', '24,32', '--synthetic_frames', '20',
            '--cascade_samples', '16,16', '--use_depth', '--depth_loss_type', 'ssi', '--depth_ssi_min_rays', '6', '--depth_sup_type',
            'mono_crop', '--lambda_depth', '0.1', '--sample_every', '2', '--world_size', '1', '--N_rand_override', '128', '--i_weights',
            '100', '--i_test', '100', '--i_print', '1', '--N_iters', '3']
    args = T.config_parser().parse_args(argv)
    T.validate_args(args)
    args.world_size = 1
    lines = []

    class Keep(logging.Handler):
        def emit(self, record):
            lines.append(record.getMessage())
    handler = Keep()
    T.logger.addHandler(handler)
    try:
        T.ddp_train_nerf(0, args)
    finally:
        T.logger.removeHandler(handler)
    text = '\n'.join(lines)
    assert 'depth_loss_type = ssi' in (tmp_path / 'ssi' / 'args.txt').read_text()
    found = re.findall(r'step: (\d+) .*?level_0/loss_depth: ([-\d.e+naif]+) .*?level_0/rgb_loss: ([-\d.e+naif]+) .*?'
                       r'level_1/loss_depth: ([-\d.e+naif]+) .*?level_1/rgb_loss: ([-\d.e+naif]+)', text)
    print('ddp_train_nerf ssi: %s' % found)
    assert [int(f[0]) for f in found] == [0, 1, 2], text[-2000:]                # (the loop counts from the checkpoint's step: 0)
    vals = np.asarray([[float(x) for x in f[1:]] for f in found])
    assert np.isfinite(vals).all() and (vals[:, [0, 2]] >= 0).all() and vals[:, [0, 2]].max() > 0

"""CPU: the float64 restatements and bounds of tests/mip360_rays_reference.py (R), which tests/test_gpu_mip360_ray_edges.py holds the
ray-side kernels to.

* the restatements equal oracle/mip360_oracle.py where they must coincide;
* float32 numpy twins of the kernels pass every bound over the very inputs of the GPU test, no case and no element excluded (this is
  the condition the inputs were chosen under; the worst ratio per kernel is printed, pytest -s);
* mutated twins are rejected, with two exceptions that are pinned as what they are: breaking a tie of the rank sort the other way and
  clipping before the sort both leave every value as it was (sorting equal values, and a monotone clip, commute with the order)."""
import numpy as np
import pytest

from oracle import mip360_oracle as O
from tests import mip360_rays_reference as R

f32, f64 = np.float32, np.float64
WORST = {}


def note(name, value):
    WORST[name] = max(WORST.get(name, 0.0), float(value))
    return float(value)


# ------------------------------------------------------------------------------------------------------------ twins
def rank_sort(cat, m, other=False):
    """the kernel's sort of [t | t0 | t1]: rank = elements smaller + equal elements before it in concatenation order (other: after it)"""
    ne = cat.shape[-1]
    idx = np.arange(ne)
    v, o = cat[..., :, None], cat[..., None, :]
    first = idx[None, :] > idx[:, None] if other else idx[None, :] < idx[:, None]
    rank = np.sum((o < v) | ((o == v) & first), -1)
    out = np.full_like(cat, np.nan)
    np.put_along_axis(out, rank, cat, -1)
    return out


def interp_twin(u, cw, t, strict=False):
    """O.sorted_interp with the bracket test as a switch: strict takes `>` for `>=`"""
    mask = (u[..., None, :] > cw[..., :, None]) if strict else (u[..., None, :] >= cw[..., :, None])
    pick = lambda v: (np.max(np.where(mask, v[..., None], v[..., :1, None]), -2), np.min(np.where(~mask, v[..., None], v[..., -1:, None]), -2))
    fp0, fp1 = pick(t)
    xp0, xp1 = pick(cw)
    with np.errstate(divide='ignore', invalid='ignore'):
        off = np.clip(np.nan_to_num((u - xp0) / (xp1 - xp0), nan=0.0), 0, 1)
    return fp0 + off * (fp1 - fp0)


RESAMPLE_MUTANTS = ('bracket_gt', 'inclusive_prefix', 'no_trim', 'pool_lo', 'pool_hi', 'no_pad')


def resample_twin(c, mut=None):
    """float32 numpy twin of resample_kernel -> sdist [n, ns + 1].  Mutants:
      bracket_gt        `>` for `>=` in the bracket search
      inclusive_prefix  the cumsum including the last bin, [cumsum(w), 1] for [0, cumsum(w[:-1]), 1]: an inclusive prefix for the exclusive
                        one (keeping the leading 0 and letting the last entry be the total instead of 1 stays within delta by construction)
      no_trim           the [1:-1] trim dropped
      pool_lo, pool_hi  the max-pool range off by one at either end: t0 < td for t0 <= td, t1 >= td for t1 > td
      clip_first        the clip applied before the sort (to the three lists, so the pool sees clipped supports too)
      no_pad            u without the half-sample pad
      tie_other         ties of the rank sort broken the other way"""
    sd, w, ns, jit = c['sd'].astype(f32), c['w'].astype(f32), c['ns'], c['jit']
    d, anneal, pad = f32(c['dilation']), f32(R.ANNEAL), f32(c['padding'])
    eps2 = f32(O.EPS32 ** 2)
    if d > 0:
        t0, t1 = sd[..., :-1] - d, sd[..., 1:] + d
        if mut == 'clip_first':
            t0, t1 = np.clip(t0, f32(0), f32(1)), np.clip(t1, f32(0), f32(1))
        cat = np.concatenate([sd, t0, t1], -1)
        td = rank_sort(cat, sd.shape[-1] - 1, mut == 'tie_other') if mut in ('tie_other', 'rank') else np.sort(cat, -1)
        td = np.clip(td, f32(0), f32(1))
        p = w / np.maximum(eps2, np.diff(sd, axis=-1))
        lo_ok = (t0[..., None, :] < td[..., None]) if mut == 'pool_lo' else (t0[..., None, :] <= td[..., None])
        hi_ok = (t1[..., None, :] >= td[..., None]) if mut == 'pool_hi' else (t1[..., None, :] > td[..., None])
        pd = np.max(np.where(lo_ok & hi_ok, p[..., None, :], f32(0)), -1)[..., :-1]
        wd = pd * np.diff(td, axis=-1)
        wd = wd / np.maximum(eps2, np.sum(wd, -1, keepdims=True))
        if mut != 'no_trim':
            td, wd = td[..., 1:-1], wd[..., 1:-1]
        t, w = td, wd
    else:
        t = sd
    with np.errstate(divide='ignore'):
        logits = np.where(t[..., 1:] > t[..., :-1], anneal * np.log(w + pad), f32(-np.inf)).astype(f32)
    sm = O.softmax(logits)
    if mut == 'inclusive_prefix':
        cw = np.concatenate([np.minimum(1, np.cumsum(sm, -1)), np.ones_like(sm[..., :1])], -1)
    else:
        cw = O.integrate_weights(sm)
    u = O.sample_u(t.shape[:-1], ns, jit, True, mut != 'no_pad', f32)
    centres = interp_twin(u, cw, t, mut == 'bracket_gt')
    out = R.intervals_of(centres)
    assert out.dtype == f32
    return out


def percentile_twin(tdist, w, t_far, strict=False):
    """float32 numpy twin of percentiles_kernel; strict: the bracket `cw < p` for `cw <= p`"""
    t = np.concatenate([tdist, t_far], -1).astype(f32)
    cw = O.integrate_weights(np.concatenate([w, np.zeros_like(w[:, :1])], -1).astype(f32))
    out = np.zeros((t.shape[0], 3), f32)
    for k, p in enumerate((0.05, 0.5, 0.95)):
        j = np.sum((cw < p) if strict else (cw <= p), -1, keepdims=True) - 1
        g = lambda a, jj: np.take_along_axis(a, jj, -1)[:, 0].astype(f64)
        c0, c1, t0, t1 = g(cw, j), g(cw, j + 1), g(t, j), g(t, j + 1)
        out[:, k] = ((t1 - t0) / (c1 - c0) * (p - c0) + t0).astype(f32)
    return out


def encode_twin(case, basis, **mut):
    """float32 numpy twin of the float32 path of cast_encode_kernel -> [rows, 504]"""
    with np.errstate(over='ignore', invalid='ignore'):
        lm, lv = R.encode_chain(*case, basis, dtype=f32, **mut)
        assert lm.dtype == f32 and lv.dtype == f32
        return R.encode_features(lm, lv, f32).reshape(-1, 504)


def encode_twin_bf16(case, basis):
    """the bf16 path: direct evaluation at the degrees 0, 2, 5, 8, angle doubling between (the twin of tests/test_layout_emulation.py
    on the float32 chain's lm / lv), rounded to bf16"""
    lm, lv = R.encode_chain(*case, basis, dtype=f32)
    lm, lv = lm.reshape(-1, 21), lv.reshape(-1, 21)
    out = np.zeros((lm.shape[0], 2, 12, 21), f32)
    sn = cs = dp = None
    with np.errstate(over='ignore', under='ignore'):
        for k in range(12):
            sc = f32(2 ** k)
            if k in (0, 2, 5, 8):
                x = lm * sc
                t = f32(314.15927)
                x = np.where(np.abs(x) >= t, x - np.floor(x / t) * t, x).astype(f32)
                n = np.rint(x * f32(0.15915494309189535)).astype(f32)
                r = (x.astype(f64) - n.astype(f64) * 6.2831854820251465).astype(f32)
                r = ((r.astype(f64) + n.astype(f64) * 1.7484556000744883e-7).astype(f32) * f32(0.15915494309189535)).astype(f32)
                sn, cs = np.sin(2 * np.pi * r.astype(f64)).astype(f32), np.cos(2 * np.pi * r.astype(f64)).astype(f32)
                dp = np.exp(-0.5 * (lv * sc * sc).astype(f64)).astype(f32)
            else:
                u = (sn + sn).astype(f32)
                s2 = (u * cs).astype(f32)
                cs = (1.0 - u.astype(f64) * sn.astype(f64)).astype(f32)
                sn = s2
                d2 = (dp * dp).astype(f32)
                dp = (d2 * d2).astype(f32)
            out[:, 0, k], out[:, 1, k] = dp * sn, dp * cs
    return R.round_bf16(out.reshape(-1, 504))


def dir_twin(v):
    return R.round_bf16(O.pos_enc(np.asarray(v, f32), 0, 4, append_identity=True).astype(f32))


# ------------------------------------------------------------------------------------------------------------ restatements
def test_step_function_is_the_oracle_where_the_float32_edges_are_exact():
    """dyadic edges k / 64 with the dyadic dilation 1 / 64: t -+ d is exact in either precision, so R.step_function (float32 edges) and
    the float64 oracle chain see the same edges and must agree to float64 roundoff; and without dilation for any edges"""
    rs = np.random.RandomState(0)
    sd = (np.sort(rs.randint(0, 65, (16, 41)), -1) / 64.0).astype(f32)
    sd[:, 0], sd[:, -1] = 0, 1
    w = O.softmax(rs.randn(16, 40) * 3).astype(f32)
    t, lg = R.step_function(sd, w, 1 / 64.0, R.ANNEAL, 1e-5)
    td, wd = O.max_dilate_weights(f64(sd), f64(w), 1 / 64.0, domain=(0., 1.), renormalize=True)
    td, wd = td[..., 1:-1], wd[..., 1:-1]
    with np.errstate(divide='ignore'):
        want = np.where(td[..., 1:] > td[..., :-1], f64(f32(R.ANNEAL)) * np.log(wd + f64(f32(1e-5))), -np.inf)
    assert np.array_equal(t, td)
    assert np.array_equal(np.isfinite(lg), np.isfinite(want))
    np.testing.assert_allclose(lg[np.isfinite(lg)], want[np.isfinite(want)], rtol=1e-12, atol=1e-12)
    t, lg = R.step_function(sd, w, 0.0, R.ANNEAL, 0.0)
    with np.errstate(divide='ignore'):
        want = np.where(np.diff(f64(sd)) > 0, f64(f32(R.ANNEAL)) * np.log(f64(w)), -np.inf)
    assert np.array_equal(t, f64(sd)) and np.array_equal(lg, want)


def test_envelope_holds_the_float64_samples_and_the_interval_rule():
    for c in R.resample_cases(65)[:8] + R.resample_cases(2)[:8]:
        b = R.resample_bounds(c['sd'], c['w'], c['dilation'], R.ANNEAL, c['padding'], c['ns'], c['jit'])
        assert (b['c_lo'] <= b['centres']).all() and (b['centres'] <= b['c_hi']).all()
        assert (b['lo'] <= b['want']).all() and (b['want'] <= b['hi']).all()
        # the float64 oracle on the same step function, u not rounded to float32: inside as well (the rounding of u is far below delta)
        o = O.sample_intervals(b['t'], b['logits'], c['ns'], c['jit'], True, domain=(0., 1.))
        assert (R.envelope_ratio(o, b['lo'], b['want'], b['hi']) <= 1).all()
        assert R.delta_cdf(b['nb']) == 2.0 ** -23 * (b['nb'] + 16)


def test_percentile_reference_is_the_oracle_and_the_twin_has_its_bits():
    for S in R.PCT_S:
        tdist, w, t_far = R.percentile_case(S, 37, 1e3)
        ref = O.volumetric_rendering(np.zeros((37, S, 3), f32), w, tdist, 1.0, t_far)
        want = R.percentile_reference(tdist, w, t_far)
        for j, k in enumerate(('distance_percentile_5', 'distance_median', 'distance_percentile_95')):
            assert np.array_equal(want[:, j], ref[k].astype(f32))
        assert np.array_equal(percentile_twin(tdist, w, t_far), want)


def test_encode_chain_is_the_oracle_chain():
    basis = O.pos_basis_t()
    for n, S in ((13, 1), (6, 32)):
        case = R.encode_case(n, S)
        ref = R.encode_reference(*case, basis)
        lm, lv = R.encode_chain(*case, basis)
        np.testing.assert_allclose(lm.reshape(-1, 21), ref['lm'], rtol=1e-13, atol=1e-13)
        np.testing.assert_allclose(lv.reshape(-1, 21), ref['lv'], rtol=1e-10, atol=1e-18)
        assert np.array_equal(R.encode_features(ref['lm'], ref['lv']), ref['want'])


def test_encode_bound_does_not_exceed_the_tolerance_it_replaces():
    """on the inputs of tests/test_gpu_mip360.py::test_cast_encode_matches_oracle every row is in R.in_todays_domain and the bound is
    everywhere at or below 2e-6 + 3e-6 2^k max(1, |lm|); the uncapped count is below it for 99 % of the elements"""
    case, basis = R.existing_encode_case(), O.pos_basis_t()
    ref = R.encode_reference(*case, basis)
    bound = R.encode_bound(ref, *R.encode_deltas(*case, basis), R.in_todays_domain(*case))
    assert R.in_todays_domain(*case).all()
    assert float((bound / R.existing_encode_bound(ref)).max()) <= 1.0
    raw = R.encode_bound(ref, *R.encode_deltas(*case, basis)) / R.existing_encode_bound(ref)
    print('cast_encode: uncapped count / replaced tolerance: median %.3f, above 1 for %.1f %% of the elements' % (np.median(raw), 100 * (raw > 1).mean()))
    assert (raw > 1).mean() < 0.02


# ------------------------------------------------------------------------------------------------------------ twins inside the bounds
@pytest.mark.parametrize('m', R.RESAMPLE_M)
def test_float32_resample_twin_is_inside_the_envelope(m):
    for c in R.resample_cases(m):
        b = R.resample_bounds(c['sd'], c['w'], c['dilation'], R.ANNEAL, c['padding'], c['ns'], c['jit'])
        with np.errstate(invalid='ignore'):
            got = resample_twin(c)
        r = R.envelope_ratio(got, b['lo'], b['want'], b['hi'])
        note('resample, off the domain ends', np.where((got > 0) & (got < 1), r, 0).max())  # (an edge clipped onto 0 or 1 sits ON its bound: ratio 1)
        assert note('resample', r.max()) <= 1.0, (c['m'], c['ns'], c['n'], c['dilation'], c['padding'], c['jitter'],
                                                  c['families'][int(np.argmax(r.max(-1)))], float(r.max()))
        assert (np.diff(got) >= 0).all() and got[:, 0].min() >= 0 and got[:, -1].max() <= 1


def test_float32_percentile_twin_is_inside_one_ulp():
    for S in R.PCT_S:
        for i, n in enumerate(R.PCT_N):
            for far in (1e3, 1e6):
                tdist, w, t_far = R.percentile_case(S, n, far, i)
                want = R.percentile_reference(tdist, w, t_far)
                assert note('distance_percentiles', R.err_ratio(percentile_twin(tdist, w, t_far), want, R.percentile_bound(want)).max()) <= 1.0


def test_float32_and_bf16_encode_twins_are_inside_the_bounds():
    basis = O.pos_basis_t()
    for n, S in R.ENCODE_ROWS + R.ENCODE_FM_ROWS:
        for seed in (0, 1):
            case = R.encode_case(n, S, seed)
            ref = R.encode_reference(*case, basis)
            b32 = R.encode_bound(ref, *R.encode_deltas(*case, basis), R.in_todays_domain(*case))
            assert np.isfinite(ref['want']).all() and np.isfinite(b32).all()
            r = R.err_ratio(encode_twin(case, basis), ref['want'], b32)
            assert note('cast_encode float32', r.max()) <= 1.0, (n, S, seed, np.unravel_index(int(np.argmax(r)), r.shape))
            r = R.err_ratio(encode_twin_bf16(case, basis), ref['want'], R.encode_bound_bf16(ref, b32))
            assert note('cast_encode bf16', r.max()) <= 1.0, (n, S, seed, np.unravel_index(int(np.argmax(r)), r.shape))


def test_dir_twin_is_inside_the_bound():
    for n, _ in R.DIR_SHAPES:
        v = R.dir_case(n)
        want = R.dir_reference(v)
        assert np.array_equal(want, O.pos_enc(f64(v), 0, 4, append_identity=True)) and want.shape == (n, 27)
        assert note('dir_encode', R.err_ratio(dir_twin(v), want, R.dir_bound(want)).max()) <= 1.0


# ------------------------------------------------------------------------------------------------------------ mutants
def _resample_rejected(mut, cases):
    worst = 0.0
    for c in cases:
        b = R.resample_bounds(c['sd'], c['w'], c['dilation'], R.ANNEAL, c['padding'], c['ns'], c['jit'])
        with np.errstate(invalid='ignore'):
            got = resample_twin(c, mut)
        if got.shape != b['lo'].shape:
            return np.inf
        worst = max(worst, float(R.envelope_ratio(got, b['lo'], b['want'], b['hi']).max()))
    return worst


@pytest.mark.parametrize('mut', RESAMPLE_MUTANTS)
def test_resample_mutants_are_rejected(mut):
    cases = [c for m in (2, 65) for c in R.resample_cases(m) if c['n'] == 37]
    if mut in ('no_trim', 'pool_lo', 'pool_hi'):
        cases = [c for c in cases if c['dilation'] > 0]
    if mut == 'no_pad':
        cases = [c for c in cases if c['jitter'] == 'none']
    if mut == 'bracket_gt':                                  # only a u that equals a cdf value sees the difference: jitter 0 puts u_0 = 0
        cases = [c for c in cases if c['jitter'] == 'zero' and c['padding'] == 0]
    assert cases
    assert _resample_rejected(mut, cases) > 1.0


def test_rank_sort_tie_order_and_clip_before_sort_change_no_value():
    """Two mutants that cannot be told apart, pinned as such.  Equal values sort to equal values whichever comes first.  The clip is
    monotone, so it commutes with the sort; and a support [t0, t1) clipped to the domain covers the same edges td in [0, 1) as the
    unclipped one -- the two differ at td = 1 only, where every bin has zero width and weight 0 either way."""
    for c in [c for m in (2, 64, 128) for c in R.resample_cases(m) if c['dilation'] > 0 and c['n'] == 37][::3]:
        with np.errstate(invalid='ignore'):
            base, ranked, other, clipped = resample_twin(c), resample_twin(c, 'rank'), resample_twin(c, 'tie_other'), resample_twin(c, 'clip_first')
        assert np.array_equal(base, ranked) and np.array_equal(base, other) and np.array_equal(base, clipped)
        b = R.resample_bounds(c['sd'], c['w'], c['dilation'], R.ANNEAL, c['padding'], c['ns'], c['jit'])
        assert R.envelope_ratio(other, b['lo'], b['want'], b['hi']).max() <= 1.0


def test_percentile_bracket_mutant_is_rejected():
    tdist, w, t_far = R.percentile_case(32, 37, 1e3)
    want = R.percentile_reference(tdist, w, t_far)
    r = R.err_ratio(percentile_twin(tdist, w, t_far, strict=True), want, R.percentile_bound(want))
    fam = np.array([R.PCT_FAMILIES[i % 6] for i in range(37)])
    assert r[fam == 'half_then_zeros'].max() > 1.0                # the tied cdf values at 0.5: the first tied edge instead of the last


@pytest.mark.parametrize('mut', [dict(floor=False), dict(diag=True), dict(rank_one=False)])
def test_encode_mutants_are_rejected(mut):
    """without the eps floor of denom an interval [0, 0] divides 0 by 0 and an interval [0, 2e-4] moves t_mean by 3e-5; the diagonal
    covariance and the Jacobian without its rank-one term change the variance of every sample off the axes / outside the unit ball"""
    basis = O.pos_basis_t()
    case = list(R.encode_case(12, 1))
    if 'floor' in mut:
        case[0] = case[0].copy()
        case[0][0], case[0][1] = (0.0, 0.0), (0.0, 2e-4)
    ref = R.encode_reference(*case, basis)
    b32 = R.encode_bound(ref, *R.encode_deltas(*case, basis), R.in_todays_domain(*case))
    assert R.err_ratio(encode_twin(case, basis), ref['want'], b32).max() <= 1.0
    assert R.err_ratio(encode_twin(case, basis, **mut), ref['want'], b32).max() > 1.0


def test_zz_report_worst_ratios():
    """the worst ratio per kernel of the float32 twins (DESIGN.md quotes them)"""
    for k in sorted(WORST):
        print('float32 twin, worst ratio  %-24s %.3f' % (k, WORST[k]))
    assert all(v <= 1.0 for v in WORST.values())

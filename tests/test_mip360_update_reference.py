"""CPU checks of tests/mip360_update_reference.py, the restatements and bounds tests/test_gpu_mip360_update.py holds the MipNeRF-360
parameter-update kernels to:
  * the float64 restatements are the oracle: tree_norm, and clip -> nan_to_num -> Adam of oracle.mip360_oracle.apply_gradients over
    several steps (exact-constant variant), to float64 rounding;
  * a float32 numpy twin of every kernel, in the kernel's written order, stays inside its bound on every input family the GPU test
    uses (a bound a correct float32 implementation misses is wrong; one it fills to less than 1 % tests nothing) -- the worst ratio
    per kernel is printed (pytest -s);
  * nine mutated twins are rejected on the same inputs, so that no bound can loosen quietly;
  * the documented distance between the kernel's float constants and optax's double ones is what the module says."""
import numpy as np
import pytest

from oracle import mip360_oracle as O
from tests import mip360_update_reference as R

f32 = np.float32
LR = 2e-3


def _report(name, worst, lo=0.01):
    print('worst ratio %-28s %.3f' % (name, worst))
    assert worst <= 1.0, (name, worst, 'a correct float32 evaluation misses the bound: the derivation is wrong')
    assert worst >= lo, (name, worst, 'the bound is too loose to test anything')


# ------------------------------------------------------------------------------------------------------------ float32 twins
def twin_sum_squares(g, n_blocks, aligned=True):
    """sumsq_partial_kernel: a block's partial in double (16-byte path: float4 i belongs to block (i / 1024) % n_blocks, the tail and
    the 4-byte path element-wise), cast to float"""
    n = g.size
    n4 = n // 4 if aligned else 0
    sq = g.astype(np.float64) ** 2
    part = np.zeros(n_blocks)
    if n4:
        part += np.bincount((np.arange(4 * n4) // 4 // 1024) % n_blocks, sq[:4 * n4], n_blocks)
    if n > 4 * n4:
        part += np.bincount((np.arange(n - 4 * n4) // 1024) % n_blocks, sq[4 * n4:], n_blocks)
    with np.errstate(over='ignore', invalid='ignore'):
        return part.astype(f32)


def twin_clip(partials, max_norm):
    """clip_mult_kernel: (mult, norm)"""
    with np.errstate(over='ignore', invalid='ignore'):
        norm = f32(np.sqrt(partials.astype(np.float64).sum()))
        mx = f32(max_norm)
        ratio = mx / (f32(2.0 ** -23) + norm)
        mult = (ratio if ratio != ratio else min(f32(1), ratio)) if mx > 0 else f32(1)
    return f32(mult), norm


def twin_adam(p, g, m, v, mult, step, lr, b1=0.9, b2=0.999, eps=1e-6, mutation=None):
    """adam_kernel in float32, operation by operation"""
    lr, b1, b2, eps = f32(lr), f32(b1), f32(b2), f32(eps)
    s = step - 1 if mutation == 'bias_step' else step
    bc1, bc2 = f32(1.0 - 0.9 ** s), f32(1.0 - 0.999 ** s)
    one, fmax = f32(1), np.finfo(f32).max
    mu_ = f32(1) if mult is None else f32(mult)
    with np.errstate(all='ignore'):
        gi = g if mutation == 'mult_late' else g * mu_
        gi = np.where(gi != gi, f32(0), gi)
        gi = np.clip(gi, -fmax, fmax)
        if mutation == 'mult_late':
            gi = gi * mu_
        w_old, w_new = (one - b2, b2) if mutation == 'swap_b2' else (b2, one - b2)
        mi = b1 * m + (one - b1) * gi
        vi = w_old * v + w_new * gi * gi
        root = np.sqrt(vi / bc2 + eps) if mutation == 'eps_inside' else np.sqrt(vi / bc2) + eps
        pn = p - lr * (mi / bc1) / root
    assert pn.dtype == f32 and mi.dtype == f32 and vi.dtype == f32
    return pn, mi, vi


def twin_slab_sum(slabs, scale, mutation=None):
    """slab_sum_kernel / slab_sum2_kernel: group g adds s = g, g + 4, ...; groups added in order; times scale"""
    ksplit, n = slabs.shape
    last = ksplit - 1 if (mutation == 'drop_last' and ksplit % 16 == 13) else ksplit
    part = np.zeros((4, n), f32)
    for s in range(last):
        part[s % 4] += slabs[s]
    r = ((part[0] + part[1]) + part[2]) + part[3]
    out = r if mutation == 'no_scale' else r * f32(scale)
    if mutation == 'skip_tail' and n % 4:
        out[n - n % 4:] = 0
    return out


def twin_col_sum(dz, nslice, scale=1.0):
    """col_sum_kernel (a slice's rows one after the other; an empty slice gives 0) + slab_sum_kernel"""
    m, n_out = dz.shape
    per = -(-m // nslice)
    part = np.zeros((nslice, n_out), f32)
    for s in range(nslice):
        for r in range(s * per, min(m, (s + 1) * per)):
            part[s] += dz[r]
    return twin_slab_sum(part, scale)


def twin_head_backward(density, g_d, rgb, g_c, pad=0.001, mutation=None):
    with np.errstate(all='ignore'):
        e = np.exp(-density)
        assert e.dtype == f32
        raw = g_d * (e if mutation == 'exp_only' else f32(1) - e)
        pad = f32(pad)
        s = (rgb + pad) / (f32(1) + f32(2) * pad)
        pre = g_c * (f32(1) + f32(2) * pad) * s * (f32(1) - s)
    return R.round_bf16(raw), R.round_bf16(pre)


def twin_pack(kernel, mutation=None):
    if mutation == 'truncate':
        return (kernel.view(np.uint32) & np.uint32(0xFFFF0000)).view(f32)
    return R.round_bf16(kernel)


# ------------------------------------------------------------------------------------------------------------ the oracle
def test_restatements_are_the_oracle_over_several_steps():
    """tree_norm, the clip lines and Adam of oracle.mip360_oracle.apply_gradients against norm_reference / clip_reference /
    adam_reference with exact constants, chained over six steps from step 1 and from step 600 (past lr_delay_steps); one step has a NaN
    gradient, one a +inf (multiplier NaN / 0: nan_to_num after the product)."""
    rs = np.random.RandomState(0)
    shapes = {'prop': [(5, 3), (3, 1)], 'nerf': [(7, 4), (4, 2), (2, 3)]}
    mk = lambda scale: {k: [(rs.randn(*s) * scale, rs.randn(s[1]) * scale) for s in v] for k, v in shapes.items()}
    for start in (0, 599):
        params = mk(1.0)
        state = O.new_train_state(params['prop'], params['nerf'])
        state['count'] = start
        mine = {k: [[a.copy() for a in (x, np.zeros_like(x), np.zeros_like(x))] for pair in params[k] for x in pair] for k in shapes}
        for i in range(6):
            grads = mk(10.0 ** (-3 * (i % 3)))
            if i == 2:
                grads['prop'][0][0][1, 1] = np.nan
            if i == 4:
                grads['nerf'][1][1][0] = np.inf
            step = state['count'] + 1
            lr = O.learning_rate_decay(state['count'], 2e-3, 2e-5, 1000, 512, 0.01)
            norms = {k: O.tree_norm(grads[k]) for k in shapes}
            with np.errstate(invalid='ignore'):
                mults = O.apply_gradients(state, grads, max_steps=1000)
            c = R.adam_constants(step, lr, exact=True)
            for k in shapes:
                flat = [x for pair in grads[k] for x in pair]
                norm = R.norm_reference(flat)
                np.testing.assert_allclose(norm, norms[k], rtol=4 * np.finfo(np.float64).eps, atol=0, equal_nan=True)
                mult = R.clip_reference(norm, 0.001)
                np.testing.assert_allclose(mult, mults[k], rtol=2 * R.U, atol=0, equal_nan=True)       # (float)0.001 against 0.001
                assert np.isnan(mult) == (i == 2 and k == 'prop') and (mult == 0) == (i == 4 and k == 'nerf')
                want = [x for pair in state[k] for x in pair]
                want_m = [x for pair in state['mu'][k] for x in pair]
                want_v = [x for pair in state['nu'][k] for x in pair]
                for t, gt in enumerate(flat):
                    pn, mn, vn = R.adam_reference(mine[k][t][0], gt, mine[k][t][1], mine[k][t][2], mults[k], c)
                    mine[k][t] = [pn, mn, vn]
                    for a, b in ((pn, want[t]), (mn, want_m[t]), (vn, want_v[t])):
                        assert np.isfinite(a).all()
                        np.testing.assert_allclose(a, b, rtol=1e-14, atol=1e-300)


def test_documented_distance_between_float_and_double_constants():
    """The module docstring's arithmetic: 1 - (float)0.999 is 1.2875e-5 below 0.001, and at step 1 with sqrt(v_hat) >> eps the update of
    the float constants is 6.7e-6 above optax's."""
    c, ce = R.adam_constants(1, LR), R.adam_constants(1, LR, exact=True)
    assert abs((ce['omb2'] - c['omb2']) / ce['omb2'] - 1.2875e-5) < 1e-8
    assert abs((c['omb1'] - ce['omb1']) / ce['omb1'] - 2.384e-7) < 1e-9
    p, g, m, v = R.adam_case(np.random.RandomState(1), 1001, 1, 1.0)
    keep = g != 0
    up = lambda cc: (R.f64(p) - R.adam_reference(R.f64(p), R.f64(g), R.f64(m), R.f64(v), None, cc)[0])[keep]
    rel = up(c) / up(ce) - 1
    assert np.all(np.abs(rel - R.ADAM_STEP1_DISTANCE) < 0.1e-6), (rel.min(), rel.max())
    # ... and constant_distance carries exactly that much: the exact-constant reference is inside adam_bounds around the other
    d = R.constant_distance(c, ce)
    assert d['rel_v'] / 2 + d['rel_m'] + d['rel_u'] < 1.1 * R.ADAM_STEP1_DISTANCE


# ------------------------------------------------------------------------------------------------------------ norm and clip
def _norm_inputs():
    for n in R.NORM_SIZES:
        for scale in R.NORM_SCALES:
            rs = np.random.RandomState(n % 1000 + int(-np.log10(scale)) + 50)
            yield n, scale, (rs.randn(n) * scale).astype(f32)


def test_norm_and_clip_twin_inside_bounds():
    worst_n = worst_c = 0.0
    for n, scale, g in _norm_inputs():
        norm = R.norm_reference([g])
        for nb in R.NORM_BLOCKS:
            for aligned in (True, False):
                for max_norm in (0.001, 1e3):
                    mult, got = twin_clip(twin_sum_squares(g, nb, aligned), max_norm)
                    worst_n = max(worst_n, R.ratio(got, norm, R.norm_bound(norm, nb)).max())
                    want = R.clip_reference(norm, max_norm)
                    if scale == 1e-20:
                        assert mult == 1 and want == 1
                    worst_c = max(worst_c, R.ratio(mult, want, R.clip_bound(norm, max_norm, nb)).max())
    _report('sum_squares (norm)', worst_n)
    _report('clip_multiplier', worst_c)
    # non-finite and switched off
    g = np.ones(9, f32)
    g[4] = np.nan
    mult, norm = twin_clip(twin_sum_squares(g, 7), 0.001)
    assert np.isnan(mult) and np.isnan(norm) and np.isnan(R.clip_reference(R.norm_reference([g]), 0.001))
    g[4] = np.inf
    mult, norm = twin_clip(twin_sum_squares(g, 7), 0.001)
    assert mult == 0 and norm == np.inf and R.clip_reference(R.norm_reference([g]), 0.001) == 0
    assert twin_clip(twin_sum_squares(np.ones(9, f32), 7), 0.0)[0] == 1 and R.clip_reference(3.0, 0.0) == 1 and R.clip_bound(3.0, 0.0, 7) == 0


# ------------------------------------------------------------------------------------------------------------ Adam
def _adam_inputs():
    for n in R.ADAM_SIZES:
        for step in R.ADAM_STEPS:
            for scale in R.ADAM_SCALES:
                for mult in (0.37, None):
                    rs = np.random.RandomState((n + 31 * step) % 100000 + int(-np.log10(scale)))
                    yield step, mult, R.adam_case(rs, n, step, scale)


def _adam_ratios(got, p, g, m, v, mult, c, **kw):
    a64 = [R.f64(x) for x in (p, g, m, v)]
    want = R.adam_reference(*a64, None if mult is None else float(f32(mult)), c)
    b = R.adam_bounds(*a64, None if mult is None else float(f32(mult)), c, **kw)
    return [R.ratio(got[i], want[i], b[k]).max() for i, k in enumerate(('p', 'mu', 'nu'))]


def test_adam_twin_inside_bounds():
    worst = np.zeros(3)
    for step, mult, (p, g, m, v) in _adam_inputs():
        got = twin_adam(p, g, m, v, mult, step, LR)
        worst = np.maximum(worst, _adam_ratios(got, p, g, m, v, mult, R.adam_constants(step, LR)))
    for name, w in zip(('adam p', 'adam mu', 'adam nu'), worst):
        _report(name, w)


@pytest.mark.parametrize('bad', ['nan', 'inf', '-inf'])
@pytest.mark.parametrize('mult', [np.nan, 0.0])
def test_adam_non_finite_gradient_decays_the_moments(bad, mult):
    p, g, m, v = R.adam_case(np.random.RandomState(3), 257, 10, 1e-3)
    g[5] = float(bad)
    c = R.adam_constants(10, LR)
    got = twin_adam(p, g, m, v, mult, 10, LR)
    want = R.adam_reference(R.f64(p), R.f64(g), R.f64(m), R.f64(v), mult, c)
    assert all(np.isfinite(x).all() for x in got + want)
    np.testing.assert_array_equal(want[1], c['b1'] * R.f64(m))
    np.testing.assert_array_equal(want[2], c['b2'] * R.f64(v))
    assert max(_adam_ratios(got, p, g, m, v, mult, c)) <= 1


@pytest.mark.parametrize('mutation', ['eps_inside', 'bias_step', 'swap_b2'])
def test_adam_mutations_are_rejected(mutation):
    """on the inputs of test_adam_twin_inside_bounds; the bias corrections of step - 1 are those of `step` in float32 from step 513 for
    b1 and at step 100 000 for both, and infinite at step 1 -- they must be caught at steps 2, 10 and 513"""
    caught = set()
    for step, mult, (p, g, m, v) in _adam_inputs():
        if mutation == 'bias_step' and step == 1:
            continue
        got = twin_adam(p, g, m, v, mult, step, LR, mutation=mutation)
        if _adam_ratios(got, p, g, m, v, mult, R.adam_constants(step, LR))[0] > 1:
            caught.add(step)
    assert caught >= ({2, 10, 513} if mutation == 'bias_step' else set(R.ADAM_STEPS)), caught


def test_adam_multiplier_after_nan_to_num_is_rejected():
    p, g, m, v = R.adam_case(np.random.RandomState(3), 257, 10, 1e-3)
    g[5] = np.inf
    got = twin_adam(p, g, m, v, np.nan, 10, LR, mutation='mult_late')
    assert max(_adam_ratios(got, p, g, m, v, np.nan, R.adam_constants(10, LR))) > 1


@pytest.mark.parametrize('start', [1, 600])
def test_adam_chain_that_is_never_restarted(start):
    """20 float32 steps against 20 float64 steps with optax's constants, never restarted: adam_bounds with the errors of the step before
    handed on (m_err, v_rel, p_err) and the constants' distance (constant_distance) -- what the GPU test's trainer link asserts."""
    rs = np.random.RandomState(start)
    n = 4001
    p, _, m, v = R.adam_case(rs, n, 1, 1.0)
    p64, m64, v64 = R.f64(p), R.f64(m), R.f64(v)
    err = dict(m_err=0.0, v_rel=0.0, p_err=0.0)
    worst = np.zeros(3)
    for i in range(20):
        step = start + i
        g = (rs.randn(n) * 3e-7 * 10.0 ** rs.uniform(-1, 1, n)).astype(f32)
        lr = O.learning_rate_decay(step - 1, 2e-3, 2e-5, 1000, 512, 0.01)
        c, ce = R.adam_constants(step, lr), R.adam_constants(step, lr, exact=True)
        p, m, v = twin_adam(p, g, m, v, 0.37, step, lr)
        b = R.adam_bounds(p64, R.f64(g), m64, v64, float(f32(0.37)), ce, **R.constant_distance(ce, c), **err)
        p64, m64, v64 = R.adam_reference(p64, R.f64(g), m64, v64, float(f32(0.37)), ce)
        err = dict(m_err=b['mu'], v_rel=b['v_rel'], p_err=b['p'])
        worst = np.maximum(worst, [R.ratio(a, w, b[k]).max() for a, w, k in ((p, p64, 'p'), (m, m64, 'mu'), (v, v64, 'nu'))])
    print('worst ratio of the free chain (p, mu, nu) from step %d: %s' % (start, worst))
    assert (worst <= 1).all()


# ------------------------------------------------------------------------------------------------------------ slab and column sums
def _slab_inputs():
    for ksplit in R.SLAB_KSPLITS + (255,):
        for family in ('random', 'cancelling'):
            for n in (15, 48, 257):
                yield R.slab_case(np.random.RandomState(ksplit * 7 + n), family, ksplit, n)


def test_slab_sum_twin_inside_bounds():
    worst = 0.0
    for slabs in _slab_inputs():
        for scale in R.SLAB_SCALES:
            worst = max(worst, R.ratio(twin_slab_sum(slabs, scale), R.slab_sum_reference(slabs, scale), R.slab_sum_bound(slabs, scale)).max())
    _report('slab_sum', worst)


@pytest.mark.parametrize('mutation', ['drop_last', 'skip_tail', 'no_scale'])
def test_slab_sum_mutations_are_rejected(mutation):
    caught = 0
    for slabs in _slab_inputs():
        for scale in R.SLAB_SCALES:
            bad = R.ratio(twin_slab_sum(slabs, scale, mutation), R.slab_sum_reference(slabs, scale), R.slab_sum_bound(slabs, scale)).max() > 1
            applies = {'drop_last': slabs.shape[0] % 16 == 13, 'skip_tail': slabs.shape[1] % 4 != 0, 'no_scale': scale != 1}[mutation]
            assert bad == applies, (mutation, slabs.shape, scale)
            caught += bad
    assert caught


def col_sum_case(rs, family, m, n_out):
    """bfloat16 values.  'random'; 'staircase': a first row of 256 and then rows of 1.5 * 2^-16, each of which float32 rounds up to a whole
    spacing of 256 -- every addition errs in the same direction, which is what the bound's row count is for."""
    if family == 'random':
        return R.round_bf16(rs.randn(m, n_out).astype(f32))
    dz = np.full((m, n_out), 1.5 * 2.0 ** -16, f32)
    dz[0] = 256
    return dz * np.where(np.arange(n_out) % 2, f32(-1), f32(1))


def test_col_sum_twin_inside_bounds():
    worst = 0.0
    for m in (1, 255, 256, 1000):
        for n_out in (1, 3):
            for nslice in (1, 3, 4, 5):
                for family in ('random', 'staircase'):
                    dz = col_sum_case(np.random.RandomState(m + nslice), family, m, n_out)
                    worst = max(worst, R.ratio(twin_col_sum(dz, nslice), R.col_sum_reference(dz), R.col_sum_bound(dz, nslice)).max())
    dz = col_sum_case(np.random.RandomState(0), 'random', 3, 2)
    np.testing.assert_array_equal(twin_col_sum(dz, 5), twin_col_sum(dz, 3))                  # nslice > m: empty slices add 0
    _report('col_sum', worst)


# ------------------------------------------------------------------------------------------------------------ head backward
def test_head_backward_twin_inside_bounds_and_mutation_rejected():
    worst = np.zeros(2)
    for rows in (1, 255, 256, 257, 4099, 200000):
        case = R.head_case(np.random.RandomState(rows), rows)
        want = R.head_backward_reference(*case)
        bound = R.head_backward_bounds(*case)
        got = twin_head_backward(*case)
        worst = np.maximum(worst, [R.ratio(got[i], want[i], bound[i]).max() for i in range(2)])
        if rows >= 255:
            bad = twin_head_backward(*case, mutation='exp_only')
            assert R.ratio(bad[0], want[0], bound[0]).max() > 1
            d = case[0]
            assert (d == 0).any() and ((d > 0) & (d < 1e-5)).any() and (d >= 88).any()
    _report('head_backward d_raw', worst[0])
    _report('head_backward d_pre', worst[1])
    assert worst.max() > 0.9                                   # the half-spacing term of the bfloat16 rounding is tight by construction


# ------------------------------------------------------------------------------------------------------------ packing
def test_pack_reference_rounds_to_even_and_truncation_is_rejected():
    k = R.pack_case(np.random.RandomState(0), 283, 128)
    low = k.view(np.uint32) & np.uint32(0xFFFF)
    kept_odd = (k.view(np.uint32) >> np.uint32(16)) & np.uint32(1)
    assert ((low == 0x8000) & (kept_odd == 0)).mean() > 0.2 and ((low == 0x8000) & (kept_odd == 1)).mean() > 0.2
    assert (np.abs(k) < R.TINY).mean() > 0.03
    q = twin_pack(k)
    np.testing.assert_array_equal(q[(low == 0x8000) & (kept_odd == 0)], twin_pack(k, 'truncate')[(low == 0x8000) & (kept_odd == 0)])
    assert (np.abs(R.f64(q) - R.f64(k)) <= np.abs(R.f64(twin_pack(k, 'truncate')) - R.f64(k))).all()
    assert (q != twin_pack(k, 'truncate')).any()
    n_in, n_out, ld_f, ld_b, ld_ff, ld_bf, rows, col0 = 283, 128, 288, 130, 288, 144, 200, 16
    dst = [np.full(s, 7.0, f32) for s in (n_out * ld_f, n_in * ld_b, 128 * ld_ff, 224 * ld_bf)]
    fwd, bwd, fwd_fm, bwd_fm = R.pack_reference(k, dst[0], ld_f, dst[1], ld_b, dst[2], ld_ff, dst[3], ld_bf, rows, col0)
    np.testing.assert_array_equal(fwd.reshape(n_out, ld_f)[:, :n_in], q.T)
    np.testing.assert_array_equal(bwd.reshape(n_in, ld_b)[:, :n_out], q)
    assert (fwd.reshape(n_out, ld_f)[:, n_in:] == 7).all() and (bwd.reshape(n_in, ld_b)[:, n_out:] == 7).all()
    assert (fwd_fm != 7).sum() + (q == 7).sum() == q.size and (bwd_fm != 7).sum() == (q[:rows] != 7).sum()
    rr, cc = np.meshgrid(np.arange(rows), np.arange(n_out), indexing='ij')
    np.testing.assert_array_equal(bwd_fm[R.fm_index(rr, cc + col0, ld_bf)], q[:rows])

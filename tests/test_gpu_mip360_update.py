"""GPU tests of the parameter-update kernels of the MipNeRF-360 trainer (csrc/mip360_train.hip), one by one through the C ABI, against
the float64 restatements of tests/mip360_update_reference.py (R) and inside the bounds that module derives from the inputs:

* mip360_sum_squares + mip360_clip_multiplier: sizes around the 16-byte path's tail, 1 / 7 / 256 blocks, gradient scales from
  underflow to 1e15, a 4-byte aligned view (the scalar path), NaN / inf, max_norm = 0, two tensors' partials back to back;
* mip360_adam_step: mu, nu and the parameter at steps 1 ... 100 000, gradients from 1e-12 to 1 (3e-7 is where sqrt(v_hat) ~ eps and
  training sits), cancelling moments, multiplier by pointer and null, non-finite gradients, nothing written past n;
* Mip360Trainer._apply_one: 20 steps on either MLP from step 1 and from step 600, every step against the float64 chain restarted from
  the device state, and the 20th against a chain that never was (optax's double constants: the documented distance);
* mip360_grad_weight_reduce / mip360_grad_bias_bf16: every loop boundary of ksplit, scalar path with a tail, rows < n_in, ldg > n_out,
  scale, with and without the bias, run-to-run and vector-path against scalar-path bits;
* mip360_grad_weight_bf16 with one output column: slices long enough for the 16-rows-in-flight body;
* mip360_head_backward: saturating and vanishing density, both ends of the colour range, the exact extent of the zero fill;
* mip360_pack_weight / _fm / mip360_pack_weights_fm_batch: ties of both parities, subnormals, padding untouched, 16 descriptors of very
  different sizes with null destinations, and TrainableMLP.repack(lazy=True) + ensure_rm().

Every tolerance below is a bound function of R; the worst |error| / bound per kernel is printed (pytest -s) and collected by the last test."""
import ctypes as C

import numpy as np
import pytest

torch = pytest.importorskip('torch')
pytestmark = pytest.mark.gpu

from oracle import mip360_oracle as O                                    # noqa: E402
from tests import mip360_update_reference as R                           # noqa: E402
from tests.test_gpu_mip360 import T, N, dev                              # noqa: E402

f32 = np.float32
LR = 2e-3
SENTINEL = 7.0
WORST = {}


@pytest.fixture(scope='module')
def M():
    dev()
    from outdoor_nerf_depth_amd import mip360
    return mip360


def call(M, name, *args):
    M._check(getattr(M.lib(), name)(M._stream(), *args), name)


def note(name, value):
    value = float(value)
    WORST[name] = max(WORST.get(name, 0.0), value)
    return value


def inside(name, got, want, bound):
    """every element within its bound; records the worst ratio"""
    r = R.ratio(got, want, bound)
    worst = note(name, r.max())
    assert worst <= 1.0, (name, worst, int(np.argmax(r)), np.ravel(R.f64(got))[np.argmax(r)], np.ravel(R.f64(want))[np.argmax(r)])


def guarded(values, dtype=torch.float32, guard=16, lead=0):
    """a device buffer [lead sentinels | values | guard sentinels]; returns (whole buffer, the view of the values)"""
    values = np.ascontiguousarray(values)
    buf = torch.full((lead + values.size + guard,), SENTINEL, dtype=dtype, device=dev())
    view = buf[lead:lead + values.size]
    view.copy_(torch.from_numpy(values.reshape(-1)).to(dtype))
    return buf, view


def untouched(buf, lead, n):
    return bool((buf[:lead] == SENTINEL).all()) and bool((buf[lead + n:] == SENTINEL).all())


def bits(t):
    """the 16-bit patterns of a bfloat16 device tensor / of bfloat16 values held in a float32 host array"""
    if isinstance(t, np.ndarray):
        return (np.ascontiguousarray(t, f32).view(np.uint32) >> np.uint32(16)).astype(np.uint16)
    return t.contiguous().view(torch.int16).cpu().numpy().view(np.uint16)


# ------------------------------------------------------------------------------------------------------------ norm and clip
def _norm(M, g, n_blocks, max_norm, partial=None):
    partial = torch.full((n_blocks + 8,), SENTINEL, device=dev()) if partial is None else partial
    out = torch.full((4,), SENTINEL, device=dev())
    call(M, 'mip360_sum_squares', g.numel(), M._p(g), M._p(partial), n_blocks)
    call(M, 'mip360_clip_multiplier', n_blocks, M._p(partial), max_norm, M._p(out))
    assert bool((partial[n_blocks:] == SENTINEL).all()) and bool((out[2:] == SENTINEL).all())
    mult, norm = N(out[:2])
    return mult, norm


@pytest.mark.parametrize('n_blocks', R.NORM_BLOCKS)
@pytest.mark.parametrize('n', R.NORM_SIZES)
def test_norm_and_clip_against_float64(M, n, n_blocks):
    """R.norm_bound / R.clip_bound.  At scale 1e-20 a block's float partial is below the normal range: the norm may come back as 0 (the
    bound's flush term says so) and the multiplier is exactly 1; at 1e15 it is far below 1.  The view one float into the allocation is
    4-byte aligned only and takes the kernel's scalar path."""
    for scale in R.NORM_SCALES:
        host = (np.random.RandomState(n % 1000 + n_blocks).randn(n) * scale).astype(f32)
        norm = R.norm_reference([host])
        for lead in (0, 1):
            _, g = guarded(host, lead=lead, guard=3)
            assert g.data_ptr() % 16 == 4 * lead
            for max_norm in (0.001, 1e3):
                mult, got = _norm(M, g, n_blocks, max_norm)
                inside('sum_squares', got, norm, R.norm_bound(norm, n_blocks))
                inside('clip_multiplier', mult, R.clip_reference(norm, max_norm), R.clip_bound(norm, max_norm, n_blocks))
                if scale == 1e-20:
                    assert mult == 1
                if scale == 1e15 and max_norm == 0.001:
                    assert mult < R.U                                   # far below 1: under one float32 roundoff


def test_norm_and_clip_non_finite_switched_off_and_two_tensors(M):
    host = np.random.RandomState(0).randn(4097).astype(f32)
    bad = host.copy()
    bad[1234] = np.nan
    mult, norm = _norm(M, T(bad), 7, 0.001)
    assert np.isnan(mult) and np.isnan(norm)                              # jnp.minimum propagates the NaN
    bad[1234] = np.inf
    mult, norm = _norm(M, T(bad), 7, 0.001)
    assert mult == 0 and norm == np.inf
    want = R.norm_reference([host])
    mult, norm = _norm(M, T(host), 7, 0.0)                                # clipping off: multiplier 1, the norm still reported
    assert mult == 1
    inside('sum_squares', norm, want, R.norm_bound(want, 7))
    # two tensors' partials back to back, 256 each: the layout of the per-image embeddings' clip
    a, b = (np.random.RandomState(1).randn(70001) * 1e-3).astype(f32), (np.random.RandomState(2).randn(37) * 10).astype(f32)
    partial = torch.full((512 + 8,), SENTINEL, device=dev())
    ta, tb = T(a), T(b)
    call(M, 'mip360_sum_squares', a.size, M._p(ta), M._p(partial), 256)
    call(M, 'mip360_sum_squares', b.size, M._p(tb), M._p(partial[256:]), 256)
    out = torch.full((4,), SENTINEL, device=dev())
    call(M, 'mip360_clip_multiplier', 512, M._p(partial), 0.001, M._p(out))
    want = R.norm_reference([np.concatenate([a, b])])
    inside('sum_squares', N(out)[1], want, R.norm_bound(want, 512))
    inside('clip_multiplier', N(out)[0], R.clip_reference(want, 0.001), R.clip_bound(want, 0.001, 512))
    assert bool((partial[512:] == SENTINEL).all()) and bool((out[2:] == SENTINEL).all())


# ------------------------------------------------------------------------------------------------------------ Adam
def _adam(M, p, g, m, v, mult, step, lr=LR):
    """one mip360_adam_step on guarded copies; mult: None (null pointer) or a float handed over by pointer.  Returns the float32 results
    and the multiplier as the kernel read it."""
    n = p.size
    bufs = [guarded(x) for x in (p, g, m, v)]
    tm_ = None if mult is None else torch.tensor([mult], dtype=torch.float32, device=dev())
    call(M, 'mip360_adam_step', n, M._p(bufs[0][1]), M._p(bufs[1][1]), M._p(bufs[2][1]), M._p(bufs[3][1]), M._p(tm_), step, lr, 0.9, 0.999, 1e-6)
    assert all(untouched(b, 0, n) for b, _ in bufs), 'written past n'
    np.testing.assert_array_equal(N(bufs[1][1]).view(np.uint32), np.ascontiguousarray(g).view(np.uint32))         # the gradient is read only
    return [N(bufs[i][1]) for i in (0, 2, 3)], (None if mult is None else float(N(tm_)[0]))


def _adam_check(got, p, g, m, v, mult, step, lr=LR):
    c = R.adam_constants(step, lr)
    a64 = [R.f64(x) for x in (p, g, m, v)]
    want = R.adam_reference(*a64, mult, c)
    bound = R.adam_bounds(*a64, mult, c)
    for i, k in enumerate(('p', 'mu', 'nu')):
        inside('adam ' + k, got[i], want[i], bound[k])
    return want


@pytest.mark.parametrize('step', R.ADAM_STEPS)
@pytest.mark.parametrize('n', R.ADAM_SIZES)
def test_adam_against_float64(M, n, step):
    """R.adam_bounds on mu, nu and the parameter, for every gradient scale and with the multiplier by pointer (0.37) and null (1)."""
    for scale in R.ADAM_SCALES:
        for mult in (0.37, None):
            p, g, m, v = R.adam_case(np.random.RandomState((n + 31 * step) % 100000 + int(-np.log10(scale))), n, step, scale)
            assert n < 7 or (g[::7] == 0).all()
            got, mult_read = _adam(M, p, g, m, v, mult, step)
            _adam_check(got, p, g, m, v, mult_read, step)


@pytest.mark.parametrize('mult', [float('nan'), 0.0])
@pytest.mark.parametrize('bad', ['nan', 'inf', '-inf'])
def test_adam_non_finite_gradient_only_decays_the_moments(M, bad, mult):
    """g * mult is NaN everywhere that matters (NaN multiplier: every element; 0: the non-finite one) and nan_to_num comes after the
    product: mu decays by b1, nu by b2, every output is finite."""
    p, g, m, v = R.adam_case(np.random.RandomState(3), 257, 10, 1e-3)
    g[5] = float(bad)
    got, mult_read = _adam(M, p, g, m, v, mult, 10)
    assert all(np.isfinite(x).all() for x in got)
    want = _adam_check(got, p, g, m, v, mult_read, 10)
    c = R.adam_constants(10, LR)
    np.testing.assert_array_equal(want[1], c['b1'] * R.f64(m))
    np.testing.assert_array_equal(want[2], c['b2'] * R.f64(v))


# ------------------------------------------------------------------------------------------------------------ trainer link
def _tratio(got, want, bound):
    r = (got.double() - want).abs() / bound
    r = torch.where((got.double() == want), torch.zeros_like(r), r)
    return float(torch.nan_to_num(r, nan=float('inf')).max())


@pytest.mark.parametrize('which', ['prop', 'nerf'])
def test_apply_one_follows_the_float64_chain_for_twenty_steps(M, which):
    """Mip360Trainer._apply_one (norm -> clip -> Adam -> re-pack) on gradients of scaled normals, 20 steps from tr.step = 1 and 20 from
    tr.step = 600 (past lr_delay_steps).  After every step: clip against R.norm_bound / R.clip_bound, flat / mu / nu against
    R.adam_reference started from the device state of the step before (R.adam_bounds, bounds do not compound).  After the 20th: against a
    float64 chain with optax's double constants and its own multipliers that was never restarted -- R.adam_bounds with the step
    before's bounds handed on and R.constant_distance, the documented distance.  The float64 chain runs in torch on the device (the
    reference functions take the array module); the gradient scales alternate between clipped (multiplier ~3e-4: g * mult ~ 3e-7, where
    sqrt(v_hat) ~ eps) and unclipped."""
    tr = M.Mip360Trainer(O.init_mlp_params(O.PROP_CFG, np.random.RandomState(0)), O.init_mlp_params(O.NERF_CFG, np.random.RandomState(1)),
                         dev(), max_steps=1000)
    k, tm = (1, tr.prop) if which == 'prop' else (0, tr.nerf)
    n = tm.flat.numel()
    gen = torch.Generator(device=dev()).manual_seed(5)
    for start in (1, 600):
        p64, m64, v64 = tm.flat.double(), tm.mu.double(), tm.nu.double()
        p_start = p64.clone()
        err = dict(m_err=0.0, v_rel=0.0, p_err=0.0)
        for i in range(20):
            tr.step = start + i
            scale = (1e-3, 1e-8 / np.sqrt(n / 5e5), 3e-5)[i % 3]
            tm.grads.normal_(generator=gen).mul_(scale)
            tm.grads[::7] = 0
            p0, m0, v0, g = tm.flat.double(), tm.mu.double(), tm.nu.double(), tm.grads.double()
            tr._apply_one(k, tm)
            lr = O.learning_rate_decay(tr.step - 1, 2e-3, 2e-5, 1000, 512, 0.01)
            norm = float(torch.sqrt((g * g).sum()))
            mult_dev, norm_dev = [float(x) for x in N(tr.clip[k])]
            inside('sum_squares', norm_dev, norm, R.norm_bound(norm, 256))
            mult = R.clip_reference(norm, tr.grad_max_norm)
            inside('clip_multiplier', mult_dev, mult, R.clip_bound(norm, tr.grad_max_norm, 256))
            assert (mult == 1) == (i % 3 == 1)
            c, ce = R.adam_constants(tr.step, lr), R.adam_constants(tr.step, lr, exact=True)
            want = R.adam_reference(p0, g, m0, v0, mult_dev, c, xp=torch)
            bound = R.adam_bounds(p0, g, m0, v0, mult_dev, c, xp=torch)
            for key, got, w in (('p', tm.flat, want[0]), ('mu', tm.mu, want[1]), ('nu', tm.nu, want[2])):
                worst = note('adam %s (trainer)' % key, _tratio(got, w, bound[key]))
                assert worst <= 1, (which, start, i, key, worst)
            # the chain that is never restarted: its own multiplier, whose distance from the device's is one more perturbation of g
            d = R.constant_distance(ce, c)
            rel_g = R.clip_bound(norm, tr.grad_max_norm, 256) / mult
            free = R.adam_bounds(p64, g, m64, v64, mult, ce, xp=torch, rel_m=d['rel_m'] + rel_g, rel_v=d['rel_v'] + 2 * rel_g,
                                 rel_u=d['rel_u'], **err)
            p64, m64, v64 = R.adam_reference(p64, g, m64, v64, mult, ce, xp=torch)
            err = dict(m_err=free['mu'], v_rel=free['v_rel'], p_err=free['p'])
        for key, got, w in (('p', tm.flat, p64), ('mu', tm.mu, m64), ('nu', tm.nu, v64)):
            worst = note('adam %s (20 steps, never restarted)' % key, _tratio(got, w, free[key]))
            assert worst <= 1, (which, start, key, worst)
        # (the accumulated bound still says something: it is a small part of how far the 20 steps moved a typical parameter)
        assert float((free['p'] / (tm.flat.double() - p_start).abs().clamp_min(R.DENORM)).median()) < 2.0 ** -7, 'the free chain bounds nothing'


# ------------------------------------------------------------------------------------------------------------ slab sums
def _reduce(M, slabs_dev, rows, n_in, n_out, ldg, ksplit, scale, with_bias):
    out = torch.full((rows * ldg + 16,), SENTINEL, device=dev())
    bias = torch.full((n_out + 16,), SENTINEL, device=dev()) if with_bias else None
    call(M, 'mip360_grad_weight_reduce', rows, n_in, n_out, ksplit, M._p(slabs_dev), M._p(out), ldg, scale, M._p(bias))
    assert untouched(out, 0, rows * ldg) and (bias is None or untouched(bias, 0, n_out))
    return out[:rows * ldg], (None if bias is None else bias[:n_out])


@pytest.mark.parametrize('ksplit', R.SLAB_KSPLITS)
@pytest.mark.parametrize('rows,n_in,n_out,ldg', R.SLAB_SHAPES)
def test_grad_weight_reduce_against_float64(M, rows, n_in, n_out, ldg, ksplit):
    """R.slab_sum_bound for the kernel slabs [ksplit, n_in, ldg] (the first rows * ldg elements of each are summed, padding columns
    included) and the bias slabs [ksplit, n_out] behind them, for both families, three scales, with and without the bias; the same call
    twice gives the same bits."""
    stride = n_in * ldg
    for family in ('random', 'cancelling'):
        rs = np.random.RandomState(ksplit * 7 + rows)
        ks, bs = R.slab_case(rs, family, ksplit, stride), R.slab_case(rs, family, ksplit, n_out)
        dev_slabs = T(np.concatenate([ks.reshape(-1), bs.reshape(-1)]))
        ks = ks[:, :rows * ldg]
        for scale in R.SLAB_SCALES:
            for with_bias in (True, False):
                out, bias = _reduce(M, dev_slabs, rows, n_in, n_out, ldg, ksplit, scale, with_bias)
                inside('slab_sum', N(out), R.slab_sum_reference(ks, scale), R.slab_sum_bound(ks, scale))
                if with_bias:
                    inside('slab_sum', N(bias), R.slab_sum_reference(bs, scale), R.slab_sum_bound(bs, scale))
        first, bias_first = _reduce(M, dev_slabs, rows, n_in, n_out, ldg, ksplit, R.SLAB_SCALES[-1], True)
        again, bias_again = _reduce(M, dev_slabs, rows, n_in, n_out, ldg, ksplit, R.SLAB_SCALES[-1], True)
        np.testing.assert_array_equal(N(again).view(np.uint32), N(first).view(np.uint32))
        np.testing.assert_array_equal(N(bias_again).view(np.uint32), N(bias_first).view(np.uint32))


@pytest.mark.parametrize('ksplit', [5, 13])
@pytest.mark.parametrize('n_out', [1, 3, 4, 257])
def test_grad_weight_reduce_bias_widths(M, n_out, ksplit):
    """the bias set's own blocks: one element, a tail, a whole 16-byte group, two blocks with a tail"""
    n_in = 8
    rs = np.random.RandomState(n_out)
    ks, bs = R.slab_case(rs, 'random', ksplit, n_in * n_out), R.slab_case(rs, 'cancelling', ksplit, n_out)
    dev_slabs = T(np.concatenate([ks.reshape(-1), bs.reshape(-1)]))
    for scale in R.SLAB_SCALES:
        out, bias = _reduce(M, dev_slabs, n_in, n_in, n_out, n_out, ksplit, scale, True)
        inside('slab_sum', N(out), R.slab_sum_reference(ks, scale), R.slab_sum_bound(ks, scale))
        inside('slab_sum', N(bias), R.slab_sum_reference(bs, scale), R.slab_sum_bound(bs, scale))


@pytest.mark.parametrize('ksplit', [5, 13, 17, 29, 33, 256])
@pytest.mark.parametrize('rows,ldg', [(4, 5), (12, 25)])
def test_slab_sum_vector_and_scalar_paths_give_the_same_bits(M, rows, ldg, ksplit):
    """The same slab values [ksplit, rows * ldg] (a multiple of 4 elements) once at a slab stride that is a multiple of 4 floats (n_in =
    rows: 16-byte loads, four slabs in flight) and once at an odd stride (n_in = rows + 1 with ldg odd: 4-byte loads, one slab at a time).
    The source says both keep one summation order; this holds it to that."""
    n = rows * ldg
    assert n % 4 == 0 and ((rows + 1) * ldg) % 2 == 1
    for family in ('random', 'cancelling'):
        vals = R.slab_case(np.random.RandomState(ksplit + n), family, ksplit, n)
        res = []
        for n_in in (rows, rows + 1):
            lay = np.full((ksplit, n_in * ldg), SENTINEL, f32)
            lay[:, :n] = vals
            out, _ = _reduce(M, T(lay), rows, n_in, ldg, ldg, ksplit, 0.25, False)
            res.append(N(out))
            inside('slab_sum', res[-1], R.slab_sum_reference(vals, 0.25), R.slab_sum_bound(vals, 0.25))
        np.testing.assert_array_equal(res[0].view(np.uint32), res[1].view(np.uint32))


def _staircase(m, n_out):
    """a first row of 256, then rows of 1.5 * 2^-16: float32 rounds every addition the same way (tests/test_mip360_update_reference.py)"""
    dz = np.full((m, n_out), 1.5 * 2.0 ** -16, f32)
    dz[0] = 256
    return dz * np.where(np.arange(n_out) % 2, f32(-1), f32(1))


@pytest.mark.parametrize('m', [1, 255, 256, 1000])
def test_grad_bias_against_float64(M, m):
    """mip360_grad_bias_bf16 (col_sum_kernel + slab_sum_kernel): R.col_sum_bound, lddz > n_out, nslice > m (empty slices add 0), twice
    the same bits, nothing written outside partial[nslice, n_out] and grad_bias[n_out]."""
    for n_out in (1, 3, 256, 257):
        lddz = n_out + 3
        for nslice in (1, 3, 4, 5):
            for family in ('random', 'staircase'):
                dz = R.round_bf16(np.random.RandomState(m + nslice).randn(m, n_out).astype(f32)) if family == 'random' else _staircase(m, n_out)
                full = np.full((m, lddz), 3.0, f32)
                full[:, :n_out] = dz
                tz = T(full).to(torch.bfloat16)
                res = []
                for scale in (1.0, -3.0, -3.0):
                    partial = torch.full((nslice * n_out + 16,), SENTINEL, device=dev())
                    out = torch.full((n_out + 16,), SENTINEL, device=dev())
                    call(M, 'mip360_grad_bias_bf16', m, n_out, M._p(tz), lddz, nslice, M._p(partial), M._p(out), scale)
                    assert untouched(partial, 0, nslice * n_out) and untouched(out, 0, n_out)
                    inside('col_sum', N(out[:n_out]), R.col_sum_reference(dz, scale), R.col_sum_bound(dz, nslice, scale))
                    res.append(N(out[:n_out]))
                np.testing.assert_array_equal(res[1].view(np.uint32), res[2].view(np.uint32))


# ------------------------------------------------------------------------------------------------------------ one output column
@pytest.mark.parametrize('lddz', [8, 32])
@pytest.mark.parametrize('m,n_in,ksplit', [(1000, 264, 3), (2048, 256, 8), (300, 8, 1), (129, 512, 1)])
def test_one_column_weight_gradient_runs_its_unrolled_body(M, m, n_in, ksplit, lddz):
    """mip360_grad_weight_bf16 with n_out = 1 (grad_weight_col_kernel): slices of 334, 256, 300 and 129 rows, so the body with 16 rows
    in flight per thread (it needs more than 120 rows) runs with a tail, without one, and exactly once; 264 columns leave a partial second
    column group.  ((300, 256, 1, 32) of tests/test_gpu_mip360.py::test_grad_weight_and_bias_against_numpy gets ksplit = 8, 38 rows per
    slice, and never enters that body.)  Against the float64 H^T z of the bfloat16 operands: R.col_dot_tolerance (the form of
    test_one_column_kernels) for the kernel gradient, R.col_dot_bias_bound for the bias."""
    rs = np.random.RandomState(m + lddz)
    h = R.round_bf16(rs.randn(m, n_in).astype(f32))
    z = R.round_bf16(rs.randn(m).astype(f32))
    ldh = n_in + 8
    hp, zp = np.full((m, ldh), 5.0, f32), np.full((m, lddz), 5.0, f32)
    hp[:, :n_in], zp[:, 0] = h, z
    th, tz = T(hp).to(torch.bfloat16), T(zp).to(torch.bfloat16)
    slabs = torch.full((ksplit * (n_in + 1) + 16,), SENTINEL, device=dev())
    gk, gb = torch.full((n_in + 16,), SENTINEL, device=dev()), torch.full((1 + 16,), SENTINEL, device=dev())
    call(M, 'mip360_grad_weight_bf16', m, n_in, 1, M._p(th), ldh, M._p(tz), lddz, ksplit, M._p(slabs), M._p(gk), 1, 1.0, M._p(gb))
    assert untouched(slabs, 0, ksplit * (n_in + 1)) and untouched(gk, 0, n_in) and untouched(gb, 0, 1)
    want_k, want_b = R.col_dot_reference(h, z)
    inside('col_dot', N(gk[:n_in]), want_k, R.col_dot_tolerance(want_k))
    inside('col_dot bias', N(gb[:1]), want_b, R.col_dot_bias_bound(z, m, ksplit))


def test_one_column_weight_gradient_refuses_an_unpadded_dz(M):
    """lddz = 1 (dZ as a plain vector) is not a shape mip360_grad_weight_bf16 takes: leading dimensions are multiples of 8.  The
    plain-vector form is mip360_grad_weight_col_fm's (tests/test_gpu_mip360_fm.py::test_one_column_kernels)."""
    x = torch.zeros(300 * 8, dtype=torch.bfloat16, device=dev())
    s = torch.zeros(64, device=dev())
    with pytest.raises(M.Mip360Error):
        call(M, 'mip360_grad_weight_bf16', 300, 8, 1, M._p(x), 8, M._p(x), 1, 1, M._p(s), M._p(s), 1, 1.0, M._p(s))


# ------------------------------------------------------------------------------------------------------------ head backward
@pytest.mark.parametrize('rows', [1, 255, 256, 257, 4099])
def test_head_backward_against_float64(M, rows):
    """R.head_backward_bounds on d_raw and d_pre (a result below 2^-126 may come back as 0: the bound says so); the zero fill covers
    exactly [raw_col + 1, raw_zero_to) of d_raw and columns 3 .. 31 of d_pre; every other bit of the sentinel-filled buffers is unchanged.
    d_pre null is the PropMLP's call (with ld_raw = 1, raw_col = 0: d_raw as a plain vector)."""
    pad = 0.001
    density, g_d, rgb, g_c = R.head_case(np.random.RandomState(rows), rows, pad)
    want_raw, want_pre = R.head_backward_reference(density, g_d, rgb, g_c, pad)
    b_raw, b_pre = R.head_backward_bounds(density, g_d, rgb, g_c, pad)
    td, tg, tc, tgc = T(density), T(g_d), T(rgb), T(g_c)
    sent = bits(np.array([SENTINEL], f32))[0]
    for raw_col, ld_raw in ((0, 64), (256, 320), (0, 1)):
        for zero_to in sorted({raw_col + 1, min(ld_raw, (raw_col + 32) // 32 * 32), ld_raw}):
            for colour in ((True, False) if ld_raw > 1 else (False,)):
                d_raw = torch.full(((rows + 2) * ld_raw,), SENTINEL, dtype=torch.bfloat16, device=dev())
                d_pre = torch.full(((rows + 2) * 32,), SENTINEL, dtype=torch.bfloat16, device=dev()) if colour else None
                call(M, 'mip360_head_backward', rows, M._p(td), M._p(tg), M._p(tc) if colour else None, M._p(tgc) if colour else None, pad,
                     M._p(d_raw), ld_raw, raw_col, zero_to, M._p(d_pre))
                raw = d_raw.view(rows + 2, ld_raw)
                inside('head_backward d_raw', N(raw[:rows, raw_col]), want_raw, b_raw)
                b = bits(raw)
                assert (b[:rows, raw_col + 1:zero_to] == 0).all()                              # +0, not -0
                assert (b[:rows, :raw_col] == sent).all() and (b[:rows, zero_to:] == sent).all() and (b[rows:] == sent).all()
                if colour:
                    pre = d_pre.view(rows + 2, 32)
                    inside('head_backward d_pre', N(pre[:rows, :3]), want_pre, b_pre)
                    b = bits(pre)
                    assert (b[:rows, 3:] == 0).all() and (b[rows:] == sent).all()


# ------------------------------------------------------------------------------------------------------------ packing
def _up(x, k):
    return -(-x // k) * k


def _pack_layout(n_in, n_out, bwd_rows=None, col0=16):
    """padded leading dimensions and buffer sizes (elements) of the four destinations of one [n_in, n_out] tensor"""
    bwd_rows = n_in if bwd_rows is None else bwd_rows
    ld = dict(ld_fwd=n_in + 8, ld_bwd=n_out + 2, ld_fwd_fm=_up(n_in, 16) + 16, ld_bwd_fm=_up(col0 + n_out, 16) + 16, bwd_rows=bwd_rows, bwd_col0=col0)
    size = dict(fwd=n_out * ld['ld_fwd'] + 8, bwd=n_in * ld['ld_bwd'] + 8, fwd_fm=_up(n_out, 32) * ld['ld_fwd_fm'] + 8,
                bwd_fm=_up(max(bwd_rows, 1), 32) * ld['ld_bwd_fm'] + 8)
    return ld, size


def _pack_want(k, ld, size, use):
    dst = {key: (np.full(size[key], SENTINEL, f32) if key in use else None) for key in ('fwd', 'bwd', 'fwd_fm', 'bwd_fm')}
    R.pack_reference(k, dst['fwd'], ld['ld_fwd'], dst['bwd'], ld['ld_bwd'], dst['fwd_fm'], ld['ld_fwd_fm'], dst['bwd_fm'], ld['ld_bwd_fm'],
                     ld['bwd_rows'], ld['bwd_col0'])
    return dst


def _pack_dst(size, use):
    return {key: (torch.full((size[key],), SENTINEL, dtype=torch.bfloat16, device=dev()) if key in use else None)
            for key in ('fwd', 'bwd', 'fwd_fm', 'bwd_fm')}


def _pack_fm_call(M, tk, n_in, n_out, dst, ld):
    call(M, 'mip360_pack_weight_fm', n_in, n_out, M._p(tk), M._p(dst['fwd']), ld['ld_fwd'], M._p(dst['bwd']), ld['ld_bwd'], M._p(dst['fwd_fm']),
         ld['ld_fwd_fm'], M._p(dst['bwd_fm']), ld['ld_bwd_fm'], ld['bwd_rows'], ld['bwd_col0'])


def _same_bits(got, want):
    for key, w in want.items():
        if w is not None:
            np.testing.assert_array_equal(bits(got[key]), bits(w), err_msg=key)


@pytest.mark.parametrize('n_in,n_out', [(504, 256), (760, 256), (256, 1), (283, 128), (128, 3)])
def test_pack_weight_rounds_to_even_and_leaves_the_padding(M, n_in, n_out):
    """mip360_pack_weight and mip360_pack_weight_fm bit for bit against R.pack_reference (round to nearest even of every element, to
    fwd[o, i], bwd[i, o] and the two fm positions) on values that sit on ties of both parities, next to ties, and below the normal range;
    every destination is sentinel-filled with padded leading dimensions, so a write outside the window shows."""
    k = R.pack_case(np.random.RandomState(n_in + n_out), n_in, n_out)
    tk = T(k)
    ld, size = _pack_layout(n_in, n_out, bwd_rows=n_in - n_in // 3)
    for use in (('fwd', 'bwd'), ('fwd',), ('bwd',)):
        dst = _pack_dst(size, use)
        call(M, 'mip360_pack_weight', n_in, n_out, M._p(tk), M._p(dst['fwd']), ld['ld_fwd'], M._p(dst['bwd']), ld['ld_bwd'])
        _same_bits(dst, _pack_want(k, ld, size, use))
    for use in (('fwd', 'bwd', 'fwd_fm', 'bwd_fm'), ('fwd_fm',), ('bwd_fm',), ('bwd', 'bwd_fm')):
        dst = _pack_dst(size, use)
        _pack_fm_call(M, tk, n_in, n_out, dst, ld)
        _same_bits(dst, _pack_want(k, ld, size, use))


def test_pack_batch_of_sixteen_very_different_tensors_equals_the_single_calls(M):
    """One mip360_pack_weights_fm_batch over 16 descriptors from 3 to 194 560 elements (the grid is sized by the largest: the blocks
    beyond a small tensor's elements must leave at once), some destinations null (one descriptor all four), some bwd_rows < n_in: bit for
    bit the per-tensor mip360_pack_weight_fm calls and R.pack_reference, padding untouched."""
    shapes = [(1, 3), (760, 256), (128, 3), (256, 1), (283, 128), (504, 256), (3, 1), (5, 7), (17, 33), (64, 64), (8, 256), (100, 10),
              (31, 1), (2, 2), (300, 5), (16, 16)]
    assert len(shapes) == 16 and min(i * o for i, o in shapes) == 3 and max(i * o for i, o in shapes) == 194560
    keys = ('fwd', 'bwd', 'fwd_fm', 'bwd_fm')
    uses = [keys, keys, ('fwd', 'fwd_fm'), ('bwd', 'bwd_fm'), keys, ('fwd_fm', 'bwd_fm'), (), keys, ('bwd_fm',), keys, ('fwd',), keys,
            ('fwd_fm',), keys, ('bwd',), keys]
    items, descs = [], []
    for t, ((n_in, n_out), use) in enumerate(zip(shapes, uses)):
        k = R.pack_case(np.random.RandomState(t), n_in, n_out)
        ld, size = _pack_layout(n_in, n_out, bwd_rows=n_in if t % 3 else max(1, n_in // 2), col0=16 * (t % 2))
        tk, batch, single = T(k), _pack_dst(size, use), _pack_dst(size, use)
        items.append((k, tk, n_in, n_out, ld, size, use, batch, single))
        ptr = lambda x: None if x is None else x.data_ptr()
        descs.append(M.PackDesc(tk.data_ptr(), n_in, n_out, ptr(batch['fwd']), ptr(batch['bwd']), ptr(batch['fwd_fm']), ptr(batch['bwd_fm']),
                                ld['ld_fwd'], ld['ld_bwd'], ld['ld_fwd_fm'], ld['ld_bwd_fm'], ld['bwd_rows'], ld['bwd_col0']))
    arr = (M.PackDesc * 16)(*descs)
    call(M, 'mip360_pack_weights_fm_batch', 16, C.cast(arr, C.c_void_p))
    for k, tk, n_in, n_out, ld, size, use, batch, single in items:
        _pack_fm_call(M, tk, n_in, n_out, single, ld)
        want = _pack_want(k, ld, size, use)
        _same_bits(batch, want)
        _same_bits(single, want)


def test_lazy_repack_then_ensure_rm_equals_a_fresh_repack(M):
    """TrainableMLP on the fm path: after the master parameters move, repack(lazy=True) refreshes the fm copies (and the row-major ones
    the fm path still reads) and marks the rest stale; ensure_rm() then leaves every row-major and fm copy equal, bit for bit, to those
    of an MLP built from the moved parameters."""
    rs = np.random.RandomState(0)
    tm = M.TrainableMLP(O.init_mlp_params(O.NERF_CFG, rs), M.NERF_CFG, dev())
    assert tm.w_fm and tm.wb_fm and not tm.rm_stale
    tm.flat.add_(torch.from_numpy(rs.randn(tm.flat.numel()).astype(f32) * f32(0.01)).to(dev()))
    fresh = M.TrainableMLP([(N(k), N(b)) for k, b in tm.state()], M.NERF_CFG, dev())
    copies = lambda x: ([('w', t, x.w[t]) for t in range(len(x.w))] + [('wb', t, v) for t, v in x.wb.items()]
                        + [('w_fm', t, v) for t, v in x.w_fm.items()] + [('wb_fm', t, v) for t, v in x.wb_fm.items()])
    stale_before = {(name, t): bits(v) for name, t, v in copies(tm)}
    tm.repack(lazy=True)
    assert tm.rm_stale
    for (name, t, got), (_, _, want) in zip(copies(tm), copies(fresh)):
        if name.endswith('_fm'):
            np.testing.assert_array_equal(bits(got), bits(want), err_msg='%s[%s] after the lazy repack' % (name, t))
    assert any((bits(got) == stale_before[(name, t)]).all() and (bits(got) != bits(want)).any()
               for (name, t, got), (_, _, want) in zip(copies(tm), copies(fresh))), 'the lazy repack skipped nothing'
    tm.ensure_rm()
    assert not tm.rm_stale
    for (name, t, got), (_, _, want) in zip(copies(tm), copies(fresh)):
        np.testing.assert_array_equal(bits(got), bits(want), err_msg='%s[%s] after ensure_rm' % (name, t))


# ------------------------------------------------------------------------------------------------------------ report
def test_worst_ratios_report():
    """the worst |error| / bound per kernel over this module's run (DESIGN.md records them); every one at most 1"""
    for name in sorted(WORST):
        print('worst ratio %-44s %.3f' % (name, WORST[name]))
    assert all(v <= 1.0 for v in WORST.values())

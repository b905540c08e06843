"""GPU tests of the hand-written non-MLP kernels of the NeRF++ path, one by one, against the float64 restatements of
tests/nerfpp_render_reference.py (R) and inside the bounds that module derives from the inputs (constants calibrated on the CPU
against float32 implementations of the reference's arithmetic, tests/test_nerfpp_render_reference.py):

* composite_fwd_kernel / composite_bwd_kernel through the inspection entry points ops.composite / ops.composite_backward: S at the
  samples-per-lane boundaries (64|65, 128|129, 192|193, 256), ray counts around the four-rays-per-workgroup mapping, zero and negative
  sigma_raw, saturating exponents, underflowing transmittance, zero-width intervals, the background's 1e10 interval, colours at 0 and
  1, |ray_d| from 1e-3 to 1e3; every element of every output, outputs as views into sentinel-padded buffers, run-to-run bits;
* loss_kernel / kl_terms_kernel (ops.loss_and_grads) above the 1024 threads of the single workgroup, priors at -0.0, fg_far and
  nextafter(fg_far, 0), exact zeros of the residuals, w == 0 and dists == 0 under the KL logarithm, an underflowing exponential; the
  fused head composite_bwd_kernel<true> bit for bit against the unfused call fed with nerfpp_loss's gradients;
* adam_kernel (ops.adam_step): steps 1 ... 500 000, gradients from 1e-20 to 1e18, overflowing g g, cancelling moments, the skip
  predicate, a dyadic step that is exact, 20 chained steps against the float64 chain restarted from the device state;
* sphere_far (ops.intersect_sphere, ops.sample_coarse): near-tangent rays, |ray_d| from 1e-3 to 1e3, and the bad-ray counter once per
  ray whatever S.

The product path reaches the two compositing kernels through the same launchers with the same grid (nerfpp_level_forward /
nerfpp_level_backward call launch_composite_fwd / launch_composite_bwd exactly as the entry points do): that tie is by construction.

Every tolerance is a bound function of R; the worst |error| / bound per kernel is printed (pytest -s) and collected by the last test."""
import functools

import numpy as np
import pytest

torch = pytest.importorskip('torch')
pytestmark = pytest.mark.gpu

from oracle import nerfpp_oracle as O                                    # noqa: E402
from tests import nerfpp_render_reference as R                           # noqa: E402
from tests.test_gpu_mip360 import T, N, dev                              # noqa: E402
from tests.test_gpu_mip360_update import guarded, untouched              # noqa: E402

f32 = np.float32
WORST = {}
LEAD = 16                                 # floats in front of every guarded output: keeps the float4 stores of dout 16-byte aligned
LOSS_NAMES = {0: 'rgbonly', 1: 'mse', 2: 'l1', 3: 'kl'}
SHAPES = dict(rgb=3, fg_rgb=3, bg_rgb=3, fg_weights='S', bg_weights='S', fg_dists='S', depth=1, fg_depth=1, bg_depth=1, bg_lambda=1)


@pytest.fixture(scope='module')
def ops():
    dev()
    from outdoor_nerf_depth_amd import ops
    return ops


def note(name, value):
    value = float(value)
    WORST[name] = max(WORST.get(name, 0.0), value)
    return value


def inside(kernel, output, got, want, bound):
    """every element within its bound; records the worst ratio under the kernel's name and under kernel.output"""
    r = R.ratio(got, want, bound)
    worst = note(kernel, r.max())
    note('%s.%s' % (kernel, output), worst)
    k = int(np.argmax(r))
    assert worst <= 1.0, (kernel, output, worst, k, np.ravel(R.f64(got))[k], np.ravel(R.f64(want))[k], np.ravel(bound + 0 * R.f64(want))[k])


def bits(t):
    return t.contiguous().view(torch.int32)


def same_bits(a, b):
    return bool(torch.equal(bits(a), bits(b)))


def nan_buffer(size):
    """a guarded output of `size` floats, NaN inside (an element the kernel leaves out fails every comparison)"""
    return guarded(np.full(size, np.nan, f32), lead=LEAD)


@functools.lru_cache(maxsize=None)
def composite_case(family, S, n):
    return R.composite_case(family, S, n)


def forward(ops, case):
    """ops.composite into guarded views; returns (ret of device views, {name: whole buffer})"""
    n, S = case['fg_z'].shape
    bufs, out = {}, {}
    for k in R.RET_KEYS:
        w = S if SHAPES[k] == 'S' else SHAPES[k]
        bufs[k], view = nan_buffer(n * w)
        out[k] = view.view(n, w) if w > 1 else view
    ret = ops.composite(*[T(case[k]) for k in R._IN_KEYS], out=out)
    for k in R.RET_KEYS:
        assert untouched(bufs[k], LEAD, ret[k].numel()), k
    return ret, bufs


def backward(ops, case, g_rgb=None, g_depth=None, g_w=None, fused_loss=None):
    n, S = case['fg_z'].shape
    (b_fg, v_fg), (b_bg, v_bg) = nan_buffer(n * S * 4), nan_buffer(n * S * 4)
    up = [None if g is None else T(g) for g in (g_rgb, g_depth, g_w)]
    dout = ops.composite_backward(*[T(case[k]) for k in R._IN_KEYS], *up, fused_loss=fused_loss, out=(v_fg.view(n * S, 4), v_bg.view(n * S, 4)))
    assert untouched(b_fg, LEAD, n * S * 4) and untouched(b_bg, LEAD, n * S * 4)
    return dout


# ------------------------------------------------------------------------------------------------------------ compositing
@pytest.mark.parametrize('S', R.COMPOSITE_S)
def test_composite_forward_against_float64(ops, S):
    """R.composite_bounds, every element of the ten outputs, every family at this S.  Everything is finite; a sample without density
    has weight exactly 0; a weight that float64 puts below 2^-149 is 0 or inside its bound; the call repeated gives the same bits; the
    ray with -sigma_raw gives the same bits."""
    for family, n in R.composite_cases(S):
        case = composite_case(family, S, n)
        ret, bufs = forward(ops, case)
        want, bound = R.composite64(**case), R.composite_bounds(case)
        got = {k: N(ret[k]) for k in R.RET_KEYS}
        for k in R.RET_KEYS:
            assert np.isfinite(got[k]).all(), (family, n, k)
            inside('composite_fwd', k, got[k], want[k], bound[k])
        zero_fg = case['raw_fg'][:, 3].reshape(n, S) == 0
        zero_bg = (case['raw_bg'][:, 3].reshape(n, S) == 0)[:, ::-1]
        assert not got['fg_weights'][zero_fg].any() and not got['bg_weights'][zero_bg].any()
        for k in ('fg_weights', 'bg_weights'):
            below = want[k] < R.DENORM
            assert np.all((got[k][below] == 0) | (np.abs(got[k][below] - want[k][below]) <= bound[k][below]))
        again, bufs2 = forward(ops, case)
        assert all(same_bits(bufs[k], bufs2[k]) for k in R.RET_KEYS)
        if family in ('general', 'zero', 'saturating'):
            mir, _ = forward(ops, R.mirrored(case))
            assert all(same_bits(ret[k], mir[k]) for k in R.RET_KEYS), family


def test_composite_forward_ray_without_density(ops):
    """sigma_raw == 0 on a whole ray: alpha == 0 everywhere, so rgb and depth are exactly 0 and bg_lambda is the product of S values
    of float32(1 + TINY), whatever the order of the products: within gamma(S) of its float64 value"""
    for S in (2, 65, 256):
        case = composite_case('zero', S, 4)
        ret, _ = forward(ops, case)
        whole = (case['raw_fg'][:, 3].reshape(4, S) == 0).all(1) & (case['raw_bg'][:, 3].reshape(4, S) == 0).all(1)
        assert whole[::2].all()
        for k in ('rgb', 'depth', 'fg_rgb', 'bg_rgb', 'fg_depth', 'bg_depth'):
            assert not N(ret[k])[whole].any(), k
        q = float(f32(1) - f32(0) + f32(R.TINY))
        lam = N(ret['bg_lambda'])[whole]
        assert np.all(np.abs(lam - q ** S) <= R.gamma(S) * q ** S)


@pytest.mark.parametrize('S', R.COMPOSITE_S)
def test_composite_backward_against_float64(ops, S):
    """R.composite_backward_bounds (the float64 gradient is autograd's, not the hand-derived backward the kernel shares with the
    oracle), every element of both dout tensors, every family and upstream gradient at this S.  A bound of 0 is an exact comparison:
    d sigma_raw at sigma_raw == 0, d rgb at colours 0 and 1 and under g_rgb == 0.  All-zero upstream gradients give all-zero dout; a
    null g_fg_weights gives the bits of a zero tensor; the call repeated gives the same bits; -sigma_raw negates d sigma_raw exactly."""
    for family, n in R.composite_cases(S):
        case = composite_case(family, S, n)
        for kind in R.UPSTREAM:
            up = R.upstream(kind, S, n)
            dout = backward(ops, case, *up)
            want, bound = R.composite_backward64(case, *up), R.composite_backward_bounds(case, *up)
            for vol, name in ((0, 'fg'), (1, 'bg')):
                got = N(dout[vol])
                assert np.isfinite(got).all(), (family, n, kind, name)
                inside('composite_bwd', 'd_rgb_' + name, got[:, :3], want[vol][:, :3], bound[vol][:, :3])
                inside('composite_bwd', 'd_sigma_' + name, got[:, 3], want[vol][:, 3], bound[vol][:, 3])
                if kind == 'zero':
                    assert not got.any(), (family, n, name)
            if kind == 'random':
                again = backward(ops, case, *up)
                assert same_bits(dout[0], again[0]) and same_bits(dout[1], again[1])
                if family in ('general', 'zero', 'saturating'):
                    mir = backward(ops, R.mirrored(case), *up)
                    for a, b in zip(dout, mir):
                        assert same_bits(a[:, :3], b[:, :3]) and bool(torch.equal(a[:, 3], -b[:, 3])), family      # (0 == -0: sign(0) = 0)
            if kind == 'no_weights':
                zeros = backward(ops, case, up[0], up[1], np.zeros((n, S), f32))
                assert same_bits(dout[0], zeros[0]) and same_bits(dout[1], zeros[1])


# ------------------------------------------------------------------------------------------------------------ loss head
def device_ret(c):
    return {k: T(c[k]) for k in ('rgb', 'depth', 'fg_weights', 'fg_dists')}


def loss64_of(c, t, lam, sig):
    return R.loss64(t, lam, sig, c['rgb'], c['rgb_gt'], c['depth'], c['depth_sup'], c['fg_weights'], c['fg_z'], c['fg_dists'], c['fg_far'])


def check_loss(kernel, c, t, got_scalars, g_rgb, g_depth, g_w, lam, sig):
    want, bound = loss64_of(c, t, lam, sig)
    sc = N(got_scalars)
    assert sc[3] == want['n_valid']
    inside(kernel, 'rgb_loss', sc[1], want['rgb_loss'], bound['rgb_loss'])
    if np.isnan(want['loss']):                                                     # empty mse / l1 mask: 0 / 0 like the reference
        assert np.isnan(sc[0]) and np.isnan(sc[2]) and not N(g_depth).any()
    else:
        inside(kernel, 'loss', sc[0], want['loss'], bound['loss'])
        inside(kernel, 'depth_loss', sc[2], want['depth_loss'], bound['depth_loss'])
    inside(kernel, 'g_rgb', N(g_rgb), want['g_rgb'], bound['g_rgb'])
    inside(kernel, 'g_depth', N(g_depth), want['g_depth'], bound['g_depth'])
    if g_w is not None:
        inside(kernel, 'g_w', N(g_w), want['g_w'], bound['g_w'])                  # (bound 0 outside the KL mask and for the other types)
    return sc


@pytest.mark.parametrize('n', R.LOSS_N)
def test_loss_head_against_float64(ops, n):
    """ops.loss_and_grads on every S x mask x type of R.loss_cases at this n (lambda_depth and kl_sigma walk through their lists).
    n_valid is exact; an empty mse / l1 mask gives NaN loss and depth_loss, the rgb_loss of the rgb-only call, and zero gradients;
    g_w outside the KL mask is exactly 0; an rgb residual of exactly 0 and depth == gt under l1 give gradients of exactly 0."""
    cases = [c for c in R.loss_cases() if c[0] == n]
    for S in R.LOSS_S:
        for mask in R.LOSS_MASKS:
            c = R.loss_case(n, S, mask)
            ret, gt, sup, z, far = device_ret(c), T(c['rgb_gt']), T(c['depth_sup']), T(c['fg_z']), T(c['fg_far'])
            rgb_loss_bits = None
            for _, _, _, t, lam, sig in [k for k in cases if k[1] == S and k[2] == mask]:
                sc, g_rgb, g_depth, g_w = ops.loss_and_grads(ret, gt, sup if t else None, LOSS_NAMES[t], lam, sig, z, far)
                host = check_loss('kl_terms+loss' if t == 3 else 'loss', c, t, sc, g_rgb, g_depth, g_w, lam, sig)
                assert not N(g_rgb)[::5].any()
                rgb_loss_bits = host[1:2].view(np.uint32) if rgb_loss_bits is None else rgb_loss_bits
                assert host[1:2].view(np.uint32) == rgb_loss_bits                  # rgb_loss does not depend on the depth term
                if t == 2:
                    same = (c['depth'] == c['depth_sup']) & (c['depth_sup'] > 0)
                    assert (same.any() or n < 8 or mask == 'none') and not N(g_depth)[same].any()


def test_loss_head_zero_fill_and_extent(ops):
    """nerfpp_loss with a g_fg_weights buffer for every type: all zeros unless KL; nothing written outside n*3, n, n*S and the 4 scalars"""
    from outdoor_nerf_depth_amd import _lib as L
    from outdoor_nerf_depth_amd._ctypes_util import p as P, stream
    for n, S in ((1, 2), (257, 65), (1025, 2)):
        c = R.loss_case(n, S, 'mixed')
        d = {k: T(v) for k, v in c.items()}
        for t in range(4):
            (b_sc, sc), (b_rgb, g_rgb), (b_dep, g_dep), (b_w, g_w) = nan_buffer(4), nan_buffer(n * 3), nan_buffer(n), nan_buffer(n * S)
            L.check(L.lib().nerfpp_loss(stream(), n, S, t, 0.3, 0.01, P(d['rgb']), P(d['rgb_gt']), P(d['depth']), P(d['depth_sup']),
                                        P(d['fg_weights']), P(d['fg_z']), P(d['fg_dists']), P(d['fg_far']), P(sc), P(g_rgb), P(g_dep), P(g_w)))
            assert untouched(b_sc, LEAD, 4) and untouched(b_rgb, LEAD, n * 3) and untouched(b_dep, LEAD, n) and untouched(b_w, LEAD, n * S)
            check_loss('kl_terms+loss' if t == 3 else 'loss', c, t, sc, g_rgb.view(n, 3), g_dep, g_w.view(n, S), 0.3, 0.01)
            if t != 3:
                assert not N(g_w).any()


@pytest.mark.parametrize('kl_sigma', R.KL_SIGMAS)
def test_kl_underflowing_exponential_is_exactly_zero(ops, kl_sigma):
    """(z - gt)^2 / (2 sigma) >= 200: every term and every gradient is exactly 0 although every ray is inside the mask"""
    n, S = 257, 65
    c = R.kl_far_case(n, S, kl_sigma)
    sc, g_rgb, g_depth, g_w = ops.loss_and_grads(device_ret(c), T(c['rgb_gt']), T(c['depth_sup']), 'kl', 1.0, kl_sigma, T(c['fg_z']), T(c['fg_far']))
    host = N(sc)
    assert host[3] == n and host[2] == 0 and host[0] == host[1] and not N(g_w).any() and not N(g_depth).any()


@pytest.mark.parametrize('n', R.FUSED_N)
def test_fused_head_equals_the_unfused_call_bit_for_bit(ops, n):
    """composite_bwd_kernel<true> forms dL/d rgb, dL/d depth and dL/d fg_weights itself, with every workgroup recounting the mse / l1
    normaliser: dout equals, bit for bit, the unfused call fed with nerfpp_loss's gradients -- all four types, mixed and empty mask"""
    S = 65 if n != 5 else 2
    case = composite_case('general', S, n)
    ret, _ = forward(ops, case)
    rs = np.random.RandomState(n)
    rgb_gt = T(rs.rand(n, 3).astype(f32))
    for mask in ('mixed', 'none'):
        sup = T(R.depth_sup_for(mask, case['fg_far'], rs))
        for t in range(4):
            lam, sig = R.LOSS_LAMBDAS[(t + 1) % 3], R.KL_SIGMAS[t % 3]
            sc, g_rgb, g_depth, g_w = ops.loss_and_grads(ret, rgb_gt, sup if t else None, LOSS_NAMES[t], lam, sig, T(case['fg_z']), T(case['fg_far']))
            unfused = backward(ops, case, N(g_rgb), N(g_depth), None if g_w is None else N(g_w))
            fused = backward(ops, case, fused_loss=dict(loss_type=LOSS_NAMES[t], lambda_depth=lam, kl_sigma=sig, ret=ret, rgb_gt=rgb_gt,
                                                        depth_sup=sup if t else None))
            assert same_bits(unfused[0], fused[0]) and same_bits(unfused[1], fused[1]), (mask, t)
            assert bool(torch.isfinite(fused[0]).all()) and bool(torch.isfinite(fused[1]).all())


# ------------------------------------------------------------------------------------------------------------ Adam
def adam(ops, p, g, m, v, step, skip=None, lead=1, **kw):
    """ops.adam_step on guarded copies (4-byte aligned views); returns the device views (p, m, v) after the step"""
    n = p.size
    (bp, dp), (bm, dm), (bv, dv) = guarded(p, lead=lead), guarded(m, lead=lead), guarded(v, lead=lead)
    ops.adam_step(dp, T(g), dm, dv, step, skip=skip, **kw)
    assert untouched(bp, lead, n) and untouched(bm, lead, n) and untouched(bv, lead, n)
    return dp, dm, dv


@pytest.mark.parametrize('step', R.ADAM_STEPS)
@pytest.mark.parametrize('n', R.ADAM_N)
def test_adam_against_float64(ops, n, step):
    """R.adam_bounds on p, m and v; the elements walk through gradients from 1e-20 to 1e18.  g == 0 with m == v == 0 leaves p's bits;
    at step 1 exp_avg is one rounding of an exact product, (float)(1 - beta1) g, and has exactly those bits."""
    p, g, m, v = R.adam_case(n, step)
    got = adam(ops, p, g, m, v, step)
    want, bound = R.adam64(p, g, m, v, step), R.adam_bounds(p, g, m, v, step)
    for k, a, b in zip('pmv', got, want):
        assert bool(torch.isfinite(a).all())
        inside('adam', k, N(a), b, bound[k])
    if step == 1:                                      # m == 0: one rounding of an exact product, so the bits are known
        exact, normal = R.adam_first_step_m(g)
        assert np.array_equal(N(got[1])[normal].view(np.uint32), exact[normal].view(np.uint32))
    still = (g == 0) & (m == 0) & (v == 0)
    assert np.array_equal(N(got[0])[still].view(np.uint32), p[still].view(np.uint32)) and not N(got[1])[still].any() and not N(got[2])[still].any()


def test_adam_overflow_skip_and_dyadic(ops):
    n = 257
    p, g, m, v = R.adam_case(n, 10)
    # g g overflows: v becomes inf, the update 0, nothing NaN -- and again on the next step from that state
    big = np.where(np.arange(n) % 2 == 0, f32(1e25), f32(-1e25)).astype(f32)
    dp, dm, dv = adam(ops, p, big, m, v, 10)
    assert same_bits(dp, T(p)) and bool(torch.isinf(dv).all()) and bool(torch.isfinite(dm).all())
    inside('adam', 'm', N(dm), R.adam64(p, big, m, v, 10)[1], R.adam_bounds(p, big, m, v, 10)['m'])
    dp2, dm2, dv2 = adam(ops, N(dp), g, N(dm), N(dv), 11)
    assert same_bits(dp2, T(p)) and bool(torch.isinf(dv2).all()) and not bool(torch.isnan(dm2).any())
    # the skip predicate: null and 0 are the same step, anything else leaves p, m and v alone
    plain = adam(ops, p, g, m, v, 10)
    zero = adam(ops, p, g, m, v, 10, skip=torch.zeros(1, device=dev()))
    assert all(same_bits(a, b) for a, b in zip(plain, zero)) and not same_bits(plain[0], T(p))
    for value in (1.0, -3.0, 1e-30, float('nan')):
        kept = adam(ops, p, g, m, v, 10, skip=torch.full((1,), value, device=dev()))
        assert all(same_bits(a, T(b)) for a, b in zip(kept, (p, m, v))), value
    # a step whose every operation is exact in float32
    p, g, m, v, kw = R.adam_dyadic_case(n)
    got = adam(ops, p, g, m, v, kw['step'], lr=kw['lr'], beta1=kw['beta1'], beta2=kw['beta2'], eps=kw['eps'])
    want = R.adam64(p, g, m, v, kw['step'], kw['lr'], kw['beta1'], kw['beta2'], kw['eps'])
    assert all(np.array_equal(R.f64(N(a)), b) for a, b in zip(got, want))


@pytest.mark.parametrize('first', (1, 1000))
def test_adam_twenty_chained_steps(ops, first):
    """every step against the float64 step restarted from the device state of the step before"""
    n = 257
    p, _, m, v = R.adam_case(n, first)
    (bp, dp), (bm, dm), (bv, dv) = guarded(p), guarded(m), guarded(v)
    for k in range(20):
        g = R.adam_case(n, first + k, seed=k)[1]
        hp, hm, hv = N(dp), N(dm), N(dv)
        ops.adam_step(dp, T(g), dm, dv, first + k)
        want, bound = R.adam64(hp, g, hm, hv, first + k), R.adam_bounds(hp, g, hm, hv, first + k)
        for name, a, b in zip('pmv', (dp, dm, dv), want):
            inside('adam', name, N(a), b, bound[name])
    assert untouched(bp, 0, n) and untouched(bm, 0, n) and untouched(bv, 0, n)


# ------------------------------------------------------------------------------------------------------------ sphere intersection
@pytest.mark.parametrize('scale', R.RAY_SCALES)
def test_sphere_far_against_float64(ops, scale):
    """closest points with pn in 0 ... 1 - 2^-23, a camera at the origin: far inside R.sphere_far_bound of float64, and the bits of
    the float32 oracle"""
    o, d = R.sphere_case(scale)
    far = N(ops.intersect_sphere(T(o), T(d)))
    want, pn = R.sphere_far64(o, d)
    assert (pn < 1).all() and np.isfinite(far).all()
    inside('sphere_far', 'far', far, want, R.sphere_far_bound(o, d))
    assert np.array_equal(far.view(np.uint32), O.intersect_sphere(o, d).view(np.uint32))
    for S in (2, 256):
        near = np.full(o.shape[0], 1e-4, f32)
        far_c, fg_z, bg_z = ops.sample_coarse(T(o), T(d), T(near), S, perturb=False)
        fg_o, bg_o = O.coarse_depths(near, O.intersect_sphere(o, d), S)
        assert np.array_equal(N(far_c).view(np.uint32), far.view(np.uint32))
        assert np.array_equal(N(fg_z).view(np.uint32), fg_o.view(np.uint32)) and np.array_equal(N(bg_z).view(np.uint32), bg_o.view(np.uint32))


@pytest.mark.parametrize('n', R.BAD_N)
def test_bad_ray_counter(ops, n):
    """k rays with pn >= 1 (one of them pn == 1 exactly): intersect_sphere raises exactly when k > 0, and sample_coarse counts every
    such ray once, not once per sample"""
    for k in sorted({0, 1, n // 2, n}):
        o, d, near, is_bad = R.bad_case(n, k)
        assert int(is_bad.sum()) == k
        if k:
            with pytest.raises(Exception, match='unit sphere'):
                ops.intersect_sphere(T(o), T(d))
        else:
            ops.intersect_sphere(T(o), T(d))
        for S in R.COARSE_S:
            bad = torch.zeros(1, dtype=torch.int32, device=dev())
            far, fg_z, bg_z = ops.sample_coarse(T(o), T(d), T(near), S, perturb=False, check=False, bad=bad)
            assert int(bad.item()) == k, (k, S)
            assert bool(torch.isfinite(fg_z[T(~is_bad)]).all())
            if k:
                with pytest.raises(Exception, match='unit sphere'):
                    ops.sample_coarse(T(o), T(d), T(near), S, perturb=False)


def test_worst_ratios_report():
    """the worst |error| / bound per kernel (and per output) over this module's run (DESIGN.md records them); every one at most 1"""
    for name in sorted(WORST):
        print('worst ratio %-44s %.3f' % (name, WORST[name]))
    assert all(v <= 1.0 for v in WORST.values())

"""CPU tests of tests/nerfpp_render_reference.py (R), the float64 restatements and bounds that tests/test_gpu_nerfpp_render_edges.py
holds the NeRF++ compositing, loss head, Adam and sphere intersection kernels to:

* the restatements agree with the float32 oracle (oracle/nerfpp_oracle.py) on ordinary inputs to float32 rounding, and the autograd
  backward with the oracle's hand-derived composite_backward;
* the calibration: the float32 implementations of the reference's arithmetic -- the oracle's compositing (nerf_forward behind stub MLPs
  that return the case's raw values) and composite_backward, loss_and_grads, intersect_sphere, float32 torch.optim.Adam -- stay inside
  every bound on every case the GPU test runs, and every constant R.C[name] is the smallest power of two that is at least four times
  the recorded worst ratio R.F32_WORST[name];
* what is exact needs no device to be exact: zero sigma, colours at 0 and 1, zero upstream gradients, masked rays, the dyadic Adam step;
* the two inspection entry points refuse bad arguments before they touch a device.

`python -m tests.test_nerfpp_render_reference` prints the measured ratios (the figures recorded in R.F32_WORST and DESIGN.md)."""
import ctypes as C
from unittest import mock

import numpy as np
import pytest

from oracle import nerfpp_oracle as O
from tests import nerfpp_render_reference as R

torch = pytest.importorskip('torch')
f32 = np.float32
LOSS_NAMES = {0: None, 1: 'mse', 2: 'l1', 3: 'kl'}


# ------------------------------------------------------------------------------------------------------------ float32 implementations
def oracle_composite(case, upstreams=()):
    """oracle.nerfpp_oracle.nerf_forward's compositing (lines 436-478) on the case's raw values: the two MLPs and depth2pts_outside are
    replaced by stubs that hand back raw_fg / raw_bg / depth_real_bg (the background flipped, as the oracle feeds its MLP), so every
    float32 operation behind them is the oracle's own.  Returns (ret, [per upstream (dout_fg, dout_bg) [n*S, 4] natural order]):
    O.composite_backward gives d rgb after the sigmoid and d |sigma|; the sigmoid's c (1 - c) and sign(sigma_raw) are applied in float32."""
    n, S = case['fg_z'].shape
    raw = {O.FG_IN: case['raw_fg'].reshape(n, S, 4), O.BG_IN: case['raw_bg'].reshape(n, S, 4)[:, ::-1]}

    def mlp(p, inp, input_ch, input_ch_viewdirs, cache=None, bf16=False):
        r = raw[input_ch].reshape(n * S, 4)
        return r[:, :3].copy(), np.abs(r[:, 3])

    def pts(ray_o, ray_d, depth):
        return np.zeros(depth.shape + (4,), f32), case['depth_real_bg'].reshape(n, S)

    cache = {}
    with mock.patch.object(O, 'mlp_forward', mlp), mock.patch.object(O, 'depth2pts_outside', pts), np.errstate(under='ignore'):
        ret = O.nerf_forward({}, np.zeros((n, 3), f32), case['ray_d'], case['fg_far'], case['fg_z'], case['bg_z'], cache=cache)
    douts = []
    for g_rgb, g_depth, g_w in upstreams:
        with np.errstate(under='ignore', over='ignore', invalid='ignore'):
            parts = O.composite_backward(cache, g_rgb, g_depth, g_w)
        out = []
        for d_rgb, d_sigma, r, flip in ((parts[0], parts[1], raw[O.FG_IN], False), (parts[2], parts[3], raw[O.BG_IN], True)):
            c = r[..., :3]
            d = np.concatenate([((d_rgb * c).astype(f32) * (f32(1) - c)).astype(f32), (d_sigma * np.sign(r[..., 3]))[..., None].astype(f32)], -1)
            out.append(np.ascontiguousarray(d[:, ::-1] if flip else d).reshape(n * S, 4))
        douts.append(tuple(out))
    return ret, douts


def oracle_loss(c, loss_type, lambda_depth, kl_sigma):
    """O.loss_and_grads as dict(loss, rgb_loss, depth_loss, g_rgb, g_depth, g_w); lambda_depth and kl_sigma as the floats a kernel gets"""
    n, S = c['fg_z'].shape
    with np.errstate(under='ignore', invalid='ignore', divide='ignore'):
        loss, rgb_loss, depth_loss, g_rgb, g_depth, g_w = O.loss_and_grads(
            c, c['fg_z'], c['fg_far'], c['rgb_gt'], c['depth_sup'], loss_type != 0, LOSS_NAMES[loss_type], f32(lambda_depth), f32(kl_sigma))
    return dict(loss=loss, rgb_loss=rgb_loss, depth_loss=0.0 if depth_loss is None else depth_loss, g_rgb=g_rgb, g_depth=g_depth,
                g_w=np.zeros((n, S), f32) if g_w is None else g_w)


def torch_adam32(p, g, m, v, step, lr=5e-4, beta1=0.9, beta2=0.999, eps=1e-8):
    """one step of float32 torch.optim.Adam (single-tensor path) from the given state; returns (p, m, v)"""
    param = torch.nn.Parameter(torch.from_numpy(p.copy()))
    param.grad = torch.from_numpy(g.copy())
    opt = torch.optim.Adam([param], lr=lr, betas=(beta1, beta2), eps=eps, foreach=False)
    opt.state[param] = dict(step=torch.tensor(float(step - 1)), exp_avg=torch.from_numpy(m.copy()), exp_avg_sq=torch.from_numpy(v.copy()))
    opt.step()
    st = opt.state[param]
    assert int(st['step']) == step
    return param.detach().numpy(), st['exp_avg'].numpy(), st['exp_avg_sq'].numpy()


def loss64_of(c, t, lam, sig):
    return R.loss64(t, lam, sig, c['rgb'], c['rgb_gt'], c['depth'], c['depth_sup'], c['fg_weights'], c['fg_z'], c['fg_dists'], c['fg_far'])


# ------------------------------------------------------------------------------------------------------------ the calibration
def measure():
    """{name: worst |error| / bound of the float32 implementations with the constant at 1} over every case of the GPU test"""
    worst = {k: 0.0 for k in R.F32_WORST}

    def note(name, got, want, bound):
        r = float(np.max(R.ratio(got, want, bound))) * R.C[name]                 # the bound functions carry C[name]: take it out again
        worst[name] = max(worst[name], r)

    for S in R.COMPOSITE_S:
        for family, n in R.composite_cases(S):
            case = R.composite_case(family, S, n)
            ups = [R.upstream(kind, S, n) for kind in R.UPSTREAM]
            ret, douts = oracle_composite(case, ups)
            want, bound = R.composite64(**case), R.composite_bounds(case)
            for k in R.RET_KEYS:
                note(k, ret[k], want[k], bound[k])
            for up, got in zip(ups, douts):
                w64, b64 = R.composite_backward64(case, *up), R.composite_backward_bounds(case, *up)
                for vol in (0, 1):
                    note('dout_rgb', got[vol][:, :3], w64[vol][:, :3], b64[vol][:, :3])
                    note('dout_sigma', got[vol][:, 3], w64[vol][:, 3], b64[vol][:, 3])
    for n, S, mask, t, lam, sig in R.loss_cases():
        c = R.loss_case(n, S, mask)
        got = oracle_loss(c, t, lam, sig)
        want, bound = loss64_of(c, t, lam, sig)
        for k in ('loss', 'rgb_loss', 'depth_loss', 'g_rgb', 'g_depth', 'g_w'):
            if np.all(np.isnan(want[k])):
                assert np.all(np.isnan(got[k]))
                continue
            note(k, got[k], want[k], bound[k])
    for n in R.ADAM_N:
        for step in R.ADAM_STEPS:
            p, g, m, v = R.adam_case(n, step)
            got = torch_adam32(p, g, m, v, step)
            want, bound = R.adam64(p, g, m, v, step), R.adam_bounds(p, g, m, v, step)
            for k, a, b in zip('pmv', got, want):
                note('adam_' + k, a, b, bound[k])
    for scale in R.RAY_SCALES:
        o, d = R.sphere_case(scale)
        note('sphere_far', O.intersect_sphere(o, d), R.sphere_far64(o, d)[0], R.sphere_far_bound(o, d))
    return worst


@pytest.fixture(scope='module')
def measured():
    return measure()


def test_float32_implementations_stay_inside_every_bound(measured):
    """the calibration, asserted with the recorded constants: four times the float32 worst ratio is at most the constant"""
    for name, worst in measured.items():
        assert 4 * worst <= R.C[name], (name, worst, R.C[name])


def test_constants_follow_the_rule():
    """C[name] = smallest power of two >= 4 F32_WORST[name], and F32_WORST holds a measurement for every bound"""
    assert set(R.C) == set(R.F32_WORST)
    for name, worst in R.F32_WORST.items():
        assert worst > 0, name
        c = R.C[name]
        assert c == 2.0 ** round(np.log2(c)) and c >= 4 * worst > c / 2, (name, worst, c)


def test_recorded_ratios_are_the_measured_ones(measured):
    """the figures in R.F32_WORST (and DESIGN.md) are this measurement (numpy's float32 exp / log may differ by an ulp between
    processors: a quarter either way still gives a constant within one power of two, which the first test then decides)"""
    for name, worst in measured.items():
        assert 0.75 * R.F32_WORST[name] <= worst <= 1.25 * R.F32_WORST[name], (name, worst, R.F32_WORST[name])


# ------------------------------------------------------------------------------------------------------------ agreement on ordinary inputs
@pytest.mark.parametrize('S', (2, 64, 192))
def test_restatements_agree_with_the_oracle_on_ordinary_inputs(S):
    case = R.composite_case('general', S, 5)
    up = R.upstream('random', S, 5)
    ret, douts = oracle_composite(case, [up])
    want = R.composite64(**case)
    for k in R.RET_KEYS:
        np.testing.assert_allclose(ret[k], want[k], rtol=2e-5, atol=2e-6, err_msg=k)
    # the autograd backward against the hand-derived Appendix-A backward of the oracle
    w64 = R.composite_backward64(case, *up)
    for vol in (0, 1):
        scale = np.abs(w64[vol]).max(0)
        assert np.all(np.abs(douts[0][vol] - w64[vol]) <= 2e-5 * scale + 1e-30), vol


def test_loss_adam_and_sphere_restatements_agree_with_the_oracle():
    c = R.loss_case(257, 64, 'mixed', edges=False)
    for t in range(4):
        got, (want, _) = oracle_loss(c, t, 0.3, 0.01), loss64_of(c, t, 0.3, 0.01)
        for k in got:
            np.testing.assert_allclose(got[k], want[k], rtol=2e-5, atol=1e-9, err_msg='%s type %d' % (k, t))
        assert want['n_valid'] == (0 if t == 0 else int((c['depth_sup'] > 0).sum()) if t < 3 else
                                   int(((c['depth_sup'] > 0) & (c['depth_sup'] < c['fg_far'])).sum()))
    p, g, m, v = (np.random.RandomState(k).randn(1000).astype(f32) * s for k, s in enumerate((0.1, 1e-3, 1e-3, 1e-3)))
    v = v * v
    want = R.adam64(p, g, m, v, 10)
    po, mo, vo = p.copy(), m.copy(), v.copy()
    O.adam_step(po, g, mo, vo, 10)
    for a, b in zip((po, mo, vo), want):
        np.testing.assert_allclose(a, b, rtol=1e-5, atol=1e-9)
    for step in R.ADAM_STEPS:
        assert R.adam_constant_distance(step) <= R.ADAM_CONSTANT_DISTANCE
    o, d = R.sphere_case(1.0)
    np.testing.assert_allclose(O.intersect_sphere(o, d), R.sphere_far64(o, d)[0], rtol=1e-5, atol=1e-6)


# ------------------------------------------------------------------------------------------------------------ exact without a device
def test_exact_cases_are_exact_in_float64():
    for S in (3, 65):
        case = R.composite_case('zero', S, 4)
        out = R.composite64(**case)
        n = 4
        zero_fg = case['raw_fg'][:, 3].reshape(n, S) == 0
        assert zero_fg[::2].all() and np.all(out['fg_weights'][zero_fg] == 0)
        assert np.all(out['bg_weights'][(case['raw_bg'][:, 3].reshape(n, S) == 0)[:, ::-1]] == 0)
        # a ray without density: every q is 1 + TINY, the product of S of them is bg_lambda
        np.testing.assert_allclose(out['bg_lambda'][::2], (1 + R.TINY) ** S, rtol=1e-15)
        up = R.upstream('random', S, n)
        d_fg, d_bg = R.composite_backward64(case, *up)
        b_fg, b_bg = R.composite_backward_bounds(case, *up)
        for d, b, raw in ((d_fg, b_fg, case['raw_fg']), (d_bg, b_bg, case['raw_bg'])):
            assert np.all(d[raw[:, 3] == 0, 3] == 0) and np.all(b[raw[:, 3] == 0, 3] == 0)      # sign(0) = 0: exact, no bound
        # mirrored sigma: same forward, d sigma_raw negated
        mir = R.mirrored(case)
        out_m = R.composite64(**mir)
        assert all(np.array_equal(out[k], out_m[k]) for k in R.RET_KEYS)
        m_fg, m_bg = R.composite_backward64(mir, *up)
        assert np.array_equal(m_fg[:, 3], -d_fg[:, 3]) and np.array_equal(m_bg[:, :3], d_bg[:, :3])
        # colours at 0 and 1: d rgb exactly 0 there; zero upstream: everything 0
        ends = R.composite_case('colour_ends', S, n)
        e_fg, e_bg = R.composite_backward64(ends, *up)
        bb = R.composite_backward_bounds(ends, *up)
        for d, b, raw in ((e_fg, bb[0], ends['raw_fg']), (e_bg, bb[1], ends['raw_bg'])):
            at_end = (raw[:, :3] == 0) | (raw[:, :3] == 1)
            assert at_end.any() and np.all(d[:, :3][at_end] == 0) and np.all(b[:, :3][at_end] == 0)
        z_fg, z_bg = R.composite_backward64(case, *R.upstream('zero', S, n))
        assert not z_fg.any() and not z_bg.any()
    # the saturating family: float64 is finite everywhere and weights behind 8 saturated samples are below the smallest float32
    sat = R.composite_case('saturating', 64, 9)
    out = R.composite64(**sat)
    assert all(np.isfinite(v).all() for v in out.values()) and (out['fg_weights'] < R.DENORM).any()


def test_masked_rays_and_empty_masks_in_float64():
    c = R.loss_case(257, 65, 'mixed')
    want, bound = loss64_of(c, 3, 1.0, 0.01)
    outside = ~((c['depth_sup'] > 0) & (c['depth_sup'] < c['fg_far']))
    assert outside.any() and not want['g_w'][outside].any() and not bound['g_w'][outside].any()
    assert (c['depth_sup'] == c['fg_far']).any() and (c['depth_sup'] == np.nextafter(c['fg_far'], f32(0))).any()
    for t in (1, 2):
        want, _ = loss64_of(R.loss_case(5, 2, 'none'), t, 0.3, 0.01)
        assert np.isnan(want['loss']) and np.isnan(want['depth_loss']) and want['n_valid'] == 0 and not want['g_depth'].any()
    far = R.kl_far_case(5, 64, 1e-2)
    want, bound = loss64_of(far, 3, 1.0, 1e-2)
    assert want['n_valid'] == 5 and np.abs(want['g_w']).max() < R.DENORM and abs(want['depth_loss']) < R.DENORM


def test_dyadic_adam_step_is_exact():
    p, g, m, v, kw = R.adam_dyadic_case(257)
    got = torch_adam32(p, g, m, v, kw['step'], kw['lr'], kw['beta1'], kw['beta2'], kw['eps'])
    want = R.adam64(p, g, m, v, kw['step'], kw['lr'], kw['beta1'], kw['beta2'], kw['eps'])
    exact = R.adam64(p, g, m, v, kw['step'], kw['lr'], kw['beta1'], kw['beta2'], kw['eps'], exact=True)
    for a, b, c in zip(got, want, exact):
        assert np.array_equal(R.f64(a), b) and np.array_equal(b, c)
    assert np.array_equal(want[0], R.f64(p) - np.sign(g) * 2.0 ** -11)
    # a first step from m == 0: one rounding of an exact product, the bits of float32 torch.optim.Adam
    p, g, m, v = R.adam_case(70001, 1)
    exact, normal = R.adam_first_step_m(g)
    assert normal.sum() > 30000 and np.array_equal(torch_adam32(p, g, m, v, 1)[1][normal].view(np.uint32), exact[normal].view(np.uint32))
    wrong = (R.f64(g) * float(f32(1) - f32(0.9))).astype(f32)                  # 1.f - beta1 formed in float: other bits
    assert (wrong[normal].view(np.uint32) != exact[normal].view(np.uint32)).mean() > 0.5


# ------------------------------------------------------------------------------------------------------------ refusals
def test_composite_entry_points_refuse_before_they_touch_a_device():
    """n_rays <= 0, n_samples < 2 or > NERFPP_MAX_SAMPLES, null pointers; only g_fg_weights may be null, and g_rgb / g_depth when the
    head is fused.  The pointers are never dereferenced: 64 stands for 'not null'."""
    from outdoor_nerf_depth_amd import _lib as L
    lib = L.lib()
    assert lib.nerfpp_abi_version() == L.ABI_VERSION
    P = 64

    def refused(fn, args, words):
        assert getattr(lib, fn)(None, *args) == 1                                   # NERFPP_ERR_ARG
        msg = lib.nerfpp_last_error().decode()
        assert msg.startswith(fn + ': requirement failed: ') and words in msg, msg

    fwd = lambda n=4, S=64, null=None: [n, S] + [None if k == null else P for k in range(17)]
    for n, S in ((0, 64), (-1, 64), (4, 1), (4, 0), (4, L.MAX_SAMPLES + 1)):
        refused('nerfpp_composite_forward', fwd(n, S), 'sizes')
    for k in range(17):
        refused('nerfpp_composite_forward', fwd(null=k), 'inputs' if k < 7 else 'outputs')

    def bwd(n=4, S=64, null=(), fused=0, loss_type=0, kl_sigma=0.01, head_null=()):
        ptrs = [None if k in null else P for k in range(12)]                        # 7 inputs, g_rgb, g_depth, g_fg_weights, dout_fg, dout_bg
        head = [None if k in head_null else P for k in range(4)]                    # rgb, depth, rgb_gt, depth_sup
        return [n, S] + ptrs + [fused, loss_type, 0.1, kl_sigma] + head

    for n, S in ((0, 64), (-1, 64), (4, 1), (4, L.MAX_SAMPLES + 1)):
        refused('nerfpp_composite_backward', bwd(n, S), 'sizes')
    for k in range(7):
        refused('nerfpp_composite_backward', bwd(null=(k,)), 'inputs')
    for k in (10, 11):
        refused('nerfpp_composite_backward', bwd(null=(k,)), 'outputs')
    for k in (7, 8):
        refused('nerfpp_composite_backward', bwd(null=(k,)), 'dL/d rgb and dL/d depth (or fused_loss)')
    # the fused fields, exactly as nerfpp_level_backward checks them
    refused('nerfpp_composite_backward', bwd(fused=1, loss_type=4), 'loss_type in 0..3')
    refused('nerfpp_composite_backward', bwd(fused=1, loss_type=-1), 'loss_type in 0..3')
    refused('nerfpp_composite_backward', bwd(fused=1, head_null=(0,)), 'fused loss head needs rgb and rgb_gt')
    refused('nerfpp_composite_backward', bwd(fused=1, head_null=(2,)), 'fused loss head needs rgb and rgb_gt')
    refused('nerfpp_composite_backward', bwd(fused=1, loss_type=1, head_null=(1,)), 'fused depth loss needs depth and depth_sup')
    refused('nerfpp_composite_backward', bwd(fused=1, loss_type=2, head_null=(3,)), 'fused depth loss needs depth and depth_sup')
    refused('nerfpp_composite_backward', bwd(fused=1, loss_type=3, kl_sigma=0.0), 'kl_sigma > 0')
    a = L.BackwardArgs()
    a.n_rays, a.n_samples, a.precision, a.fused_loss, a.loss_type = 4, 64, 1, 1, 3
    for k in ('ray_d', 'fg_far', 'fg_z', 'bg_z', 'packed', 'workspace', 'tables', 'grads', 'params', 'rgb', 'rgb_gt', 'depth', 'depth_sup'):
        setattr(a, k, P)
    assert lib.nerfpp_level_backward(None, C.byref(a)) == 1
    assert lib.nerfpp_last_error().decode() == 'nerfpp_level_backward: requirement failed: kl_sigma > 0'


if __name__ == '__main__':
    for name, worst in measure().items():
        print('%-12s worst %.4g  ->  C = %g' % (name, worst, R.pow2_at_least(4 * worst)))

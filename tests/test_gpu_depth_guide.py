"""GPU: depth-guided fine sampling of the NeRF++ path (depthguide_merge, csrc/depthguide_kernels.hip) against
tests/depth_guide_reference.py, in the trainer, in render_single_image and through the CLI.

Gates of the kernel tests.  `mode` is exact.  A ray in mode 0 or 2 involves only products, sums, compares and correctly rounded
float64 divisions of the float32 inputs: `guide` and `z_merged` are bit-equal to the reference.  A ray in mode 1 adds a float64 square
root, and its sums are formed in the kernel's order by the reference too: every element within one float32 spacing of the reference
(np.spacing(np.float32(|ref|))), since a last-bit difference of the square root can move the one final rounding by at most that.
That was the gate to start from; on the MI355X every mode-1 element came out bit-equal as well, so the gate is tightened to equality
for all three modes (the spacing figure is still printed first).
Every case with n >= 3 holds one ray of each planted kind (tests/depth_guide_reference.py: KINDS); a call of 3 rays cannot hold
twelve, so the case of n = 3 is four calls of 3 rays.  A deviation of exactly 0 with min_std = 0 fails the mask's s_eff > 0 and guides
no ray (kind std_zero, mode 1); the ray whose G samples all tie at p is the one with a deviation of 1e-30 (std_tiny, and
prior_on_sample, whose p is bit-equal to one of zin).  Every figure is printed before it is asserted.
"""
import logging
import os
import re
import subprocess
import sys

import numpy as np
import pytest

torch = pytest.importorskip('torch')
pytestmark = pytest.mark.gpu

from tests import depth_guide_reference as R                                # noqa: E402
from tests.test_gpu_mip360 import T, N, dev                                # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(1, 1, 1), (2, 3, 2), (64, 64 + 63, 65), (64, 64 + 64, 64), (65, 128, 63), (64, 384, 128)]
RAYS = (1, 3, 257)
# the training-effect test: the G of the sweep {8, 16, 24} that the test runs
TRAIN_G, TRAIN_STEPS, TRAIN_SEEDS = 16, 200, (0, 1, 2, 3)


@pytest.fixture(scope='module')
def DG():
    dev()
    from outdoor_nerf_depth_amd import depth_guide
    return depth_guide


_drawn = {}


def case(n, shape):
    """the calls of the case (n, S_prev, S_in, G) with their references, drawn once and shared"""
    key = (n,) + tuple(shape)
    if key not in _drawn:
        calls = R.draw(1000 * n + sum(shape), n, *shape)
        for c in calls:
            c['ref'] = R.depth_guide(c['zp'], c['wp'], c['zin'], c['lo'], c['hi'], shape[2], prior=c['p'], prior_std=c['s'], v=c['v'])
        _drawn[key] = calls
    return _drawn[key]


def call(DG, c, G, v='given', **kw):
    v = T(c['v']) if isinstance(v, str) else v
    z, mode, guide = DG.depth_guide(T(c['zp']), T(c['wp']), T(c['zin']), T(c['lo']), T(c['hi']), G, prior=T(c['p']), prior_std=T(c['s']),
                                    v=v, return_guide=True, **kw)
    torch.cuda.synchronize()
    return N(z), mode.cpu().numpy(), N(guide)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def check(ref, z, mode, guide, tag):
    """the gates of the module docstring; returns the worst mode-1 difference in float32 spacings"""
    assert mode.dtype == np.int32
    np.testing.assert_array_equal(mode, ref['mode'])
    exact = ref['mode'] != 1
    assert (bits(guide)[exact] == bits(ref['guide'])[exact]).all(), tag
    assert (bits(z)[exact] == bits(ref['z_merged'])[exact]).all(), tag
    worst = 0.0
    for got, want in ((guide[~exact], ref['guide'][~exact]), (z[~exact], ref['z_merged'][~exact])):
        if got.size:
            nan = np.isnan(want)
            assert (np.isnan(got) == nan).all(), tag
            ulp = np.abs(got.astype(np.float64) - want)[~nan] / np.spacing(np.abs(want[~nan]).astype(np.float32)).astype(np.float64)
            worst = max(worst, float(ulp.max()) if ulp.size else 0.0)
    print('%s: modes %s; %d mode-1 rays, worst difference %.3f float32 spacings' % (tag, np.bincount(mode, minlength=3).tolist(),
                                                                                   (~exact).sum(), worst))
    assert worst <= 1.0, tag
    # tightened: the MI355X's float64 square root returned the reference's bits in every case of this file (worst difference 0
    # spacings over 1 000 mode-1 rays), so mode 1 is held to equality as well
    assert (bits(guide) == bits(ref['guide'])).all() and (bits(z) == bits(ref['z_merged'])).all(), tag
    return worst


# ------------------------------------------------------------------------------------------------ 1. the kernel
@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: '%d-%d-%d' % s)
@pytest.mark.parametrize('n', RAYS)
def test_parity_with_the_reference(DG, n, shape):
    calls = case(n, shape)
    kinds = [k for c in calls for k in c['kinds'] if k]
    assert kinds == (list(R.KINDS) if n >= 3 else [])
    for i, c in enumerate(calls):
        for r, k in enumerate(c['kinds']):
            if k:
                assert c['ref']['mode'][r] == R.EXPECTED_MODE[k], k
        z, mode, guide = call(DG, c, shape[2])
        check(c['ref'], z, mode, guide, '(n %d, S_prev %d, S_in %d, G %d) call %d' % ((n,) + tuple(shape) + (i,)))


def test_min_std_floors_both_gaussians(DG):
    c = dict(case(257, (65, 128, 63))[0])
    ref = R.depth_guide(c['zp'], c['wp'], c['zin'], c['lo'], c['hi'], 63, prior=c['p'], prior_std=c['s'], v=c['v'], min_std=0.3)
    assert (ref['mode'] != c['ref']['mode']).any()                               # the ray of deviation 0 is guided now
    check(ref, *call(DG, c, 63, min_std=0.3), tag='min_std 0.3')


def test_no_prior_and_a_constant_deviation(DG):
    c = case(257, (64, 128, 64))[0]
    z, mode, guide = DG.depth_guide(T(c['zp']), T(c['wp']), T(c['zin']), T(c['lo']), T(c['hi']), 64, v=T(c['v']), return_guide=True)
    ref = R.depth_guide(c['zp'], c['wp'], c['zin'], c['lo'], c['hi'], 64, v=c['v'])
    assert not (ref['mode'] == 0).any()
    check(ref, N(z), mode.cpu().numpy(), N(guide), 'no prior')
    z, mode, guide = DG.depth_guide(T(c['zp']), T(c['wp']), T(c['zin']), T(c['lo']), T(c['hi']), 64, prior=T(c['p']), std_const=0.07, v=T(c['v']),
                                    return_guide=True)
    ref = R.depth_guide(c['zp'], c['wp'], c['zin'], c['lo'], c['hi'], 64, prior=c['p'], std_const=0.07, v=c['v'])
    assert (ref['mode'] == 0).sum() > 100
    check(ref, N(z), mode.cpu().numpy(), N(guide), 'constant deviation')


def test_same_call_twice_is_bit_identical(DG):
    for n, shape in ((257, (64, 384, 128)), (257, (64, 127, 65)), (3, (2, 3, 2))):
        for c in case(n, shape):
            a, b = call(DG, c, shape[2]), call(DG, c, shape[2])
            for x, y in zip(a, b):
                assert (x.view(np.uint32) == y.view(np.uint32)).all(), (n, shape)


def test_rng_mode_is_the_explicit_call_on_stream_5(DG):
    from outdoor_nerf_depth_amd import ops
    from oracle.nerfpp_oracle import philox_uniform
    for n, shape, seed, step in ((257, (64, 128, 64), 777, 1), (3, (65, 128, 63), (1 << 40) + 5, 123456)):
        G = shape[2]
        c = case(n, shape)[0]
        v = ops.rng_uniform(seed, step, DG.RNG_STREAM, (n, G), dev())
        assert (N(v).ravel() == philox_uniform(seed, step, 5, n * G)).all() and (N(v) < 1).all() and N(v).std() > 0.2
        given, drawn = call(DG, c, G, v=v), call(DG, c, G, v=None, rng=(seed, step))
        for x, y in zip(given, drawn):
            assert (x.view(np.uint32) == y.view(np.uint32)).all(), (n, shape)
        other = call(DG, c, G, v=None, rng=(seed, step + 1))
        assert (other[2] != drawn[2]).any()
    with pytest.raises(DG.DepthGuideError, match='v and rng'):
        DG.depth_guide(T(c['zp']), T(c['wp']), T(c['zin']), T(c['lo']), T(c['hi']), G, v=v, rng=(1, 1))


def test_deterministic_mode_is_v_one_half(DG):
    for n, shape in ((257, (64, 128, 64)), (3, (1, 1, 1))):
        c = case(n, shape)[0]
        half = call(DG, c, shape[2], v=T(np.full(c['v'].shape, 0.5, np.float32)))
        det = call(DG, c, shape[2], v=None)
        for x, y in zip(half, det):
            assert (x.view(np.uint32) == y.view(np.uint32)).all(), (n, shape)


# ------------------------------------------------------------------------------------------------ 2. the trainer
def _batch(n, seed=3, std=True):
    from outdoor_nerf_depth_amd.synthetic import SyntheticKitti
    rs = np.random.RandomState(seed)
    b = SyntheticKitti().random_batch(n, rs)
    b['depth_sup'] = np.where(rs.rand(n) < 0.7, rs.uniform(0.02, 0.2, n), 0).astype(np.float32)
    if std:
        b['depth_std'] = (b['depth_sup'] * rs.uniform(0.01, 0.2, n)).astype(np.float32)
    return {k: T(np.asarray(v, np.float32)) for k, v in b.items() if isinstance(v, np.ndarray)}


def _trainer(cascade=(16, 32), **kw):
    from outdoor_nerf_depth_amd.trainer import NerfppTrainer
    from outdoor_nerf_depth_amd.model import init_level_params
    return NerfppTrainer(dev(), precision=2, cascade_samples=cascade, level_params=init_level_params(2), **kw)


class Tap(object):
    """an engine's forward, keeping the depths it got and what it returned (clones)"""

    def __init__(self, eng):
        self.fn, self.calls = eng.forward, []
        eng.forward = self

    def __call__(self, ray_o, ray_d, far, fg_z, bg_z, **kw):
        ret = self.fn(ray_o, ray_d, far, fg_z, bg_z, **kw)
        self.calls.append(dict(far=far.clone(), fg_z=fg_z.clone(), bg_z=bg_z.clone(), ret={k: v.clone() for k, v in ret.items()}))
        return ret


def _same(a, b, what):
    assert a.shape == b.shape and (bits(N(a)) == bits(N(b))).all(), what


@pytest.mark.parametrize('kind,with_std', [('rgbonly', True), ('mse', True), ('mse', False)])
def test_replayed_step_is_the_hand_composed_sequence(DG, kind, with_std):
    """a step with G = 12 of 32 on replayed uniforms: level 1's depths are sample_fine(S1 - G), sample_fine(S1) and the one new call
    on the previous level's depths and weights, and its forward sees exactly those; whatever the depth loss is"""
    from outdoor_nerf_depth_amd import ops
    n, S0, S1, G = 64, 16, 32, 12
    batch = _batch(n, std=with_std)
    rs = np.random.RandomState(11)
    U_ = lambda *s: T(rs.rand(*s).astype(np.float32))
    uniforms = dict(t_fg=U_(n, S0), t_bg=U_(n, S0), u_fg=U_(n, S1 - G), u_bg=U_(n, S1), v_fg=U_(n, G))
    kw = dict(use_depth=kind != 'rgbonly', depth_loss_type='mse' if kind == 'rgbonly' else kind, lambda_depth=0.1, depth_guide_samples=G,
              depth_guide_min_std=0.001, **({} if with_std else dict(depth_guide_std=0.02)))
    tr = _trainer(**kw)
    taps = [Tap(e) for e in tr.engines]
    tr.train_step(batch, uniforms=uniforms)
    tr.flush()
    torch.cuda.synchronize()
    l0, l1 = taps[0].calls[0], taps[1].calls[0]
    far, fg0, bg0 = ops.sample_coarse(batch['ray_o'], batch['ray_d'], batch['min_depth'], S0, uniforms['t_fg'], uniforms['t_bg'])
    _same(fg0, l0['fg_z'], 'level 0 fg_z')
    z_in = ops.sample_fine(fg0, l0['ret']['fg_weights'], S1 - G, u=uniforms['u_fg'])
    bg1 = ops.sample_fine(bg0, l0['ret']['bg_weights'], S1, u=uniforms['u_bg'])
    fg1, mode = DG.depth_guide(fg0, l0['ret']['fg_weights'], z_in, batch['min_depth'], far, G, prior=batch['depth_sup'],
                               prior_std=batch.get('depth_std'), std_const=0.02, min_std=0.001, v=uniforms['v_fg'])
    _same(fg1, l1['fg_z'], 'level 1 fg_z')
    _same(bg1, l1['bg_z'], 'level 1 bg_z')
    z = N(l1['fg_z'])
    assert z.shape == (n, S0 + S1) and (np.diff(z, axis=-1) >= 0).all()
    assert (tr.last_depth_guide[0] is None) and (tr.last_depth_guide[1].cpu().numpy() == mode.cpu().numpy()).all()
    guided = (mode == 0).float().mean().item()
    print('%s, depth_std %s: %.3f of the rays guided by the prior' % (kind, with_std, guided))
    assert 0.5 < guided < 0.9                                                     # 70 % of the batch has a prior
    # ... then forward: a second trainer from the same initial state returns the same level-1 rendering for those depths
    fresh = _trainer(**kw)
    ret = fresh.engines[1].forward(batch['ray_o'], batch['ray_d'], far, fg1, bg1, training=True)
    for k in ('rgb', 'depth', 'fg_weights'):
        _same(ret[k], l1['ret'][k], 'level 1 ' + k)


def test_a_prior_without_a_deviation_needs_the_constant(DG):
    tr = _trainer(use_depth=False, depth_guide_samples=8)
    with pytest.raises(ValueError, match='depth prior without depth_std'):
        tr.train_step(_batch(64, std=False))
    b = _batch(64, std=False)
    del b['depth_sup']                                                           # no prior at all: every ray in mode 1 or 2
    tr = _trainer(use_depth=False, depth_guide_samples=8)
    tr.train_step(b)
    tr.flush()
    torch.cuda.synchronize()
    assert (tr.last_depth_guide[1] > 0).all()


def test_rng_and_torch_rng_steps_run_and_differ_from_off(DG):
    batch = _batch(64)
    out = {}
    for name, kw in (('off', {}), ('rng', dict(depth_guide_samples=8)), ('torch', dict(depth_guide_samples=8, torch_rng=True))):
        tr = _trainer(use_depth=True, depth_loss_type='mse', lambda_depth=0.1, **kw)
        taps = [Tap(e) for e in tr.engines]
        torch.manual_seed(5)
        sc = [N(s) for s in tr.train_step(batch)]
        tr.flush()
        torch.cuda.synchronize()
        out[name] = (sc, N(taps[1].calls[0]['fg_z']))
        assert np.isfinite(sc[1]).all() and out[name][1].shape == (64, 48) and (np.diff(out[name][1], axis=-1) >= 0).all()
    assert (out['rng'][1] != out['off'][1]).any() and (out['rng'][0][0] == out['off'][0][0]).all()       # level 0 is untouched


def test_off_is_the_trainer_without_it(DG, monkeypatch, tmp_path):
    monkeypatch.setattr(DG, '_lib', None)
    monkeypatch.setattr(DG, 'LIB_PATH', str(tmp_path / 'libdepthguide_hip.so'))
    batch = _batch(64)
    a, b = _trainer(use_depth=False), _trainer(use_depth=False, depth_guide_samples=0)
    assert b.depth_guide is None and b.depth_guide_samples == 0
    for tr in (a, b):
        tr.out = [N(s) for s in tr.train_step(batch)]
        tr.flush()
        torch.cuda.synchronize()
    for x, y in zip(a.out + [N(g) for g in a.grads], b.out + [N(g) for g in b.grads]):
        assert (bits(x) == bits(y)).all()
    assert b.last_depth_guide is None and DG._lib is None
    with pytest.raises(DG.DepthGuideError, match='libdepthguide_hip.so not found'):
        _trainer(use_depth=False, depth_guide_samples=8).train_step(batch)
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ 3. rendering
def test_render_single_image_composes_the_same_calls_per_chunk(DG):
    """an 8 x 10 frame, cascade (8, 16), G = 8, chunks of 32 rays (the last one ragged): level 1 of every chunk is the deterministic
    composition, without a prior"""
    from outdoor_nerf_depth_amd import ops
    from outdoor_nerf_depth_amd.ddp_train_nerf import render_single_image
    from outdoor_nerf_depth_amd.data_loader_split import synthetic_ray_samplers
    sampler = synthetic_ray_samplers('test', 1, 'gt', 20, 8, 10)[0]
    S0, S1, G, chunk = 8, 16, 8, 32
    tr = _trainer(cascade=(S0, S1), use_depth=False, depth_guide_samples=G, depth_guide_min_std=0.002)
    out = render_single_image(0, 1, tr, sampler, chunk, keep_dists=False)
    off = render_single_image(0, 1, _trainer(cascade=(S0, S1), use_depth=False), sampler, chunk, keep_dists=False)
    b = sampler.get_all()
    rgb, depth = [], []
    for s in range(0, 80, chunk):
        o, d, md = (T(np.ascontiguousarray(b[k][s:s + chunk])) for k in ('ray_o', 'ray_d', 'min_depth'))
        far, fg_z, bg_z = ops.sample_coarse(o, d, md, S0, perturb=False)
        r0 = tr.engines[0].forward(o, d, far, fg_z, bg_z)
        z_in = ops.sample_fine(fg_z, r0['fg_weights'], S1 - G, det=True)
        bg1 = ops.sample_fine(bg_z, r0['bg_weights'], S1, det=True)
        fg1, mode = DG.depth_guide(fg_z, r0['fg_weights'], z_in, md, far, G, min_std=0.002)
        assert (mode > 0).all() and fg1.shape[1] == S0 + S1
        r1 = tr.engines[1].forward(o, d, far, fg1, bg1)
        rgb.append(N(r1['rgb']))
        depth.append(N(r1['depth']))
    torch.cuda.synchronize()
    assert (bits(out[1]['rgb'].numpy().reshape(-1, 3)) == bits(np.concatenate(rgb))).all()
    assert (bits(out[1]['depth'].numpy().reshape(-1)) == bits(np.concatenate(depth))).all()
    assert (bits(out[0]['rgb'].numpy()) == bits(off[0]['rgb'].numpy())).all() and (out[1]['rgb'].numpy() != off[1]['rgb'].numpy()).any()


# ------------------------------------------------------------------------------------------------ 4. it does what it is for
def noisy_batch(scene, frame, pix, rs):
    """a batch of the dense-prior scene whose prior carries Gaussian noise of known standard deviation -- 20 % of the depth at a
    third of the pixels, 1 % elsewhere (the noise of test_gpu_depth_gnll's noisy scene) -- with that deviation as depth_std; depth_gt
    stays the true depth"""
    b = scene.batch(frame, pix)
    share = np.where(scene._pixel_hash(frame + 31337, pix) < 1.0 / 3.0, 0.2, 0.01)
    true = b['depth_gt'].astype(np.float64)
    b['depth_sup'] = np.where(true > 0, np.maximum(true * (1.0 + share * rs.randn(len(pix))), 1e-4), 0).astype(np.float32)
    b['depth_std'] = np.where(true > 0, share * true, 0).astype(np.float32)
    return {k: T(np.asarray(v, np.float32)) for k, v in b.items() if isinstance(v, np.ndarray)}


def _held_out(tr, batch):
    """a deterministic forward of both levels on `batch`, sampled as a render samples -> (mean |depth - true depth| over the rays that
    have one, PSNR)"""
    from outdoor_nerf_depth_amd import ops
    tr.flush()
    S0, S1 = tr.cascade_samples
    far, fg_z, bg_z = ops.sample_coarse(batch['ray_o'], batch['ray_d'], batch['min_depth'], S0, perturb=False)
    ret = tr.engines[0].forward(batch['ray_o'], batch['ray_d'], far, fg_z, bg_z)
    if tr.depth_guide_samples > 0:
        fg_z, bg_z, _ = tr.depth_guide.fine_level(fg_z, ret['fg_weights'], bg_z, ret['bg_weights'], S1, tr.depth_guide_samples,
                                                  batch['min_depth'], far, min_std=tr.depth_guide_min_std, det=True)
    else:
        fg_z, bg_z = ops.sample_fine_pair(fg_z, ret['fg_weights'], bg_z, ret['bg_weights'], S1, det=True)
    ret = tr.engines[1].forward(batch['ray_o'], batch['ray_d'], far, fg_z, bg_z)
    torch.cuda.synchronize()
    mse = float(((N(ret['rgb']).astype(np.float64) - N(batch['rgb'])) ** 2).mean())
    gt = N(batch['depth_gt']).astype(np.float64)
    return float(np.abs(N(ret['depth']) - gt)[gt > 0].mean()), -10 * np.log10(mse)


def train_arm(seed, G, steps=TRAIN_STEPS, n_rays=256):
    """`steps` steps of 256 rays with the mse depth loss, cascade (16, 32), from the initial state and the batches that `seed` fixes"""
    from outdoor_nerf_depth_amd.synthetic import SyntheticKitti
    scene = SyntheticKitti(depth_sup_type='mono_crop')
    rs = np.random.RandomState(100 + seed)
    tr = _trainer(use_depth=True, depth_loss_type='mse', lambda_depth=0.1, seed=777 + seed, depth_guide_samples=G)
    for _ in range(steps):
        frame, pix = int(rs.randint(0, scene.n_train())), rs.randint(0, scene.H * scene.W, n_rays)
        tr.train_step(noisy_batch(scene, frame, pix, rs))
    hs = np.random.RandomState(999)
    return _held_out(tr, noisy_batch(scene, int(hs.randint(0, scene.n_train())), hs.choice(scene.H * scene.W, 1024, replace=False), hs))


def paired(G, seeds=TRAIN_SEEDS, steps=TRAIN_STEPS):
    """-> rows [seed] = (off depth error, off PSNR, on depth error, on PSNR), printed"""
    rows = []
    for seed in seeds:
        off, on = train_arm(seed, 0, steps), train_arm(seed, G, steps)
        print('G %d seed %d: off depth error %.6f psnr %.3f | on depth error %.6f psnr %.3f' % ((G, seed) + off + on))
        rows.append(off + on)
    return np.asarray(rows)


def summary(rows, G):
    """-> (mean, standard error) of the paired differences off - on of the depth error and on - off of the PSNR, printed"""
    out = []
    for name, d in (('depth error, off - on', rows[:, 0] - rows[:, 2]), ('PSNR, on - off', rows[:, 3] - rows[:, 1])):
        se = d.std(ddof=1) / np.sqrt(len(d))
        print('G %d: %s = %.6f +- %.6f (standard error of %d paired differences) = %.1f standard errors' % (G, name, d.mean(), se, len(d), d.mean() / se))
        out.append((d.mean(), se))
    print('G %d: means over seeds: off depth error %.6f psnr %.3f | on depth error %.6f psnr %.3f' % ((G,) + tuple(rows.mean(0))))
    return out


def test_guided_samples_on_noisy_priors(DG):
    """The dense synthetic prior with per-pixel Gaussian noise of known standard deviation (20 % of the depth at a third of the
    pixels, 1 % elsewhere), the mse depth loss and the prior's own deviation for the guide; 200 steps of 256 rays, cascade (16, 32),
    four seeds; both arms of a seed start from the same state and see the same batches.  One fixed held-out batch of 1024 rays is
    scored by a deterministic forward that samples as a render does: the mean |depth - true depth| and the PSNR.
    Measured on an MI355X (the sweep of DESIGN 9.12), paired differences over the seeds, in standard errors: depth error off - on
    G = 8: 0.0217 +- 0.0127 (1.7), G = 16: 0.327 +- 0.331 (1.0), G = 24: 0.338 +- 0.338 (1.0); PSNR on - off -0.03 +- 0.19, +0.26 +- 0.25,
    +0.19 +- 0.13 dB.  No G lowers the depth error by 3 standard errors (the scene's depth is a per-pixel hash that no held-out ray
    can know, and three of four seeds differ by less than 0.02), so no gain is claimed and the gate is the other one: at G = 16 the
    on arm is no worse than the off arm by more than 2 standard errors, in depth error and in PSNR."""
    (d_depth, se_depth), (d_psnr, se_psnr) = summary(paired(TRAIN_G), TRAIN_G)
    assert d_depth >= -2 * se_depth, (d_depth, se_depth)
    assert d_psnr >= -2 * se_psnr, (d_psnr, se_psnr)


# ------------------------------------------------------------------------------------------------ 5. CLI
CLI = ['--basedir', None, '--synthetic', '--synthetic_hw', '24,32', '--synthetic_frames', '20', '--cascade_samples', '16,16', '--sample_every', '2',
       '--world_size', '1', '--N_rand_override', '128', '--i_weights', '100', '--i_test', '100', '--i_print', '1', '--N_iters', '3']


def test_cli_logs_the_share_of_guided_rays(tmp_path):
    dev()
    from outdoor_nerf_depth_amd import ddp_train_nerf as T_
    argv = ['--expname', 'guide', '--depth_guide_samples', '8', '--depth_guide_min_std', '0.05', '--depth_sup_type', 'mono_crop'] + CLI
    argv[argv.index('--basedir') + 1] = str(tmp_path)
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
    assert 'depth_guide_samples = 8' in (tmp_path / 'guide' / 'args.txt').read_text()
    found = re.findall(r'step: (\d+) .*?level_1/guided: ([-\d.e+naif]+)', text)
    print('ddp_train_nerf with guided samples: %s' % found)
    assert [int(f[0]) for f in found] == [0, 1, 2], text[-2000:]
    share = np.asarray([float(f[1]) for f in found])
    assert (share > 0).all() and (share <= 1).all()                              # the dense synthetic prior leaves the top rows out
    assert 'level_0/guided' not in text


def test_cli_without_the_flag_loads_nothing_of_it(tmp_path):
    """a fresh process: three steps of ddp_train_nerf without the flag, then neither the module nor the library is in the process"""
    argv = ['--expname', 'plain'] + CLI
    argv[argv.index('--basedir') + 1] = str(tmp_path)
    code = ('import sys\n'
            'from outdoor_nerf_depth_amd import ddp_train_nerf as T\n'
            'args = T.config_parser().parse_args(%r)\n'
            'T.validate_args(args)\n'
            'args.world_size = 1\n'
            'T.ddp_train_nerf(0, args)\n'
            "assert not [m for m in sys.modules if 'depth_guide' in m], [m for m in sys.modules if 'depth_guide' in m]\n"
            "maps = open('/proc/self/maps').read()\n"
            "assert 'libnerfpp_hip.so' in maps and 'libdepthguide_hip.so' not in maps\n"
            "print('clean')\n" % (argv,))
    out = subprocess.run([sys.executable, '-c', code], cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and 'clean' in out.stdout, out.stdout[-1000:] + out.stderr[-3000:]

"""GPU: the distortion and opacity regularisers on the foreground weights of the NeRF++ path (rayreg_level,
csrc/rayreg_kernels.hip) against tests/ray_reg_reference.py, in the trainer and through the CLI.

Gates of the kernel tests.  They follow from the arithmetic contract -- float64 inside, one float32 rounding on the way out: `stats`
exact; a value within 1e-6 * (the sum of the absolute values of its terms) of the float64 reference; a gradient entry (the buffer is
pre-filled and ACCUMULATED into) within 2^-23 |ideal| + 1e-12 * (the sum of the absolute values of the entry's terms) of ideal = prefill
+ float64 gradient: one float32 rounding, doubled, and float64 summation over at most 1024 + 64 additions of 2^-53 each; a row that
receives no term bit-equal to its prefill.  Every case with n >= 3 is asserted to hold a ray with tied positions (S >= 2: one sample
cannot tie), a ray of all-zero weights, a ray with hi <= lo and a ray whose weights sum to 1.  Every figure is printed before it is
asserted.
"""
import logging
import re

import numpy as np
import pytest

torch = pytest.importorskip('torch')
pytestmark = pytest.mark.gpu

from tests import ray_reg_reference as R                                   # noqa: E402
from tests.test_gpu_mip360 import T, N, dev                               # noqa: E402

SAMPLES = (1, 2, 63, 64, 65, 192, 1024)
RAYS = (1, 3, 257)
LD, LO = 0.7, 0.05                                                        # the kernel tests' lambdas
# the training-effect test's lambdas, chosen on an MI355X: the largest pair of a sweep that costs no PSNR; three times
# as much empties the foreground (opacity entropy 0.25 -> 0.01, PSNR 28.0 -> 24.7 dB)
TRAIN_LD, TRAIN_LO = 0.01, 0.001
TRAIN_STEPS, TRAIN_SEEDS = 200, (0, 1, 2, 3)


@pytest.fixture(scope='module')
def G():
    dev()
    from outdoor_nerf_depth_amd import ray_reg
    return ray_reg


_drawn = {}


def case(n, S):
    """the case of shape (n, S) with its three references (both terms, distortion alone, opacity alone), drawn once and shared"""
    if (n, S) not in _drawn:
        c = R.draw(1000 * n + S, n, S)
        c['ref'] = {k: R.ray_reg(c['w'], c['z'], c['lo'], c['hi'], *k) for k in ((LD, LO), (LD, 0.0), (0.0, LO))}
        _drawn[(n, S)] = c
    return _drawn[(n, S)]


def call(G, c, ld=LD, lo=LO, grads=True, fold=None):
    g_w = T(c['g0']) if grads else None
    values, stats = G.ray_reg(T(c['w']), T(c['z']), T(c['lo']), T(c['hi']), ld, lo, g_w, fold)
    torch.cuda.synchronize()
    return N(values).astype(np.float64), N(stats).astype(np.float64), None if g_w is None else N(g_w)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def check(c, ref, values, stats, g_w, tag):
    """values, stats and the accumulated gradient against a reference; returns the worst shares of the bounds"""
    np.testing.assert_array_equal(stats, ref['stats'])
    worst_v = 0.0
    for k in (0, 1):
        err, bound = abs(values[k] - ref['values'][k]), 1e-6 * ref['abs_sum'][k]
        print('%s: values[%d] %.9g, float64 %.9g, |difference| %.3e, bound %.3e' % (tag, k, values[k], ref['values'][k], err, bound))
        assert err <= bound, (tag, k)
        worst_v = max(worst_v, err / bound if bound > 0 else 0.0)
    ideal = c['g0'].astype(np.float64) + ref['grad']
    bound = 2.0 ** -23 * np.abs(ideal) + 1e-12 * ref['grad_abs']
    err = np.abs(g_w.astype(np.float64) - ideal)
    rows = ref['touched']
    share = float((err[rows] / bound[rows]).max()) if rows.any() else 0.0
    print('%s: %d of %d rows take a term; worst gradient entry at %.3f of its bound' % (tag, rows.sum(), len(rows), share))
    assert share <= 1.0, tag
    assert (bits(g_w)[~rows] == bits(c['g0'])[~rows]).all(), tag
    return worst_v, share


# ------------------------------------------------------------------------------------------------ 1. the kernel
@pytest.mark.parametrize('S', SAMPLES)
@pytest.mark.parametrize('n', RAYS)
def test_values_stats_and_gradients(G, n, S):
    c = case(n, S)
    ref = c['ref'][(LD, LO)]
    if n >= 3:
        assert S < 2 or (np.diff(c['z'][R.TIED]) == 0).any()
        assert not c['w'][R.ZERO].any() and np.isfinite(ref['opac'][R.ZERO]) and ref['opac'][R.ZERO] > 0
        assert c['hi'][R.INVALID] <= c['lo'][R.INVALID] and not ref['valid'][R.INVALID]
        assert abs(c['w'][R.UNIT].astype(np.float64).sum() - 1.0) <= 1e-6
        assert ref['stats'][0] == n - 1
    values, stats, g_w = call(G, c)
    check(c, ref, values, stats, g_w, '(n %d, S %d)' % (n, S))
    assert np.isfinite(g_w).all()


def test_rows_without_a_term_keep_their_bits(G):
    """lambda_opac = 0: the rows of invalid rays keep a sentinel's bits (a NaN with a payload, which no arithmetic would return)"""
    c = dict(case(257, 65))
    c['hi'] = c['hi'].copy()
    c['hi'][5::7] = c['lo'][5::7]
    sentinel = np.full(c['w'].shape, np.uint32(0x7fc12345)).view(np.float32)
    c['g0'] = np.where((c['hi'] > c['lo'])[:, None], c['g0'], sentinel)
    ref = R.ray_reg(c['w'], c['z'], c['lo'], c['hi'], LD, 0.0)
    values, stats, g_w = call(G, c, LD, 0.0)
    invalid = ~ref['valid']
    print('%d invalid rays of %d; their rows hold %s' % (invalid.sum(), len(invalid), sorted(set(map(hex, bits(g_w)[invalid].ravel())))))
    assert invalid.sum() >= 37 and stats[0] == ref['stats'][0] == (~invalid).sum()
    assert (bits(g_w)[invalid] == 0x7fc12345).all()
    assert np.isfinite(g_w[~invalid]).all() and (bits(g_w)[~invalid] != bits(c['g0'])[~invalid]).any()
    assert abs(values[0] - ref['values'][0]) <= 1e-6 * ref['abs_sum'][0] and values[1] == 0


def test_same_call_twice_is_bit_identical(G):
    for n, S in ((257, 192), (257, 1024), (3, 63)):
        a, b = call(G, case(n, S)), call(G, case(n, S))
        for x, y, name in zip(a, b, ('values', 'stats', 'g_w')):
            assert (bits(x) == bits(y)).all(), (n, S, name)


@pytest.mark.parametrize('n,S', [(257, 65), (3, 1), (257, 1024)])
def test_one_term_off(G, n, S):
    c = case(n, S)
    values, stats, g_w = call(G, c, LD, 0.0)
    assert values[1] == 0 and bits(values.astype(np.float32))[1] == 0
    check(c, c['ref'][(LD, 0.0)], values, stats, g_w, '(n %d, S %d) distortion alone' % (n, S))
    values, stats, g_w = call(G, c, 0.0, LO)
    assert values[0] == 0 and bits(values.astype(np.float32))[0] == 0
    check(c, c['ref'][(0.0, LO)], values, stats, g_w, '(n %d, S %d) opacity alone' % (n, S))


def test_fold_and_null_pointers(G):
    c = case(257, 192)
    fold = T(np.array([0.375], np.float32))
    values, stats, g_w = call(G, c, fold=fold)
    v32 = values.astype(np.float32)
    want = np.float32(0.375) + np.float32(LD * float(v32[0]) + LO * float(v32[1]))
    got = N(fold)[0]
    print('fold_total %.9g, host float32 arithmetic %.9g' % (got, want))
    assert bits(got) == bits(want) and got != np.float32(0.375)
    only, stats2, none = call(G, c, grads=False)                                 # a null g_w and a null fold_total
    assert none is None and (bits(only) == bits(values)).all() and (stats2 == stats).all()


def test_argument_errors_name_the_tensor(G):
    w, v = torch.zeros(8, 4, device=dev()), torch.zeros(8, device=dev())
    ok = lambda **kw: {**dict(weights=w, z=w.clone(), lo=v, hi=v + 1, lambda_distortion=1.0, lambda_opacity=1.0), **kw}
    for kw, what in ((dict(z=torch.zeros(8, 5, device=dev())), r'z: expected a contiguous tensor of shape \(8, 4\)'),
                     (dict(lo=torch.zeros(7, device=dev())), r'lo: expected a contiguous tensor of shape \(8,\)'),
                     (dict(hi=v.double()), 'hi: expected torch.float32'),
                     (dict(z=torch.zeros(4, 8, device=dev()).t()), 'z: expected a contiguous tensor'),
                     (dict(hi=torch.zeros(8)), 'hi: expected a CUDA/HIP float32 tensor'),
                     (dict(g_weights=torch.zeros(8, 3, device=dev())), 'g_weights: expected a contiguous tensor'),
                     (dict(fold_total=torch.zeros(2, device=dev())), 'fold_total: expected a one-element'),
                     (dict(lambda_distortion=-1.0), 'lambda_distortion = -1.0'),
                     (dict(lambda_opacity=float('inf')), 'lambda_opacity = inf'),
                     (dict(lambda_distortion=0.0, lambda_opacity=0.0), 'both 0')):
        with pytest.raises(G.RayRegError, match=what):
            G.ray_reg(**ok(**kw))
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ 2. the trainer
class Recorder(object):
    """ray_reg.ray_reg, keeping what every call got and left (host copies; synchronises, which a test may)"""

    def __init__(self, G):
        self.fn, self.calls = G.ray_reg, []

    def __call__(self, weights, z, lo, hi, lambda_distortion, lambda_opacity, g_weights=None, fold_total=None):
        torch.cuda.synchronize()
        c = dict(w=N(weights), z=N(z), lo=N(lo), hi=N(hi), ld=lambda_distortion, lo_=lambda_opacity, g_before=N(g_weights),
                 total_before=N(fold_total)[0])
        out = self.fn(weights, z, lo, hi, lambda_distortion, lambda_opacity, g_weights, fold_total)
        torch.cuda.synchronize()
        c.update(g_after=N(g_weights), values=N(out[0]), stats=N(out[1]))
        self.calls.append(c)
        return out


def _batch(n, seed=3):
    from outdoor_nerf_depth_amd.synthetic import SyntheticKitti
    rs = np.random.RandomState(seed)
    b = SyntheticKitti().random_batch(n, rs)
    b['depth_sup'] = np.where(rs.rand(n) < 0.7, rs.uniform(0.02, 0.2, n), 0).astype(np.float32)
    return {k: T(np.asarray(v, np.float32)) for k, v in b.items() if isinstance(v, np.ndarray)}


def _trainer(**kw):
    from outdoor_nerf_depth_amd.trainer import NerfppTrainer
    from outdoor_nerf_depth_amd.model import init_level_params
    return NerfppTrainer(dev(), precision=2, cascade_samples=(16, 32), level_params=init_level_params(2), **kw)


def _step(tr, batch):
    scalars = [N(s) for s in tr.train_step(batch)]
    tr.flush()
    torch.cuda.synchronize()
    return scalars, [N(g) for g in tr.grads]


@pytest.mark.parametrize('kind', ['mse', 'kl'])
def test_trainer_calls_once_per_level(G, monkeypatch, kind):
    from outdoor_nerf_depth_amd import ops
    rec = Recorder(G)
    monkeypatch.setattr(G, 'ray_reg', rec)
    ld, lo = 0.3, 0.02
    batch = _batch(64)
    kw = dict(use_depth=True, depth_loss_type=kind, lambda_depth=0.1)
    tr = _trainer(lambda_distortion=ld, lambda_opacity=lo, **kw)
    scalars, grads = _step(tr, batch)
    far = N(ops.sample_coarse(batch['ray_o'], batch['ray_d'], batch['min_depth'], 16, perturb=False)[0])
    assert len(rec.calls) == 2 and len(tr.last_ray_reg) == 2
    for m, (sc, c) in enumerate(zip(scalars, rec.calls)):
        S = (16, 48)[m]
        assert c['w'].shape == c['z'].shape == c['g_before'].shape == (64, S) and (c['ld'], c['lo_']) == (ld, lo)
        np.testing.assert_array_equal(c['lo'], N(batch['min_depth']))
        np.testing.assert_array_equal(c['hi'], far)
        assert (np.diff(c['z'], axis=-1) >= 0).all()
        assert c['g_before'].any() == (kind == 'kl')
        ref = R.ray_reg(c['w'], c['z'], c['lo'], c['hi'], ld, lo)
        fold = np.float32(ld * float(c['values'][0]) + lo * float(c['values'][1]))
        print('%s level %d: head total %.9g, values %s (float64 %s), valid %s, loss %.9g' % (kind, m, c['total_before'], c['values'],
                                                                                              ref['values'], c['stats'], sc[0]))
        assert abs(float(sc[0]) - (float(c['total_before']) + float(fold))) <= 2e-6 * (abs(float(c['total_before'])) + abs(float(fold)))
        for k in (0, 1):
            assert abs(c['values'][k] - ref['values'][k]) <= 1e-6 * ref['abs_sum'][k]
        assert c['stats'][0] == ref['stats'][0] == 64
        ideal = c['g_before'].astype(np.float64) + ref['grad']
        assert (np.abs(c['g_after'] - ideal) <= 2.0 ** -23 * np.abs(ideal) + 1e-12 * ref['grad_abs']).all()
        np.testing.assert_array_equal(N(tr.last_ray_reg[m][0]), c['values'])
        np.testing.assert_array_equal(N(tr.last_ray_reg[m][1]), c['stats'])
    monkeypatch.undo()
    off_scalars, off_grads = _step(_trainer(**kw), batch)
    for m in (0, 1):
        assert np.isfinite(grads[m]).all() and (grads[m] != off_grads[m]).any()
        assert off_scalars[m][1] == scalars[m][1]                                 # the same forward: the same rgb loss


def test_lambdas_off_is_the_trainer_without_them(G, monkeypatch, tmp_path):
    monkeypatch.setattr(G, '_lib', None)
    monkeypatch.setattr(G, 'LIB_PATH', str(tmp_path / 'librayreg_hip.so'))
    batch = _batch(64)
    for kw in (dict(use_depth=False), dict(use_depth=True, depth_loss_type='kl', lambda_depth=0.1)):
        a_sc, a_g = _step(_trainer(**kw), batch)
        tr = _trainer(lambda_distortion=0.0, lambda_opacity=0.0, **kw)
        b_sc, b_g = _step(tr, batch)
        assert tr.ray_reg is None and tr.last_ray_reg is None
        for x, y in zip(a_sc + a_g, b_sc + b_g):
            assert (bits(x) == bits(y)).all()
    assert G._lib is None
    with pytest.raises(G.RayRegError, match='librayreg_hip.so not found'):
        _trainer(use_depth=False, lambda_opacity=0.01).train_step(batch)
    torch.cuda.synchronize()


def test_inline_and_concurrent_backward_agree(G):
    """the level's backward on its own stream reads the g_w the regularisers wrote on the main stream"""
    batch = _batch(64)
    out = []
    for concurrent in (True, False):
        tr = _trainer(use_depth=False, lambda_distortion=0.3, lambda_opacity=0.02)
        tr.concurrent_backward = concurrent
        out.append(_step(tr, batch))
    for x, y in zip(out[0][0] + out[0][1], out[1][0] + out[1][1]):
        assert (bits(x) == bits(y)).all()


# ------------------------------------------------------------------------------------------------ 3. it does what it is for
def _held_out(tr, batch):
    """a deterministic forward of both levels on `batch` -> (mean dist_r of the last level by the host reference, PSNR, mean
    |depth - true depth| over the rays that have one)"""
    from outdoor_nerf_depth_amd import ops
    tr.flush()
    far, fg_z, bg_z = ops.sample_coarse(batch['ray_o'], batch['ray_d'], batch['min_depth'], tr.cascade_samples[0], perturb=False)
    ret = None
    for m, eng in enumerate(tr.engines):
        if m > 0:
            fg_z, bg_z = ops.sample_fine_pair(fg_z, ret['fg_weights'], bg_z, ret['bg_weights'], tr.cascade_samples[1], det=True)
        ret = eng.forward(batch['ray_o'], batch['ray_d'], far, fg_z, bg_z, training=False)
    torch.cuda.synchronize()
    ref = R.ray_reg(N(ret['fg_weights']), N(fg_z), N(batch['min_depth']), N(far), 1.0, 1.0)
    mse = float(((N(ret['rgb']).astype(np.float64) - N(batch['rgb'])) ** 2).mean())
    gt = N(batch['depth_gt']).astype(np.float64)
    return ref['values'][0], ref['values'][1], -10 * np.log10(mse), float(np.abs(N(ret['depth']) - gt)[gt > 0].mean())


def train_arm(seed, ld, lo, steps=TRAIN_STEPS, n_rays=256):
    """`steps` rgb-only steps of 256 rays, cascade (16, 32), from the initial state and the batches that `seed` fixes"""
    from outdoor_nerf_depth_amd.synthetic import SyntheticKitti
    scene = SyntheticKitti()
    rs = np.random.RandomState(100 + seed)
    tr = _trainer(use_depth=False, seed=777 + seed, lambda_distortion=ld, lambda_opacity=lo)
    for _ in range(steps):
        frame, pix = int(rs.randint(0, scene.n_train())), rs.randint(0, scene.H * scene.W, n_rays)
        b = scene.batch(frame, pix)
        tr.train_step({k: T(np.asarray(v, np.float32)) for k, v in b.items() if isinstance(v, np.ndarray)})
    held = SyntheticKitti().random_batch(1024, np.random.RandomState(999))
    return _held_out(tr, {k: T(np.asarray(v, np.float32)) for k, v in held.items() if isinstance(v, np.ndarray)})


def test_regularisers_lower_the_distortion_of_held_out_rays(G):
    """rgb-only training, 200 steps of 256 rays, cascade (16, 32), four seeds; both arms of a seed start from the same state and see
    the same batches.  On one fixed held-out batch of 1024 rays, the mean dist_r of the last level's deterministic forward, scored by
    the host reference, must be lower with the regularisers on by more than 3 standard errors of the paired differences.  PSNR and
    the depth error against the scene's true depth are printed, not gated.  Measured on an MI355X at lambdas (0.01, 0.001), means
    over the seeds: dist 0.016325 off, 0.006191 on, off - on = 0.010134 +- 0.002135 = 4.7 standard errors; foreground opacity entropy
    0.250 -> 0.153; PSNR 27.991 -> 28.018 dB; depth error 467133 -> 434800."""
    rows = []
    for seed in TRAIN_SEEDS:
        off, on = train_arm(seed, 0.0, 0.0), train_arm(seed, TRAIN_LD, TRAIN_LO)
        print('seed %d: off dist %.6f opac %.6f psnr %.3f depth error %.6f | on dist %.6f opac %.6f psnr %.3f depth error %.6f'
              % ((seed,) + off + on))
        rows.append(off + on)
    rows = np.asarray(rows)
    d = rows[:, 0] - rows[:, 4]
    se = d.std(ddof=1) / np.sqrt(len(d))
    print('mean over seeds: off dist %.6f psnr %.3f depth error %.6f | on dist %.6f psnr %.3f depth error %.6f'
          % (rows[:, 0].mean(), rows[:, 2].mean(), rows[:, 3].mean(), rows[:, 4].mean(), rows[:, 6].mean(), rows[:, 7].mean()))
    print('off - on = %.6f +- %.6f (standard error of %d paired differences) = %.1f standard errors' % (d.mean(), se, len(d), d.mean() / se))
    assert d.mean() > 3 * se, (d.mean(), se)


# ------------------------------------------------------------------------------------------------ 4. CLI
def test_cli_runs_three_steps(tmp_path):
    dev()
    from outdoor_nerf_depth_amd import ddp_train_nerf as T_
    argv = ['--expname', 'reg', '--basedir', str(tmp_path), '--synthetic', '--synthetic_hw', '24,32', '--synthetic_frames', '20',
            '--cascade_samples', '16,16', '--lambda_distortion', '0.01', '--lambda_opacity', '0.002', '--sample_every', '2',
            '--world_size', '1', '--N_rand_override', '128', '--i_weights', '100', '--i_test', '100', '--i_print', '1', '--N_iters', '3']
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
    saved = (tmp_path / 'reg' / 'args.txt').read_text()
    assert 'lambda_distortion = 0.01' in saved and 'lambda_opacity = 0.002' in saved
    num = r'([-\d.e+naif]+)'
    found = re.findall(r'step: (\d+) .*?' + ' .*?'.join('level_%d/%s: %s' % (m, k, num) for m in (0, 1)
                                                         for k in ('distortion', 'opacity', 'ray_reg_valid')), text)
    print('ddp_train_nerf with the regularisers: %s' % found)
    assert [int(f[0]) for f in found] == [0, 1, 2], text[-2000:]
    vals = np.asarray([[float(x) for x in f[1:]] for f in found])
    assert np.isfinite(vals).all() and (vals[:, [2, 5]] > 0).all() and (vals[:, [2, 5]] <= 1).all()

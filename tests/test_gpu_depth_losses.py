"""GPU: the one after-call of both trainers (depth_losses.after) against the sequence of public calls it stands for,
written out by hand: the head without a depth term, then depth_loss_rays / ssi_loss / gnll_loss with the level weights, the
gradient buffers and the fold spelled out here.  Both sides run the same kernels on the same inputs and the kernels give equal
bits for equal inputs, so everything is compared with assert_array_equal: the scalars, every gradient buffer handed to the
backward, the stats.  The shapes are the smallest that have every level and more than one group: MipNeRF-360 32 rays of 4 frames,
32 / 32 / 32 samples; NeRF++ 64 rays, cascade (16, 16), split-bf16."""
import numpy as np
import pytest

torch = pytest.importorskip('torch')
pytestmark = pytest.mark.gpu

from tests.test_gpu_mip360 import T, N, dev                                                 # noqa: E402
from tests.test_gpu_depth_gnll import _mip360_inputs, _mip360_params, _nerfpp_batch          # noqa: E402

LAMBDA = 0.1


def bits(t):
    return N(t).view(np.int32)


def same(got, want, tag):
    np.testing.assert_array_equal(bits(got), bits(want), err_msg=tag)


@pytest.mark.parametrize('kind', ['kl_ray', 'urf_ray', 'ssi', 'gnll'])
def test_mip360_after_call_is_the_hand_written_sequence(kind):
    from outdoor_nerf_depth_amd import mip360 as M
    from outdoor_nerf_depth_amd import depth_ssi, depth_gnll
    n, sigma = 32, 0.3
    rays, gt, sup, std, jit = _mip360_inputs(n)
    cam = T(np.arange(n, dtype=np.int32) % 4)
    prop0, nerf0 = _mip360_params()
    tr = M.Mip360Trainer(prop0, nerf0, dev(), max_steps=1000, depth_loss_type=kind, lambda_depth=LAMBDA, depth_sigma=sigma,
                         num_prop_samples=32, num_nerf_samples=32, depth_ssi_groups=4, depth_ssi_min_rays=2)
    lv = tr.forward(rays, 0.0, jit)                      # the first step's forward: train_frac = 0, the initial parameters
    props, nerf = lv[:-1], lv[-1]
    head = (nerf['rgb'], gt, nerf['distance_mean'], sup, nerf['sdist'], nerf['weights'], [p['sdist'] for p in props],
            [p['weights'] for p in props])
    kw = dict(lambda_depth=LAMBDA, dm_prop=[p['distance_mean'] for p in props], tdist_nerf=nerf['tdist'],
              tdist_prop=[p['tdist'] for p in props], directions=rays['directions'], depth_sigma=sigma)

    # what Mip360Trainer.train_step asks of losses()
    extra = dict(prior_std=std, group=cam, n_groups=4, min_rays=2)
    got = M.losses(*head, depth_loss_type=kind, extra=extra, **kw)

    # by hand: the head with depth type 0, then the loss's own call.  train_utils.py:136-143: the NeRF level enters the total as
    # data_loss_mult * lambda (inside `data`) + (depth_weight - 1) * lambda (loss_disp_mse), a proposal level as
    # prop_depth_weight * lambda; data_loss_mult = 1, depth_weight = 2, prop_depth_weight = 1 are losses()'s defaults
    sc, g_rgb, g_dm, g_wn, g_wp, g_dmp = M.losses(*head, depth_loss_type=None, **kw)
    k_nerf, kp = (1.0 + (2.0 - 1.0)) * LAMBDA, 1.0 * LAMBDA
    scale = [kp, kp, k_nerf]
    w = [p['weights'] for p in props] + [nerf['weights']]
    td = [p['tdist'] for p in props] + [nerf['tdist']]
    dm = [p['distance_mean'] for p in props] + [nerf['distance_mean']]
    fold = dict(total=sc[0:1], last=sc[2:3], others=sc[5:6])
    stats = None
    if kind == 'kl_ray':
        M.depth_loss_rays('kl_ray', w, td, sup, None, rays['directions'], sigma, scale, g_wp + [g_wn], None, sc)
    elif kind == 'urf_ray':
        M.depth_loss_rays('urf_ray', w, td, sup, dm, None, sigma, scale, g_wp + [g_wn], g_dmp + [g_dm], sc)
    elif kind == 'ssi':
        stats = depth_ssi.ssi_loss(dm, sup, cam, 4, 2, 'all', scale, g_dmp + [g_dm], fold)[2]
    else:
        stats = depth_gnll.gnll_loss(w, td, dm, sup, std, None, True, scale, g_wp + [g_wn], g_dmp + [g_dm], fold)[1]

    # one step of the trainer from the same state: its scalars and the stats it keeps
    step_sc = tr.train_step(rays, gt, sup, jitter01=jit, cam_idx=cam, depth_std=std)
    tr.flush()
    torch.cuda.synchronize()
    print('%s: scalars %s' % (kind, N(sc)))
    assert np.isfinite(N(sc)).all() and N(sc)[2] != 0
    same(got[0], sc, 'scalars of losses()')
    same(step_sc, sc, 'scalars of train_step')
    for name, a, b in (('g_rgb', got[1], g_rgb), ('g_dm', got[2], g_dm), ('g_wn', got[3], g_wn)):
        same(a, b, name)
    assert len(got[4]) == len(g_wp) == 2 and len(got[5]) == len(g_dmp) == 2
    for k in range(2):
        same(got[4][k], g_wp[k], 'g_wp[%d]' % k)
        same(got[5][k], g_dmp[k], 'g_dmp[%d]' % k)
    if stats is None:
        assert tr.last_ssi_stats is None and tr.last_gnll_stats is None and extra['stats'] is None
    else:
        kept = tr.last_ssi_stats if kind == 'ssi' else tr.last_gnll_stats
        assert (tr.last_gnll_stats if kind == 'ssi' else tr.last_ssi_stats) is None
        assert tuple(kept.shape) == (3, 2 if kind == 'ssi' else 3) and N(stats)[2, 0] > 0
        same(kept, stats, 'stats of train_step')
        same(extra['stats'], stats, 'stats of losses()')


@pytest.mark.parametrize('kind', ['ssi', 'gnll'])
def test_nerfpp_after_call_is_the_hand_written_sequence(kind, monkeypatch):
    from outdoor_nerf_depth_amd import ops, depth_ssi, depth_gnll
    from outdoor_nerf_depth_amd.trainer import NerfppTrainer
    from outdoor_nerf_depth_amd.model import init_level_params
    tr = NerfppTrainer(dev(), precision=2, cascade_samples=(16, 16), use_depth=True, depth_loss_type=kind, lambda_depth=LAMBDA,
                       level_params=init_level_params(2), depth_ssi_min_rays=2)
    batch = _nerfpp_batch(64)
    seen, handed = [], []                                # per level: what the loss head was given / what the backward was handed
    inner = ops.loss_and_grads

    def head(ret, rgb_gt, depth_sup, loss_type, *rest):
        assert depth_sup is None and loss_type == 'rgbonly'
        seen.append(({k: (v.clone() if torch.is_tensor(v) else v) for k, v in ret.items()}, rgb_gt.clone()))
        return inner(ret, rgb_gt, depth_sup, loss_type, *rest)
    monkeypatch.setattr(ops, 'loss_and_grads', head)
    z_vals = []
    for name in ('sample_coarse', 'sample_fine_pair'):   # fg_z of a level: the first of the pair both samplers return last
        def sampler(*a, _inner=getattr(ops, name), **k):
            out = _inner(*a, **k)
            z_vals.append((out[-2].clone(), out[0].clone()))
            return out
        monkeypatch.setattr(ops, name, sampler)
    for eng in tr.engines:
        def backward(g_rgb, g_depth, g_w, *a, _inner=eng.backward, **k):
            handed.append([None if g is None else g.clone() for g in (g_rgb, g_depth, g_w)])      # (on the backward's stream)
            return _inner(g_rgb, g_depth, g_w, *a, **k)
        eng.backward = backward
    scalars = tr.train_step(batch)
    tr.flush()
    torch.cuda.synchronize()
    monkeypatch.undo()
    assert len(seen) == len(handed) == len(z_vals) == 2
    far = z_vals[0][1]                                   # sample_coarse returns (far, fg_z, bg_z)
    for m in range(2):
        ret, rgb_gt = seen[m]
        fg_z = z_vals[m][0]
        sc, g_rgb, g_depth, g_w = ops.loss_and_grads(ret, rgb_gt, None, 'rgbonly', LAMBDA)
        fold = dict(total=sc[0:1], last=sc[2:3], n_sup=sc[3:4])
        if kind == 'ssi':
            depth_ssi.ssi_loss([ret['depth']], batch['depth_sup'], None, 1, 2, 'supervised', [LAMBDA], [g_depth], fold)
        else:
            g_w = torch.zeros_like(ret['fg_weights'])
            _, stats = depth_gnll.gnll_loss([ret['fg_weights']], [fg_z], [ret['depth']], batch['depth_sup'], batch['depth_std'],
                                            limit=far, scale=[LAMBDA], g_weights=[g_w], g_pred=[g_depth], fold=fold)
        torch.cuda.synchronize()
        print('%s level %d: scalars %s' % (kind, m, N(sc)))
        assert np.isfinite(N(sc)).all() and N(sc)[2] != 0 and N(sc)[3] > 0
        same(scalars[m], sc, 'level %d scalars' % m)
        for name, a, b in zip(('g_rgb', 'g_depth', 'g_w'), handed[m], (g_rgb, g_depth, g_w)):
            assert (a is None) == (b is None) == (kind == 'ssi' and name == 'g_w'), name      # ssi: the rgb-only head's, none
            if b is not None:
                same(a, b, 'level %d %s' % (m, name))
        if kind == 'gnll':
            assert tuple(tr.last_gnll_stats[m].shape) == (1, 3)
            same(tr.last_gnll_stats[m], stats, 'level %d stats' % m)
    assert len(tr.last_gnll_stats or []) == (2 if kind == 'gnll' else 0) and not hasattr(tr, 'last_ssi_stats')

"""GPU: the multi-view consistency check of depth priors (depthcons_check, csrc/depthcons_kernels.hip) against
tests/depth_consistency_reference.py, through the CLI on both on-disk layouts and through the load-time flags of both trainers.

Gates.  The kernel does the reference's float64 arithmetic in the reference's order without contraction, so every discrete output
-- counts, the kept mask, depth_out (bit for bit, NaN payloads included) and rows -- must be EQUAL, and std_out, whose only
rounding that can differ is the final float64 -> float32 one, within 2 float32 ulp.  The scene, the shapes and the priors are those
of tests/test_depth_consistency.py; every figure is printed before it is asserted.

Measured on an MI355X: std_out 0 ulp from the reference in every case.  test_filtering_outliers_helps_the_depth_of_an_mse_run (the
float64 mean |distance_mean - true depth| over the rays with a true depth, per batch, mean over the last 50 of 400 batches +-
standard error): mse with Config.depth_cons_views = 4 0.078975 +- 0.000466, plain mse 0.279229 +- 0.002622, rgb-only 0.345908 +-
0.001898; unfiltered - filtered = 75.2 standard errors of the difference (gate: 3).
"""
import logging
import os
import re

import numpy as np
import pytest

torch = pytest.importorskip('torch')
pytestmark = pytest.mark.gpu

from tests import depth_consistency_reference as R                                       # noqa: E402
from tests.test_gpu_mip360 import T, N, dev                                              # noqa: E402
from tests.test_depth_consistency import (SHAPES, analytic_scene, prior_of, reference, corrupted, axis_angle,   # noqa: E402
                                          write_colmap_scene, write_nerfpp_scene)

KINDS = ('exact', 'corrupted', 'sparse', 'invalids')


@pytest.fixture(scope='module')
def DC():
    dev()
    from outdoor_nerf_depth_amd import depth_consistency
    return depth_consistency


def ulps(a, b):
    """float32 ulp distance of two arrays of non-negative finite floats"""
    return np.abs(a.view(np.int32).astype(np.int64) - b.view(np.int32).astype(np.int64))


def assert_matches(DC, prior, cams, nbr, tag, ref=None, **params):
    """one call against the reference: the discrete outputs equal, std_out within 2 ulp; returns the call's host outputs"""
    ref = ref if ref is not None else R.check(prior, cams, nbr, **params)
    got = DC.check_async(T(prior), cams, nbr, counts=True, **params).get()
    valid = prior > 0
    worst = int(ulps(got['std'], ref['std_out']).max())
    print('%s: rows total %s, std_out worst %d ulp (gate 2)' % (tag, got['rows'].sum(0).tolist(), worst))
    np.testing.assert_array_equal(got['counts'], ref['counts'])
    np.testing.assert_array_equal(valid & (got['depth'] > 0), ref['keep'])
    np.testing.assert_array_equal(got['depth'].view(np.int32), ref['depth_out'].view(np.int32))
    np.testing.assert_array_equal(got['rows'], ref['rows'])
    np.testing.assert_array_equal(got['std'] > 0, ref['std_out'] > 0)
    assert worst <= 2
    return got


# ------------------------------------------------------------------------------------------------ 1. parity
@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('shape', SHAPES)
def test_parity_with_the_reference(DC, shape, kind):
    s = analytic_scene(shape)
    prior = prior_of(kind, shape)
    got = assert_matches(DC, prior, s['cams'], s['nbr'], '%s %s' % (shape, kind), ref=reference(kind, shape))
    assert got['rows'][:, 0].sum() == (prior > 0).sum() and got['rows'][:, 1].sum() > 0        # the case has something to decide
    if kind != 'sparse':
        assert got['rows'][:, 3].sum() > 0 or kind == 'invalids'


def test_parity_with_other_parameters(DC):
    shape = SHAPES[1]
    s = analytic_scene(shape)
    prior = corrupted(prior_of('exact', shape))[0]
    for params in (dict(min_views=1, pix_tol=0.5, rel_tol=0.002), dict(min_views=3, keep_unverified=False, std_floor=0.05),
                   dict(pix_tol=0.0, rel_tol=0.0), dict(min_views=4, pix_tol=3.0, rel_tol=0.3, std_floor=1e-4)):
        assert_matches(DC, prior, s['cams'], s['nbr'], str(params), **params)


# ------------------------------------------------------------------------------------------------ 2. branches
def _pair_cams(DC, c2w, H=16, W=40):
    return DC.pack_cams(np.array([[30.0, 0, W / 2.0], [0, 30.0, H / 2.0], [0, 0, 1.0]]), c2w)


def test_a_frame_turned_around_sees_nothing(DC):
    c2w = np.tile(np.eye(4)[:3], (3, 1, 1))
    c2w[:, 0, 3] = (0.0, 0.2, 0.4)
    c2w[1, :, :3] = axis_angle([0, 1, 0], np.pi)                                             # looks down -z: Pj.z <= 0 for every point
    cams = _pair_cams(DC, c2w)
    prior = np.full((3, 16, 40), 5.0, np.float32)
    nbr = np.array([[1], [0], [0]], np.int32)
    got = assert_matches(DC, prior, cams, nbr, 'turned', min_views=1)
    assert (got['counts'][0] == 0).all() and (got['counts'][1] == 0).all() and got['counts'][2, ..., 0].any()
    assert got['rows'].tolist()[0] == [640, 0, 640, 0]
    got = assert_matches(DC, prior, cams, nbr, 'turned, unverified dropped', min_views=1, keep_unverified=False)
    assert got['rows'].tolist()[0] == [640, 0, 0, 640] and (got['depth'][0] == 0).all() and (got['std'][0] == 0).all()


def test_a_frame_far_away_projects_outside(DC):
    c2w = np.tile(np.eye(4)[:3], (2, 1, 1))
    c2w[1, 0, 3] = 1000.0
    got = assert_matches(DC, np.full((2, 16, 40), 5.0, np.float32), _pair_cams(DC, c2w), np.array([[1], [0]], np.int32), 'displaced', min_views=1)
    assert (got['counts'] == 0).all() and got['rows'].tolist() == [[640, 0, 640, 0]] * 2


def test_one_sixteen_and_padded_neighbour_lists(DC):
    shape = SHAPES[2]
    s = analytic_scene(shape)
    prior = corrupted(s['depth'])[0]
    assert_matches(DC, prior, s['cams'], s['nbr'][:, :1].copy(), 'K = 1', min_views=1)
    nbr = np.full((shape[0], 16), -1, np.int32)
    nbr[:, [0, 5, 9, 15]] = s['nbr']                                                         # -1 padding in the middle of every list
    got = assert_matches(DC, prior, s['cams'], nbr, 'K = 16, padded')
    np.testing.assert_array_equal(got['depth'], reference('corrupted', shape)['depth_out'])  # the padding changes nothing
    every = DC.neighbours(s['c2w'][:, :, 3], 16)                                             # 7 others, 9 pads at the end
    assert (every[:, 7:] == -1).all()
    assert_matches(DC, prior, s['cams'], every, 'K = 16, every frame', min_views=5)


def test_min_views_above_k_makes_everything_unverifiable(DC):
    shape = SHAPES[0]
    s = analytic_scene(shape)
    prior = prior_of('invalids', shape)
    n_valid = int((prior > 0).sum())
    for keep in (True, False):
        got = assert_matches(DC, prior, s['cams'], s['nbr'], 'min_views 5 > K 4, keep %s' % keep, min_views=5, keep_unverified=keep)
        assert got['rows'].sum(0).tolist() == [n_valid, 0, n_valid if keep else 0, 0 if keep else n_valid]


def test_a_single_frame_has_no_neighbours(DC):
    s = analytic_scene(SHAPES[0])
    prior = np.ascontiguousarray(prior_of('invalids', SHAPES[0])[:1])
    for nbr in (np.zeros((1, 0), np.int32), np.full((1, 3), -1, np.int32), DC.neighbours(s['c2w'][:1, :, 3], 4)):
        got = assert_matches(DC, prior, s['cams'][:1], nbr, 'F = 1, K = %d' % nbr.shape[1])
        assert (got['counts'] == 0).all() and got['rows'][0, 1] == 0 and got['rows'][0, 2] == (prior > 0).sum()
        np.testing.assert_array_equal(got['std'][prior > 0], (0.01 * prior[prior > 0].astype(np.float64)).astype(np.float32))


# ------------------------------------------------------------------------------------------------ 3. reproducibility
def test_same_call_twice_and_sub_batches_are_bit_identical(DC):
    shape = SHAPES[2]
    s = analytic_scene(shape)
    prior = corrupted(prior_of('exact', shape))[0]
    a = DC.check_async(T(prior), s['cams'], s['nbr'], counts=True).get()
    b = DC.check_async(T(prior), s['cams'], s['nbr'], counts=True).get()
    for k in a:
        np.testing.assert_array_equal(a[k].view(np.uint8), b[k].view(np.uint8))
    for i in (0, 3, 7):
        sub = sorted(set([i]) | set(int(j) for j in s['nbr'][i]))
        pos = {f: n for n, f in enumerate(sub)}
        nbr = np.array([[pos.get(int(j), -1) for j in s['nbr'][f]] for f in sub], np.int32)
        c = DC.check_async(T(prior[sub]), s['cams'][sub], nbr, counts=True).get()
        for k in a:
            np.testing.assert_array_equal(a[k][i].view(np.uint8), c[k][pos[i]].view(np.uint8), err_msg='frame %d, %s' % (i, k))


def test_rows_are_the_counts_of_the_maps_and_null_outputs_are_accepted(DC):
    shape = SHAPES[1]
    s = analytic_scene(shape)
    prior = prior_of('invalids', shape) * np.where(corrupted(prior_of('exact', shape))[1], np.float32(1.2), np.float32(1))
    full = DC.check_async(T(prior), s['cams'], s['nbr'], counts=True, min_views=2).get()
    valid = prior > 0
    kept = valid & (full['depth'] > 0)
    F = shape[0]
    rows = np.stack([valid.reshape(F, -1).sum(1), (valid & (full['counts'][..., 0] >= 2)).reshape(F, -1).sum(1), kept.reshape(F, -1).sum(1),
                     (valid & ~kept).reshape(F, -1).sum(1)], 1)
    np.testing.assert_array_equal(full['rows'], rows)
    assert full['rows'].dtype == np.int64 and full['counts'].dtype == np.uint8
    bare = DC.check_async(T(prior), s['cams'], s['nbr'], std=False, counts=False, rows=False)
    assert sorted(bare.tensors) == ['depth']
    np.testing.assert_array_equal(bare.get()['depth'].view(np.int32), full['depth'].view(np.int32))
    one = DC.check_async(T(prior), s['cams'], s['nbr'], std=True, counts=False, rows=False).get()
    np.testing.assert_array_equal(one['std'], full['std'])
    d, sd, rw = DC.filter_priors(T(prior), s['cams'], 4)
    assert torch.equal(d, T(full['depth'])) or np.array_equal(N(d).view(np.int32), full['depth'].view(np.int32))
    np.testing.assert_array_equal(N(sd), full['std'])
    np.testing.assert_array_equal(rw.cpu().numpy(), full['rows'])


def test_device_argument_errors_name_the_tensor(DC):
    s = analytic_scene(SHAPES[0])
    prior = T(s['depth'])
    for bad, text in ((prior.double(), r'depth: expected torch.float32, got torch.float64'), (prior[0], r'depth: expected \[F, H, W\]'),
                      (prior[:, :, ::2], 'depth: expected a contiguous tensor')):
        with pytest.raises(DC.DepthConsError, match=text):
            DC.check_async(bad, s['cams'], s['nbr'])
    with pytest.raises(DC.DepthConsError, match='depth_out overlaps depth'):
        DC.check_async(prior, s['cams'], s['nbr'], depth_out=prior)
    with pytest.raises(DC.DepthConsError, match='depth_out overlaps depth'):
        DC.check_async(prior[1:], s['cams'][1:], np.full((5, 1), -1), depth_out=prior[:5])
    with pytest.raises(DC.DepthConsError, match=r'depth_out \(5, 24, 32\)'):
        DC.check_async(prior, s['cams'], s['nbr'], depth_out=torch.empty_like(prior[:5]))
    with pytest.raises(DC.DepthConsError, match='cams: 5 cameras for 6 frames'):
        DC.check_async(prior, s['cams'][:5], np.full((5, 1), -1))
    with pytest.raises(DC.DepthConsError, match='nbr: frame 0 lists itself'):
        DC.check_async(prior, s['cams'], np.zeros((6, 1), np.int32))
    # the library's own alias check, below the binding's
    lib, out = DC.lib(), torch.empty_like(prior)
    cams, nbr = T(s['cams']), T(s['nbr'])
    rc = lib.depthcons_check(None, 6, 24, 32, 4, prior.data_ptr(), cams.data_ptr(), nbr.data_ptr(), 1.0, 0.01, 2, 1, 0.0, None,
                             out.data_ptr(), prior.data_ptr(), None, None)
    assert rc == 1 and 'std_out overlaps depth' in DC.last_error()
    ok = DC.check_async(prior, s['cams'], s['nbr'], depth_out=out).get()
    np.testing.assert_array_equal(ok['depth'], s['depth'] * (ok['depth'] > 0))


# ------------------------------------------------------------------------------------------------ 4. the CLI on both layouts
PARAMS = ['--views', '4', '--rel_tol', '0.02', '--std_floor', '0.01']
PARAMS_KW = dict(rel_tol=0.02)


@pytest.fixture(scope='module')
def colmap_scene(tmp_path_factory):
    dev()
    root = tmp_path_factory.mktemp('depth_cons_colmap')
    names, mask = write_colmap_scene(str(root / 'scene'))
    return root / 'scene', names, mask


def _scene(data, sup_type, extra=()):
    from outdoor_nerf_depth_amd import mip360_data as D
    return D.Scene(D.parse_gin(bindings=["Config.data_dir = '%s'" % data, "Config.depth_sup_type = '%s'" % sup_type, 'Config.sample_every = 1'] + list(extra)))


def test_cli_on_a_colmap_scene(DC, colmap_scene):
    from PIL import Image
    data, names, mask = colmap_scene
    rows = DC.main(['--data_dir', str(data), '--depth_sup_type', 'noisy'] + PARAMS)
    scene = _scene(data, 'noisy')
    d, sd, rw = DC.filter_priors(T(scene.depths_sup), DC.cams_from_scene(scene), 4, std_floor=0.01 * scene.scale, **PARAMS_KW)
    d, sd, rw = N(d), N(sd), rw.cpu().numpy()
    np.testing.assert_array_equal(rows, rw)
    kept = (scene.depths_sup > 0) & (d > 0)
    print('colmap CLI: totals %s; corrupted pixels dropped %.1f %%, clean pixels kept %.1f %%'
          % (rw.sum(0).tolist(), 100.0 * (~kept)[mask].mean(), 100.0 * kept[~mask].mean()))
    assert (~kept)[mask].mean() > 0.8 and kept[~mask].mean() > 0.8
    # the folders, read back through the loader under T_cons, equal the in-memory result
    cons = _scene(data, 'noisy_cons', ["Config.depth_loss_type = 'gnll'"])                       # gnll finds the _std twin
    assert cons.depth_std_source == 'folder'
    np.testing.assert_array_equal(cons.depths_sup > 0, kept)
    np.testing.assert_array_equal(cons.depths_sup[kept], d[kept])
    assert (cons.depths_sup[~kept] < 0).all()
    np.testing.assert_array_equal(cons.depths_std > 0, kept)
    metres = sd.astype(np.float64) / scene.scale
    assert (metres[kept] >= 0.01 * (1 - 1e-6)).all()                                           # --std_floor is in metres
    err = np.abs(cons.depths_std.astype(np.float64) / scene.scale - np.clip(metres, 2.0 / 256, 65535.0 / 256))[kept]
    print('colmap CLI: std read back within %.3g m of the in-memory one (half a PNG step is %.3g m)' % (err.max(), 0.5 / 256))
    assert err.max() <= 0.5 / 256 + 1e-6
    # kept pixels carry the input's own 16-bit value, dropped ones 0
    for i, name in enumerate(scene.names):
        raw = np.asarray(Image.open(str(data / 'depths_noisy' / name)))
        out = np.asarray(Image.open(str(data / 'depths_noisy_cons' / name)))
        np.testing.assert_array_equal(out, np.where(kept[i] | (raw < 2), raw, 0))
        assert out.dtype == raw.dtype
    # the text file
    lines = (data / 'consistency_noisy.txt').read_text().splitlines()
    assert len(lines) == 2 + len(names) and lines[-1].split()[:5] == ['total'] + [str(v) for v in rw.sum(0)]
    for i, name in enumerate(scene.names):
        assert lines[1 + i].split()[:5] == [name] + [str(v) for v in rw[i]]
    absrel_kept, absrel_dropped = (float(v) for v in lines[-1].split()[5:])
    print('colmap CLI: AbsRel of the raw prior over kept %.5f, over dropped %.5f' % (absrel_kept, absrel_dropped))
    assert absrel_kept < 0.1 < absrel_dropped


def test_cli_on_a_nerfpp_scene(DC, tmp_path):
    from PIL import Image
    from outdoor_nerf_depth_amd.data_loader_split import load_data_split
    write_nerfpp_scene(str(tmp_path), F=8)
    done = DC.main(['--datadir', str(tmp_path), '--scene', 'scene', '--depth_sup_type', 'noisy', '--min_views', '1'] + PARAMS)
    assert sorted(done) == ['test', 'train']
    for split in ('train', 'test'):
        before = load_data_split(str(tmp_path), 'scene', split, depth_sup_type='noisy')
        H, W, scale = before[0].H, before[0].W, before[0].depth_scale
        prior = np.stack([s.depth_sup.reshape(H, W) for s in before], 0)
        d, sd, rw = DC.filter_priors(T(prior), DC.cams_from_samplers(before), 4, min_views=1, std_floor=0.01 * scale, **PARAMS_KW)
        d, sd, rw = N(d), N(sd), rw.cpu().numpy()
        np.testing.assert_array_equal(done[split], rw)
        kept = d > 0
        print('nerfpp CLI %s: totals %s' % (split, rw.sum(0).tolist()))
        assert 0 < rw[:, 3].sum() < rw[:, 0].sum()
        after = load_data_split(str(tmp_path), 'scene', split, depth_sup_type='noisy_cons', depth_std=0.0)   # gnll's loader call
        np.testing.assert_array_equal(np.stack([s.depth_sup.reshape(H, W) for s in after], 0), d)
        std = np.stack([s.depth_std.reshape(H, W) for s in after], 0)
        np.testing.assert_array_equal(std > 0, kept)
        err = np.abs(std.astype(np.float64) / scale - np.clip(sd.astype(np.float64) / scale, 2.0 / 256, None))[kept]
        assert err.max() <= 0.5 / 256 + 1e-6
        split_dir = tmp_path / 'scene' / split
        for i, f in enumerate(sorted((split_dir / 'depth_noisy').iterdir())):
            raw, out = np.asarray(Image.open(str(f))), np.asarray(Image.open(str(split_dir / 'depth_noisy_cons' / f.name)))
            np.testing.assert_array_equal(out, np.where(kept[i], raw, 0))
        lines = (split_dir / 'consistency_noisy.txt').read_text().splitlines()
        assert lines[-1].split()[:5] == ['total'] + [str(v) for v in rw.sum(0)] and len(lines[-1].split()) == 7


# ------------------------------------------------------------------------------------------------ 5. the load-time flags
CONS = ['Config.depth_cons_views = 4', 'Config.depth_cons_rel_tol = 0.02']


def _one_mip360_step(scene, train, cfg):
    from outdoor_nerf_depth_amd import mip360 as M
    from outdoor_nerf_depth_amd import mip360_train as TR
    tr = TR.make_trainer(cfg, dev(), n_train_frames=train['cams'].shape[0])
    b = M.sample_batch(train['cams'], train['rgb_u8'], train['depth_sup'], 0, 0, 256, scene.near, scene.far)
    kw = dict(depth_std=TR.batch_depth_std(train['depth_std'], b['pix'])) if 'depth_std' in train else {}
    sc = N(tr.train_step(b['rays'], b['rgb'], b['depth_sup'], jitter01=list(b['jitter01']), **kw))
    tr.flush()
    torch.cuda.synchronize()
    return b, sc


def test_mip360_flag_filters_the_training_split_only(DC, colmap_scene, capsys, tmp_path):
    from outdoor_nerf_depth_amd import mip360_data as D
    data = colmap_scene[0]
    base = ["Config.data_dir = '%s'" % data, "Config.depth_sup_type = 'noisy'", 'Config.sample_every = 1', 'Config.batch_size = 256']
    plain = D.Scene(D.parse_gin(bindings=base))
    raw = plain.device_frames('train', dev())
    assert 'depth_cons_rows' not in raw
    cfg = D.parse_gin(bindings=base + CONS)
    scene = D.Scene(cfg)
    train = scene.device_frames('train', dev())
    assert 'depth consistency' not in capsys.readouterr().out                               # the trainer's rank 0 logs, not the loader
    want, _, rows = DC.filter_priors(raw['depth_sup'], DC.cams_from_scene(plain, plain.train), 4, rel_tol=0.02)
    assert torch.equal(train['depth_sup'], want) and torch.equal(train['depth_cons_rows'], rows) and 'depth_std' not in train
    tot = rows.sum(0).tolist()
    assert tot[3] > 0
    # the CLI: one log line with the totals
    from tests.test_gpu_mip360_app import _run
    b = base + CONS + ["Config.checkpoint_dir = '%s'" % (tmp_path / 'run'), 'Config.max_steps = 2', 'Config.checkpoint_every = 100',
                       'Config.print_every = 1', 'Config.lr_delay_steps = 0', 'Config.render_chunk_size = 1024']
    out = _run('mip360_train', sum([['--gin_bindings', x] for x in b], []))
    line = [l for l in out.splitlines() if l.startswith('depth consistency check')]
    print(line)
    assert line == ['depth consistency check (4 views): 11 frames, %d valid prior pixels, %d verifiable, %d kept, %d dropped' % tuple(tot)], out[-2000:]
    assert 'step 2/2' in out
    test = scene.device_frames('test', dev())
    assert torch.equal(test['depth_sup'], plain.device_frames('test', dev())['depth_sup']) and 'depth_cons_rows' not in test
    b, sc = _one_mip360_step(scene, train, cfg)                                            # the step's prior is the filtered one
    f, x, y = b['pix'].long().unbind(1)
    assert torch.equal(b['depth_sup'].reshape(-1), want[f, y, x]) and np.isfinite(sc).all()
    assert int((raw['depth_sup'][f, y, x] != want[f, y, x]).sum()) > 0
    # a gnll run without maps or a constant takes the check's spread
    cfg = D.parse_gin(bindings=base + CONS + ["Config.depth_loss_type = 'gnll'", 'Config.depth_cons_std_floor = 0.02'])
    scene = D.Scene(cfg)
    train = scene.device_frames('train', dev())
    _, std, _ = DC.filter_priors(raw['depth_sup'], DC.cams_from_scene(plain, plain.train), 4, rel_tol=0.02, std_floor=0.02 * scene.scale)
    assert torch.equal(train['depth_std'], std) and float(std[want > 0].min()) >= 0.02 * scene.scale * (1 - 1e-6)
    _, sc = _one_mip360_step(scene, train, cfg)
    assert np.isfinite(sc).all()


def _run_nerfpp(argv):
    from outdoor_nerf_depth_amd import ddp_train_nerf as T_
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
    return '\n'.join(lines)


def _nerfpp_argv(base, loss='mse', extra=()):
    return ['--expname', 'cons_' + loss, '--basedir', str(base), '--synthetic', '--synthetic_hw', '24,32', '--synthetic_frames', '20',
            '--cascade_samples', '16,16', '--use_depth', '--depth_loss_type', loss, '--depth_sup_type', 'mono_crop', '--lambda_depth',
            '0.1', '--sample_every', '2', '--world_size', '1', '--N_rand_override', '128', '--i_weights', '100', '--i_test', '100',
            '--i_print', '1', '--N_iters', '2'] + list(extra)


def test_nerfpp_flag_filters_the_samplers(DC, tmp_path):
    from outdoor_nerf_depth_amd.data_loader_split import load_data_split
    from outdoor_nerf_depth_amd.device_sampler import DeviceRaySamplers
    from outdoor_nerf_depth_amd.trainer import NerfppTrainer
    from outdoor_nerf_depth_amd.model import init_level_params
    write_nerfpp_scene(str(tmp_path), F=8)
    samplers = load_data_split(str(tmp_path), 'scene', 'train', depth_sup_type='noisy', depth_std=0.0, depth_std_optional=True)
    H, W, scale = samplers[0].H, samplers[0].W, samplers[0].depth_scale
    prior = np.stack([s.depth_sup.reshape(H, W) for s in samplers], 0)
    cams = DC.cams_from_samplers(samplers)
    ref = R.check(prior, cams, DC.neighbours(cams[:, [7, 11, 15]], 3), min_views=1, rel_tol=0.02, std_floor=0.01 * scale)
    rows = DC.filter_samplers(samplers, dev(), 3, want_std=True, min_views=1, rel_tol=0.02, std_floor=0.01 * scale)
    np.testing.assert_array_equal(rows, ref['rows'])
    assert 0 < rows[:, 3].sum() < rows[:, 0].sum()
    for i, s in enumerate(samplers):                                                           # host sampling reads these
        np.testing.assert_array_equal(s.depth_sup, ref['depth_out'][i].reshape(-1))
        assert ulps(s.depth_std, ref['std_out'][i].reshape(-1)).max() <= 2
        assert set(s.random_sample(16)) >= {'depth_sup', 'depth_std'}
    ds = DeviceRaySamplers(samplers, dev(), seed=1)                                            # and so does the device sampler
    np.testing.assert_array_equal(N(ds.depth_sup).reshape(len(samplers), -1), ref['depth_out'].reshape(len(samplers), -1))
    batch = ds.random_sample(64)
    sup = N(batch['depth_sup'])
    assert np.isin(sup, ref['depth_out']).all()
    tr = NerfppTrainer(dev(), precision=2, cascade_samples=(16, 16), use_depth=True, depth_loss_type='mse', level_params=init_level_params(2))
    assert all(np.isfinite(N(s)[:2]).all() for s in tr.train_step(batch))
    tr.flush()
    torch.cuda.synchronize()
    rows_4 = R.check(prior, cams, DC.neighbours(cams[:, [7, 11, 15]], 4), min_views=1, rel_tol=0.02)['rows']
    # the trainer's own flags on the written scene: one log line with the totals, for an mse run and for a gnll run, which has neither
    # maps nor a constant: its standard deviation comes from the check
    on_disk = ['--basedir', str(tmp_path), '--datadir', str(tmp_path), '--scene', 'scene', '--cascade_samples', '16,16', '--use_depth',
               '--depth_sup_type', 'noisy', '--lambda_depth', '0.1', '--world_size', '1', '--N_rand_override', '128', '--i_weights', '100',
               '--i_test', '100', '--i_print', '1', '--N_iters', '2', '--testskip', '1', '--depth_cons_views', '4',
               '--depth_cons_min_views', '1', '--depth_cons_rel_tol', '0.02', '--depth_cons_std_floor', '0.05']
    for loss in ('mse', 'gnll'):
        text = _run_nerfpp(on_disk + ['--expname', 'cons_' + loss, '--depth_loss_type', loss])
        found = re.findall(r'depth consistency check \(4 views\): (\d+) frames, (\d+) valid prior pixels, (\d+) verifiable, (\d+) kept, (\d+) dropped', text)
        print('ddp_train_nerf %s: %s' % (loss, found))
        assert len(found) == 1 and [int(v) for v in found[0]] == [len(samplers)] + rows_4.sum(0).tolist(), text[-2000:]
        assert len(re.findall(r'step: \d+ .*level_1/loss_depth: [-\d.e+]+ ', text)) == 2, text[-2000:]


def test_without_the_flags_the_library_is_never_loaded(DC, colmap_scene, monkeypatch, tmp_path):
    """with the library unloaded and its path pointing nowhere, both trainers load their frames and step; with the flags they do not"""
    from outdoor_nerf_depth_amd import mip360_data as D
    monkeypatch.setattr(DC, '_lib', None)
    monkeypatch.setattr(DC, 'LIB_PATH', str(tmp_path / 'libdepthcons_hip.so'))
    base = ["Config.data_dir = '%s'" % colmap_scene[0], "Config.depth_sup_type = 'noisy'", 'Config.sample_every = 1', 'Config.batch_size = 256']
    cfg = D.parse_gin(bindings=base)
    scene = D.Scene(cfg)
    _, sc = _one_mip360_step(scene, scene.device_frames('train', dev()), cfg)
    assert np.isfinite(sc).all()
    text = _run_nerfpp(_nerfpp_argv(tmp_path))
    assert 'depth consistency' not in text and len(re.findall(r'step: \d+ ', text)) == 2
    assert DC._lib is None
    with pytest.raises(DC.DepthConsError, match='libdepthcons_hip.so not found'):
        D.Scene(D.parse_gin(bindings=base + CONS)).device_frames('train', dev())
    with pytest.raises(DC.DepthConsError, match='libdepthcons_hip.so not found'):
        _run_nerfpp(_nerfpp_argv(tmp_path, 'l1', ['--depth_cons_views', '4']))
    assert DC._lib is None


# ------------------------------------------------------------------------------------------------ 6. it does what it is for
def _train_400(data, kind, extra=()):
    """400 steps of 1024 rays from seed 0 -> the float64 mean |last_distance_mean - TRUE depth| over the rays that have a true depth,
    for each of the last 50 batches (the metric of the gnll test)"""
    from outdoor_nerf_depth_amd import mip360 as M
    from outdoor_nerf_depth_amd import mip360_data as D
    from outdoor_nerf_depth_amd import mip360_train as TR
    b = ["Config.data_dir = '%s'" % data, 'Config.max_steps = 400', 'Config.batch_size = 1024', 'Config.lr_delay_steps = 0',
         "Config.depth_sup_type = 'noisy'", 'Config.sample_every = 1', 'Config.compute_disp_metrics = %s' % (kind is not None),
         "Config.depth_loss_type = '%s'" % (kind or 'mse')] + list(extra)
    cfg = D.parse_gin(bindings=b)
    scene = D.Scene(cfg)
    train = scene.device_frames('train', dev())
    tr = TR.make_trainer(cfg, dev(), n_train_frames=train['cams'].shape[0])
    kept = []
    for step in range(400):
        bt = M.sample_batch(train['cams'], train['rgb_u8'], train['depth_sup'], 0, step, 1024, scene.near, scene.far, depth_gt=train['depth_gt'])
        tr.train_step(bt['rays'], bt['rgb'], bt['depth_sup'], jitter01=list(bt['jitter01']))
        if step >= 350:
            kept.append((tr.last_distance_mean, bt['depth_gt']))
    tr.flush()
    torch.cuda.synchronize()
    out = []
    for dm, gt in kept:
        dm, gt = N(dm).astype(np.float64), N(gt).astype(np.float64)
        out.append(np.abs(dm - gt)[gt > 0].mean())
    return np.asarray(out)


def test_filtering_outliers_helps_the_depth_of_an_mse_run(DC, colmap_scene):
    """The analytic scene as a COLMAP scene, 12 frames of 32 x 40, 15 % of the prior's pixels multiplied by 1.5.  Metric: the float64
    mean |distance_mean - depth_gt| over the rays with a true depth, per batch over the last 50 of 400 batches of 1024 rays.  'mse'
    with Config.depth_cons_views = 4 must be lower than plain 'mse' by more than 3 standard errors of the difference of the two means;
    rgb-only is printed."""
    data = str(colmap_scene[0])
    res = {'filtered': _train_400(data, 'mse', ['Config.depth_cons_views = 4']), 'unfiltered': _train_400(data, 'mse'),
           'rgb-only': _train_400(data, None)}
    stat = {k: (e.mean(), e.std(ddof=1) / np.sqrt(len(e))) for k, e in res.items()}
    for k, (mean, se) in stat.items():
        print('%-10s mean |distance_mean - true depth| = %.6f +- %.6f (standard error, 50 batches)' % (k, mean, se))
    gap, se = stat['unfiltered'][0] - stat['filtered'][0], np.hypot(stat['unfiltered'][1], stat['filtered'][1])
    print('unfiltered - filtered = %.6f = %.1f standard errors' % (gap, gap / se))
    gap_rgb = stat['rgb-only'][0] - stat['filtered'][0]
    print('rgb-only - filtered = %.6f = %.1f standard errors' % (gap_rgb, gap_rgb / np.hypot(stat['rgb-only'][1], stat['filtered'][1])))
    assert gap > 3 * se, (gap, se)

"""GPU: the sparse depth prior from a point cloud with tracks (depthpoints_splat, csrc/depthpoints_kernels.hip) against
tests/depth_points_reference.py, through the CLI on both on-disk layouts and through the load-time flags of both trainers.

Gates.  The kernel does the reference's float64 arithmetic in the reference's order without contraction, rounds z to float32 once
as the reference does, takes a minimum over integer keys and counts in integers: nothing is rounded differently, so EVERY output --
depth_out and std_out as their bits, point, origin and rows -- must be EQUAL to the reference.  There is no tolerance.  The cloud is
that of tests/test_depth_points.py: 1 500 world points of the analytic box scene, 200 pushed 30 % farther along their ray, 50
degenerate ones; tracks are the frames whose analytic depth at the projection agrees within 1 %.

Measured on an MI355X (reported figures, not gates).  Every case: equal.  One call on 295 frames of 375 x 1242 with an assumed cloud of
200 000 points and 1.2 M observations (tools/depth_points_bench.py, profiles/depth_points_time.json): `track` 1.340 ms in its
launches and 3.782 ms through the binding, `all` 1.864 ms and 2.936 ms, 2.08 and 2.90 times the compulsory 4.0 GB at 6.2 TB/s.  Flags
off, the `mse` step against the parent commit, medians of 6 alternating runs: MipNeRF-360 7.488 against 7.483 ms (the parent's spread
0.012), NeRF++ 2.0740 against 2.0775 ms (spread 0.013).  Training effect on the per-frame distorted scene, mean |rendered - true
depth| over the last 50 of 400 batches, three seeds: `mse` on the prior aligned to the points 0.267 (max - min 0.041), on the raw
prior 0.876 (0.006), rgb-only about 2.1 on two seeds (the third ends at 1e5 on one ray at the far plane).
"""
import os
import re

import numpy as np
import pytest

torch = pytest.importorskip('torch')
pytestmark = pytest.mark.gpu

from tests import depth_points_reference as R                                            # noqa: E402
from tests.test_gpu_mip360 import T, N, dev                                              # noqa: E402
from tests.test_depth_consistency import SHAPES, write_colmap_scene, write_nerfpp_scene   # noqa: E402
from tests.test_depth_points import EYE, at, bits, cloud, write_points3d_txt               # noqa: E402

OUTPUTS = (('depth', 'depth_out'), ('std', 'std_out'), ('point', 'point'), ('origin', 'origin'), ('rows', 'rows'))
PARAMS = dict(near=0.5, far=12.0, occl_tol=0.05, std_scale=1.5, std_floor=0.002)


@pytest.fixture(scope='module')
def DP():
    dev()
    from outdoor_nerf_depth_amd import depth_points
    return depth_points


def assert_equal(got, ref, tag=''):
    """the call's host outputs against the reference's: equal, the float maps as bits"""
    for mine, theirs in OUTPUTS:
        if mine not in got:
            continue
        a, b = got[mine], ref[theirs]
        assert a.dtype == b.dtype and a.shape == b.shape, (tag, mine, a.dtype, b.dtype, a.shape, b.shape)
        if a.dtype == np.float32:
            a, b = a.view(np.int32), b.view(np.int32)
        np.testing.assert_array_equal(a, b, err_msg='%s: %s' % (tag, mine))


_scatters = {}


def reference(shape, mode, radius):
    """the reference on the cloud of one shape with PARAMS: the scatter computed once per (shape, mode) and shared by the radii"""
    c = cloud(shape)
    if (shape, mode) not in _scatters:
        _scatters[shape, mode] = R.scatter(c['cams'], c['points'], c['obs'] if mode == 'track' else None, shape, PARAMS['near'], PARAMS['far'])
    zbuf, n_obs, n_proj = _scatters[shape, mode]
    depth, std, point, origin, counts = R.resolve(c['cams'], c['points'], zbuf, shape, radius, PARAMS['occl_tol'], PARAMS['std_scale'],
                                                  PARAMS['std_floor'])
    return dict(depth_out=depth, std_out=std, point=point, origin=origin, rows=np.stack([n_obs, n_proj, counts[:, 0], counts[:, 1]], 1))


def run(DP, cams, points, obs, shape, **kw):
    return DP.splat_async(cams, points, obs, shape, device=dev(), **kw).get()


# ------------------------------------------------------------------------------------------------ 1. equality
@pytest.mark.parametrize('radius', (0, 2, 8))
@pytest.mark.parametrize('mode', ('track', 'all'))
@pytest.mark.parametrize('shape', SHAPES)
def test_equal_to_the_reference(DP, shape, mode, radius):
    c = cloud(shape)
    ref = reference(shape, mode, radius)
    got = run(DP, c['cams'], c['points'], c['obs'] if mode == 'track' else None, shape, occl_radius=radius, **PARAMS)
    print('%s %s r=%d: rows total %s' % (shape, mode, radius, got['rows'].sum(0).tolist()))
    assert_equal(got, ref, '%s %s %d' % (shape, mode, radius))
    tot = got['rows'].sum(0)
    assert tot[2] > 300 and (tot[3] > 0) == (radius > 0) and (got['std'][got['origin'] == 1] >= np.float32(0.002)).all()
    assert tot[0] == (len(c['obs']) if mode == 'track' else shape[0] * len(c['points']))
    assert tot[1] == tot[0] if mode == 'track' else tot[1] < tot[0]          # a tracked point projects where it was matched; a frustum holds some


def test_mode_defaults_of_the_radius(DP):
    shape = SHAPES[0]
    c = cloud(shape)
    assert_equal(run(DP, c['cams'], c['points'], c['obs'], shape, **PARAMS), reference(shape, 'track', 0), 'track default')
    four = R.splat(c['cams'], c['points'], None, shape, occl_radius=4, **PARAMS)
    assert_equal(run(DP, c['cams'], c['points'], None, shape, **PARAMS), four, 'all default')


# ------------------------------------------------------------------------------------------------ 2. contention and ties
def test_contention_on_one_pixel_and_ties_go_to_the_lowest_index(DP):
    rs = np.random.RandomState(3)
    n, shape = 4096, (2, 24, 32)
    cams = np.repeat(EYE, 2, 0)
    d = rs.uniform(4.0, 8.0, n)
    tied = np.sort(rs.choice(n, 64, replace=False))
    d[tied] = 2.0 + np.arange(64) * 2.0 ** -40                               # 64 different float64 depths, one float32
    assert len(set(d[tied])) == 64 and len(set(np.float32(d[tied]))) == 1
    jx, jy = rs.uniform(-0.4, 0.4, n), rs.uniform(-0.4, 0.4, n)
    pts = np.stack([(21.5 + jx - 16) / 32 * d, (9.5 + jy - 12) / 32 * d, d, rs.uniform(0.001, 0.01, n)], 1)
    obs = np.stack([np.arange(n), np.ones(n, int)], 1)
    ref = R.splat(cams, pts, obs, shape)
    assert ref['rows'].tolist() == [[0, 0, 0, 0], [n, n, 1, 0]] and ref['point'][1, 9, 21] == tied[0]
    first = run(DP, cams, pts, obs, shape)
    assert_equal(first, ref, 'contention')
    assert first['point'][1, 9, 21] == tied[0] and bits(first['depth'][1, 9, 21]) == bits(2.0)
    for k in range(3):                                                       # repeated, and in another order of the observations
        again = run(DP, cams, pts, obs[rs.permutation(n)] if k else obs, shape)
        assert_equal(again, ref, 'contention, order %d' % k)
    assert_equal(run(DP, cams[1:], pts, None, (1, 24, 32), occl_radius=0), {k: v[1:] for k, v in ref.items()}, 'contention, all')


# ------------------------------------------------------------------------------------------------ 3. edges
def test_edges_of_the_tables_and_the_frame(DP):
    shape = SHAPES[0]
    c = cloud(shape)
    none, nobs = np.zeros((0, 4)), np.zeros((0, 2), np.int32)
    for tag, pts, obs, shp, cams in (('no points, track', none, nobs, shape, c['cams']), ('no points, all', none, None, shape, c['cams']),
                                     ('no observations', c['points'], nobs, shape, c['cams']),
                                     ('one point, all', np.array([at(3, 5, 4.0)]), None, (1, 24, 32), EYE),
                                     ('one point, track', np.array([at(3, 5, 4.0)]), np.array([[0, 0]]), (1, 24, 32), EYE),
                                     ('one frame', c['points'], c['obs'][c['obs'][:, 1] == 0], (1,) + shape[1:], c['cams'][:1])):
        ref = R.splat(cams, pts, obs, shp, **PARAMS)
        assert_equal(run(DP, cams, pts, obs, shp, **PARAMS), ref, tag)
        assert (ref['rows'][:, 2].sum() > 0) == tag.startswith('one'), tag
    # a frame of one pixel
    one = np.array([[1.0, 1.0, 0.5, 0.5] + [1., 0, 0, 0, 0, 1., 0, 0, 0, 0, 1., 0]])
    pts = np.array([[0.0, 0.0, 3.0, 0.01], [0.2, -0.3, 2.0, 0.02], [0.0, 2.0, 2.5, 0.01]])       # the third falls outside
    ref = R.splat(one, pts, None, (1, 1, 1), occl_radius=8)
    assert ref['rows'].tolist() == [[3, 2, 1, 0]] and ref['point'].tolist() == [[[1]]]
    assert_equal(run(DP, one, pts, None, (1, 1, 1), occl_radius=8), ref, '1 x 1')
    # a frame that receives nothing; rows with a frame outside the call are skipped
    obs = c['obs'][c['obs'][:, 1] != 2]
    out = np.concatenate([obs[:40] * (1, 0) + (0, -1), obs, obs[:40] * (1, 0) + (0, shape[0])], 0)
    ref = R.splat(c['cams'], c['points'], obs, shape, **PARAMS)
    assert ref['rows'][2].tolist() == [0, 0, 0, 0] and not ref['origin'][2].any()
    assert_equal(run(DP, c['cams'], c['points'], out, shape, **PARAMS), ref, 'frames outside')
    assert_equal(run(DP, c['cams'], c['points'], out, shape, **PARAMS), R.splat(c['cams'], c['points'], out, shape, **PARAMS), 'frames outside, reference')
    # a row whose point is outside the table is refused with its number, before anything is uploaded
    bad = obs.copy()
    bad[17, 0] = len(c['points'])
    with pytest.raises(DP.DepthPointsError, match='obs: row 17 names point 1750, but the table holds 1750 points'):
        run(DP, c['cams'], c['points'], bad, shape)


# ------------------------------------------------------------------------------------------------ 4. determinism and buffers
def test_repeats_sub_batches_workspace_reuse_and_null_outputs(DP):
    a, b = SHAPES[0], SHAPES[1]
    ca, cb = cloud(a), cloud(b)
    kw = dict(occl_radius=2, **PARAMS)
    first = run(DP, ca['cams'], ca['points'], ca['obs'], a, **kw)
    other = run(DP, cb['cams'], cb['points'], None, b, **kw)                   # another shape takes the second workspace ...
    again = run(DP, ca['cams'], ca['points'], ca['obs'], a, **kw)               # ... and the first is used again
    for k in first:
        np.testing.assert_array_equal(first[k].view(np.uint8), again[k].view(np.uint8), err_msg=k)
    assert_equal(other, reference(b, 'all', 2), 'second shape')
    # a sub-batch of frames with the same points: identical bits for the shared frames, in both modes
    keep = np.array([1, 3, 4])
    sel = np.isin(ca['obs'][:, 1], keep)
    sub_obs = np.stack([ca['obs'][sel, 0], np.searchsorted(keep, ca['obs'][sel, 1])], 1)
    sub = run(DP, ca['cams'][keep], ca['points'], sub_obs, (3,) + a[1:], **kw)
    for k in first:
        np.testing.assert_array_equal(sub[k].view(np.uint8), first[k][keep].view(np.uint8), err_msg='sub-batch, track: ' + k)
    every, sub = run(DP, ca['cams'], ca['points'], None, a, **kw), run(DP, ca['cams'][keep], ca['points'], None, (3,) + a[1:], **kw)
    for k in every:
        np.testing.assert_array_equal(sub[k].view(np.uint8), every[k][keep].view(np.uint8), err_msg='sub-batch, all: ' + k)
    # null optional outputs: the depth alone, the same bits
    for obs in (ca['obs'], None):
        bare = run(DP, ca['cams'], ca['points'], obs, a, std=False, point=False, origin=False, rows=False, **kw)
        assert sorted(bare) == ['depth']
        np.testing.assert_array_equal(bare['depth'].view(np.int32), (first if obs is not None else every)['depth'].view(np.int32))
    d, s, p, rows = DP.splat_priors(ca['cams'], ca['points'], ca['obs'], a, dev(), **kw)
    assert torch.equal(d, T(first['depth'])) and torch.equal(s, T(first['std'])) and torch.equal(p, T(first['point'])) and torch.equal(rows, T(first['rows']))


# ------------------------------------------------------------------------------------------------ 5. the CLI
def _write_cloud(sparse, shape, box):
    """points3D.txt of the cloud of `shape` next to a model of the analytic cameras whose image ids are frame + 1; errors 0.2 .. 1.8 px"""
    c = cloud(shape, box=box)
    tracks = [[] for _ in c['points']]
    for p, f in c['obs']:
        tracks[p].append(f + 1)
    error = np.random.RandomState(4).uniform(0.2, 1.8, len(tracks))
    write_points3d_txt(os.path.join(str(sparse), 'points3D.txt'), c['points'][:, :3], error, tracks)


def _colmap(root, shape, box=True, stems=None):
    """the analytic scene as a COLMAP scene with its cloud; stems: file stems instead of write_colmap_scene's frame_%03d"""
    F, H, W = shape
    names, _ = write_colmap_scene(str(root), F=F, H=H, W=W, box=box)
    if stems is not None:
        from tests.test_mip360_scene import write_colmap
        from tests.test_depth_consistency import analytic_cameras, FOCAL
        _, c2w = analytic_cameras(F, H, W)
        for d in ('images', 'depths_gt', 'depths_noisy'):
            for old, new in zip(names, stems):
                os.rename(str(root / d / old), str(root / d / (new + '.png')))
        for f in os.listdir(str(root / 'sparse' / '0')):
            os.remove(str(root / 'sparse' / '0' / f))
        names = [s + '.png' for s in stems]
        write_colmap(str(root / 'sparse' / '0'), 'PINHOLE', [FOCAL, FOCAL, W / 2.0, H / 2.0], W, H,
                     [(p[:, :3].T, -p[:, :3].T @ p[:, 3]) for p in c2w], names)
    _write_cloud(root / 'sparse' / '0', shape, box)
    return names


def _gin(data, *extra):
    return ["Config.data_dir = '%s'" % data, 'Config.sample_every = 1', 'Config.batch_size = 256'] + list(extra)


def _png(path):
    from PIL import Image
    return np.asarray(Image.open(str(path)))


def test_cli_on_a_colmap_scene(DP, tmp_path):
    from outdoor_nerf_depth_amd import mip360_data as D
    shape = (8, 48, 64)
    data = tmp_path / 'scene'
    names = _colmap(data, shape)
    rows = DP.main(['--data_dir', str(data), '--min_track', '2'])
    scene = D.Scene(D.parse_gin(bindings=_gin(data, "Config.depth_sup_type = 'gt'")))
    prm = DP.check_params('track', **DP.scene_params({'depth_points_min_track': 2}, scene.scale))
    depth, std, point, want = DP.splat_scene(scene, np.arange(len(names)), dev(), prm)
    depth, std = N(depth), N(std)
    np.testing.assert_array_equal(rows, want.cpu().numpy())
    # the direct call is the reference's
    points, obs = DP.scene_points(scene, None, min_track=2)
    call = {k: prm[k] for k in DP.CALL_PARAMS}
    ref = R.splat(DP.cams_from_scene(scene), points, obs, shape, **call)
    assert_equal(dict(depth=depth, std=std, point=point.cpu().numpy(), rows=rows), ref, 'colmap CLI')
    assert rows[:, 2].sum() > 500 and (rows[:, 2] > 20).all()
    assert sorted(os.listdir(str(data / 'depths_points'))) == sorted(os.listdir(str(data / 'depths_points_std'))) == sorted(names)
    for i, name in enumerate(names):                                          # the PNGs are the call's depth rounded to 1 / 256 m
        np.testing.assert_array_equal(_png(data / 'depths_points' / name), DP.encode(depth[i].astype(np.float64) / scene.scale, depth[i] > 0))
        np.testing.assert_array_equal(_png(data / 'depths_points_std' / name), DP.encode(std[i].astype(np.float64) / scene.scale, depth[i] > 0))
    lines = open(str(data / 'points.txt')).read().splitlines()
    assert lines[0].split() == ['#', 'frame'] + list(DP.ROW_NAMES) + ['coverage', 'absrel'] and [l.split()[0] for l in lines[1:]] == names + ['total']
    tot = lines[-1].split()
    assert [int(v) for v in tot[1:5]] == rows.sum(0).tolist() and abs(float(tot[5]) - (depth > 0).mean()) < 1e-6
    print('colmap CLI: totals %s, coverage %s, AbsRel against depths_gt %s' % (rows.sum(0).tolist(), tot[5], tot[6]))
    assert np.isfinite(float(tot[6])) and float(tot[6]) < 0.02                 # tracked points are right to 1 %, and to half a PNG step
    # the loaders find the result under the type 'points', and its standard deviation in a gnll run
    got = D.Scene(D.parse_gin(bindings=_gin(data, "Config.depth_sup_type = 'points'", "Config.depth_loss_type = 'gnll'")))
    assert got.depth_std_source == 'folder' and ((got.depths_sup > 0) == (depth > 0)).all()
    assert (np.abs(got.depths_sup.astype(np.float64) - depth)[depth > 0] / scene.scale).max() <= 0.5 / 256 + 1e-5
    # the other mode presents every point to every frame: before the visibility window no pixel is lost, and the window hides some
    every = DP.main(['--data_dir', str(data), '--min_track', '2', '--vis', 'all', '--occl_radius', '0'])
    assert (every[:, 0] == len(points)).all() and every[:, 1].sum() > rows[:, 1].sum() and (every[:, 2] >= rows[:, 2]).all()
    assert DP.main(['--data_dir', str(data), '--min_track', '2', '--vis', 'all'])[:, 3].sum() > 0


def test_cli_on_a_nerfpp_scene_with_a_model(DP, tmp_path):
    shape = (6, 24, 32)
    stems = ['%06d' % i for i in range(6)]
    scale = write_nerfpp_scene(str(tmp_path), F=6, H=24, W=32)
    model = tmp_path / 'colmap'
    _colmap(model, shape, box=False, stems=stems)
    done = DP.main(['--datadir', str(tmp_path), '--scene', 'scene', '--points_model', str(model / 'sparse' / '0'), '--min_track', '2'])
    assert sorted(done) == ['test', 'train']
    for split in done:
        assert abs(done[split][1] - scale) <= 1e-9 * scale, (split, done[split][1], scale)
        assert done[split][0][:, 2].sum() > 100
        assert os.path.isfile(str(tmp_path / 'scene' / split / 'points.txt'))
    DP.main(['--data_dir', str(model), '--min_track', '2'])                    # the COLMAP-layout run on all six frames
    for s in stems[0::2]:
        np.testing.assert_array_equal(_png(tmp_path / 'scene' / 'train' / 'depth_points' / (s + '.png')), _png(model / 'depths_points' / (s + '.png')),
                                      err_msg=s)
    assert sorted(os.listdir(str(tmp_path / 'scene' / 'test' / 'depth_points_std'))) == [s + '.png' for s in stems[1::2]]
    # poses that are not a shifted, scaled copy of the model's cameras, and a frame the model lacks
    pose = tmp_path / 'scene' / 'train' / 'pose' / '000002.txt'
    kept = pose.read_text()
    m = np.array([float(v) for v in kept.split()]).reshape(4, 4)
    m[1, 3] += 0.01
    pose.write_text(' '.join(repr(float(v)) for v in m.reshape(-1)))
    with pytest.raises(DP.DepthPointsError, match='the pose files are not a shifted, scaled copy of the model\'s cameras: .* frame 000002 is off'):
        DP.main(['--datadir', str(tmp_path), '--scene', 'scene', '--points_model', str(model / 'sparse' / '0')])
    pose.write_text(kept)
    other = tmp_path / 'fewer'
    _colmap(other, (4, 24, 32), box=False, stems=stems[:4])
    with pytest.raises(DP.DepthPointsError, match='frame 000004 is missing from the model'):
        DP.main(['--datadir', str(tmp_path), '--scene', 'scene', '--points_model', str(other / 'sparse' / '0')])


# ------------------------------------------------------------------------------------------------ 6. the load-time flags
@pytest.fixture(scope='module')
def colmap_scene(tmp_path_factory):
    from tests.test_gpu_depth_align import _distort_folder
    dev()
    root = tmp_path_factory.mktemp('depth_points_colmap') / 'scene'
    shape = (12, 32, 40)
    names = _colmap(root, shape)
    _distort_folder(root / 'depths_gt', root / 'depths_mono', 'depth', 3)
    return root, names, shape


POINTS = ["Config.depth_points_vis = 'track'", 'Config.depth_points_min_track = 2', 'Config.depth_points_std_floor = 0.01']
TRAIN = ['Config.max_steps = 2', 'Config.checkpoint_every = 100', 'Config.print_every = 1', 'Config.lr_delay_steps = 0', 'Config.render_chunk_size = 1024']


def _direct(DP, scene):
    """the direct calls for the training split of a scene built with POINTS"""
    points, obs = DP.scene_points(scene, scene.train, min_track=2)
    return DP.splat_priors(DP.cams_from_scene(scene, scene.train), points, obs, (len(scene.train), scene.height, scene.width), dev(),
                           std_floor=0.01 * scene.scale, near=0.5 * scene.scale, far=200.0 * scene.scale)


def test_mip360_flag_computes_the_prior_of_the_training_split_only(DP, colmap_scene, tmp_path):
    from outdoor_nerf_depth_amd import mip360_data as D
    from tests.test_gpu_depth_consistency import _one_mip360_step
    from tests.test_gpu_mip360_app import _run
    data = colmap_scene[0]
    assert not os.path.exists(str(data / 'depths_points')) and not os.path.exists(str(data / 'depths_points_std'))
    base = _gin(data, "Config.depth_sup_type = 'points'", "Config.depth_loss_type = 'gnll'")
    cfg = D.parse_gin(bindings=base + POINTS)
    scene = D.Scene(cfg)
    assert scene.depth_std_source == 'points'
    train = scene.device_frames('train', dev())
    depth, std, _, rows = _direct(DP, scene)
    assert torch.equal(train['depth_sup'], depth) and torch.equal(train['depth_std'], std) and torch.equal(train['depth_points_rows'], rows)
    assert int(rows[:, 2].sum()) > 200 and float(std[depth > 0].min()) >= np.float32(0.01 * scene.scale)
    gt = train['depth_gt']
    m = depth > 0
    assert float(((depth - gt).abs() / gt)[m].max()) < 0.012                                # in scene units, like depths_gt
    test = scene.device_frames('test', dev())
    assert not bool(test['depth_sup'].any()) and 'depth_points_rows' not in test and 'depth_std' not in test
    b, sc = _one_mip360_step(scene, train, cfg)                                            # the step's prior is the computed one
    f, x, y = b['pix'].long().unbind(1)
    assert torch.equal(b['depth_sup'].reshape(-1), train['depth_sup'][f, y, x]) and np.isfinite(sc).all()
    bind = base + POINTS + TRAIN + ["Config.checkpoint_dir = '%s'" % (tmp_path / 'run')]
    out = _run('mip360_train', sum([['--gin_bindings', x] for x in bind], []))
    lines = [l for l in out.splitlines() if l.startswith('sparse-point depth prior')]
    print(lines)
    assert lines == [DP.totals_line(rows.cpu().numpy(), 'track')] and 'step 2/2' in out, out[-2000:]


def test_mip360_flag_computes_the_anchor_of_a_distorted_prior(DP, colmap_scene, tmp_path):
    from outdoor_nerf_depth_amd import depth_align as DAL
    from outdoor_nerf_depth_amd import mip360_data as D
    from outdoor_nerf_depth_amd.depth_consistency import absrel
    from tests.test_gpu_mip360_app import _run
    data = colmap_scene[0]
    base = _gin(data, "Config.depth_sup_type = 'mono'")
    raw = D.Scene(D.parse_gin(bindings=base)).device_frames('train', dev())
    anchored = base + ["Config.depth_align_anchor = 'points'", 'Config.depth_align_min_points = 8'] + POINTS
    scene = D.Scene(D.parse_gin(bindings=anchored))
    assert scene.depth_points_target == 'anchor' and scene.depths_anchor is None
    train = scene.device_frames('train', dev())
    anchor, _, _, rows = _direct(DP, scene)
    want, _, align_rows = DAL.align_priors(raw['depth_sup'], anchor, **scene.depth_align_prm)
    assert torch.equal(train['depth_sup'], want) and torch.equal(train['depth_align_rows'], align_rows) and torch.equal(train['depth_points_rows'], rows)
    assert 'depth_std' not in train
    e0 = absrel(N(raw['depth_sup']), N(raw['depth_gt']), N(raw['depth_sup']) > 0)
    e1 = absrel(N(want), N(train['depth_gt']), N(want) > 0)
    print('anchor: %s points per frame, statuses %s, AbsRel of the training prior %.4f -> %.4f'
          % (rows.cpu().numpy()[:, 2].tolist(), align_rows.cpu().numpy()[:, 5].tolist(), e0, e1))
    assert (align_rows.cpu().numpy()[:, 5] == 0).all() and e1 < 0.02 < e0
    test = scene.device_frames('test', dev())
    assert torch.equal(test['depth_sup'], D.Scene(D.parse_gin(bindings=base)).device_frames('test', dev())['depth_sup'])
    assert 'depth_points_rows' not in test and 'depth_align_rows' not in test
    bind = anchored + TRAIN + ["Config.checkpoint_dir = '%s'" % (tmp_path / 'run')]
    out = _run('mip360_train', sum([['--gin_bindings', x] for x in bind], []))
    lines = [l for l in out.splitlines() if l.startswith(('sparse-point depth prior', 'depth align'))]
    print(lines)
    assert lines[0] == DP.totals_line(rows.cpu().numpy(), 'track') and lines[1] == DAL.totals_line(align_rows.cpu().numpy(), 'points') and 'step 2/2' in out, out[-2000:]


def _nerfpp(tmp_path):
    stems = ['%06d' % i for i in range(8)]
    write_nerfpp_scene(str(tmp_path), F=8)
    _colmap(tmp_path / 'colmap', (8, 24, 32), box=False, stems=stems)
    return str(tmp_path / 'colmap' / 'sparse' / '0')


def test_nerfpp_flag_computes_the_prior_of_the_samplers(DP, tmp_path):
    from outdoor_nerf_depth_amd.data_loader_split import load_data_split
    from outdoor_nerf_depth_amd.device_sampler import DeviceRaySamplers
    from tests.test_gpu_depth_consistency import _run_nerfpp
    model = _nerfpp(tmp_path)
    samplers = load_data_split(str(tmp_path), 'scene', 'train', depth_sup_type='points', depth_std=0.0, depth_std_optional=True)
    assert all(s.depth_sup is None and s.depth_std is None for s in samplers)               # no depth_points/ on disk
    H, W, scale = samplers[0].H, samplers[0].W, samplers[0].depth_scale
    cams = DP.cams_from_samplers(samplers)
    points, obs, s_fit = DP.model_points(model, ['%06d' % i for i in range(0, 8, 2)], cams[:, [7, 11, 15]], min_track=2)
    assert abs(s_fit - scale) < 1e-6 * scale                                                 # (the samplers hold float32 poses)
    ref = R.splat(cams, points, obs, (4, H, W), near=0.5 * scale, far=200.0 * scale, std_floor=0.01 * scale)
    rows, depth = DP.splat_samplers(samplers, dev(), model, 'track', 'prior', want_std=True, min_track=2, near=0.5 * scale, far=200.0 * scale,
                                    std_floor=0.01 * scale)
    np.testing.assert_array_equal(rows, ref['rows'])
    assert rows[:, 2].sum() > 100
    for i, s in enumerate(samplers):                                                           # host sampling reads these
        np.testing.assert_array_equal(s.depth_sup.view(np.int32), ref['depth_out'][i].reshape(-1).view(np.int32))
        np.testing.assert_array_equal(s.depth_std.view(np.int32), ref['std_out'][i].reshape(-1).view(np.int32))
        assert set(s.random_sample(16)) >= {'depth_sup', 'depth_std'}
    ds = DeviceRaySamplers(samplers, dev(), seed=1)                                            # and so does the device sampler
    np.testing.assert_array_equal(N(ds.depth_sup).reshape(len(samplers), -1), ref['depth_out'].reshape(len(samplers), -1))
    gt = np.stack([s.depth_gt for s in samplers], 0)
    m = depth > 0
    assert (np.abs(depth - gt)[m] / gt[m]).max() < 0.011 + 0.5 / 256 / 3.0                    # scene units, like depth/ (a PNG of metres x 256)
    # the trainer's own flags: one log line with the totals; the gnll loss reads the computed standard deviation
    argv = ['--basedir', str(tmp_path), '--datadir', str(tmp_path), '--scene', 'scene', '--cascade_samples', '16,16', '--use_depth',
            '--lambda_depth', '0.1', '--world_size', '1', '--N_rand_override', '128', '--i_weights', '100', '--i_test', '100', '--i_print', '1',
            '--N_iters', '2', '--testskip', '1', '--depth_points_model', model, '--depth_points_min_track', '2']
    text = _run_nerfpp(argv + ['--expname', 'points', '--depth_sup_type', 'points', '--depth_loss_type', 'gnll', '--depth_points_std_floor', '0.01'])
    found = [l for l in text.splitlines() if l.startswith('sparse-point depth prior')]
    print(found)
    assert found == [DP.totals_line(rows, 'track')], text[-2000:]
    assert len(re.findall(r'step: \d+ .*level_1/loss_depth: [-\d.e+]+ ', text)) == 2, text[-2000:]
    # as the anchor of the noisy prior: the alignment's line follows
    text = _run_nerfpp(argv + ['--expname', 'anchor', '--depth_sup_type', 'noisy', '--depth_align_anchor', 'points', '--depth_align_min_points', '8'])
    found = [l for l in text.splitlines() if l.startswith(('sparse-point depth prior', 'depth align'))]
    print(found)
    assert len(found) == 2 and found[0].startswith('sparse-point depth prior (track): 4 frames') and found[1].startswith('depth align'), text[-2000:]
    assert len(re.findall(r'step: \d+ ', text)) == 2


def test_without_the_flags_the_library_is_never_loaded(DP, colmap_scene, monkeypatch, tmp_path):
    """with the library unloaded and its path pointing nowhere, both trainers load their frames and step; with the flags they do not"""
    from outdoor_nerf_depth_amd import mip360_data as D
    from tests.test_gpu_depth_consistency import _one_mip360_step, _run_nerfpp, _nerfpp_argv
    monkeypatch.setattr(DP, '_lib', None)
    monkeypatch.setattr(DP, 'LIB_PATH', str(tmp_path / 'libdepthpoints_hip.so'))
    base = _gin(colmap_scene[0], "Config.depth_sup_type = 'mono'")
    cfg = D.parse_gin(bindings=base)
    scene = D.Scene(cfg)
    _, sc = _one_mip360_step(scene, scene.device_frames('train', dev()), cfg)
    assert np.isfinite(sc).all()
    text = _run_nerfpp(_nerfpp_argv(tmp_path))
    assert 'sparse-point' not in text and len(re.findall(r'step: \d+ ', text)) == 2
    assert DP._lib is None
    with pytest.raises(DP.DepthPointsError, match='libdepthpoints_hip.so not found'):
        D.Scene(D.parse_gin(bindings=_gin(colmap_scene[0], "Config.depth_sup_type = 'points'") + POINTS)).device_frames('train', dev())
    model = _nerfpp(tmp_path / 'n')
    with pytest.raises(DP.DepthPointsError, match='libdepthpoints_hip.so not found'):
        _run_nerfpp(['--basedir', str(tmp_path), '--datadir', str(tmp_path / 'n'), '--scene', 'scene', '--cascade_samples', '16,16', '--use_depth',
                     '--depth_sup_type', 'points', '--world_size', '1', '--N_rand_override', '128', '--N_iters', '2', '--expname', 'off',
                     '--depth_points_model', model])
    assert DP._lib is None

"""No GPU: the sparse depth prior from the reconstruction's point cloud -- the points3D readers, the host selection
(scene_points against the reference's loop), the reference on exactly representable geometry, the fit of a shift and a scale to
matched camera centres, the library's argument checks and both flag surfaces.  The cloud of tests/test_gpu_depth_points.py and the
writer of points3D.txt live here.

Exactly representable geometry: an identity camera with fx = fy = 32, cx = 16, cy = 12 and points at
((u + 0.5 - cx) / fx * d, (v + 0.5 - cy) / fy * d, d) with d a power of two: every product and quotient of the projection is exact,
so the pixel is (u, v) and the depth float32(d) with no rounding anywhere.
"""
import os
import struct
import subprocess
import sys
from types import SimpleNamespace

import numpy as np
import pytest

from outdoor_nerf_depth_amd import depth_consistency as DC
from outdoor_nerf_depth_amd import depth_points as P
from outdoor_nerf_depth_amd import mip360_data as D
from tests import depth_points_reference as R
from tests.test_depth_consistency import analytic_cameras, analytic_scene, axis_angle, write_colmap_scene
from tests.test_depth_mvs import world_points

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------------ shared with the GPU tests
def write_points3d_txt(path, xyz, error, tracks):
    """points3D.txt from the format: POINT3D_ID X Y Z R G B ERROR then (IMAGE_ID POINT2D_IDX) pairs; tracks: lists of image ids"""
    with open(path, 'w') as f:
        f.write('# 3D point list with one line of data per point:\n#   POINT3D_ID, X, Y, Z, R, G, B, ERROR, TRACK[] as (IMAGE_ID, POINT2D_IDX)\n')
        for k, (p, e, tr) in enumerate(zip(xyz, error, tracks)):
            f.write('%d %s 128 128 128 %r %s\n' % (k + 1, ' '.join(repr(float(v)) for v in p), float(e),
                                                   ' '.join('%d %d' % (int(i), j) for j, i in enumerate(tr))))


def write_points3d_bin(path, xyz, error, tracks):
    with open(path, 'wb') as f:
        f.write(struct.pack('<Q', len(xyz)))
        for k, (p, e, tr) in enumerate(zip(xyz, error, tracks)):
            f.write(struct.pack('<QdddBBBdQ', k + 1, p[0], p[1], p[2], 128, 128, 128, e, len(tr)))
            for j, i in enumerate(tr):
                f.write(struct.pack('<ii', int(i), j))


_clouds = {}


def cloud(shape, seed=0, box=True):
    """{'points' [1750, 4], 'obs' int32 [T, 2] sorted by (frame, point), 'cams', 'shape'} for the analytic scene (with its box, or without) of one shape, built
    once and shared (read-only): the world points of 1 500 random pixels of random frames, 200 of them again 30 % farther along their
    ray (something to hide), and 50 degenerate points (NaN, behind every camera, beyond far); a point's track is the frames whose
    analytic depth at its projection agrees within 1 %; coef is random in 0.001 .. 0.01."""
    key = (tuple(shape), seed, box)
    if key not in _clouds:
        F, H, W = shape
        s = analytic_scene(shape, box=box)
        rs = np.random.RandomState(seed)
        world = world_points(s['K'], s['c2w'], s['depth'])
        f, y, x = rs.randint(0, F, 1500), rs.randint(0, H, 1500), rs.randint(0, W, 1500)
        near_pts = world[f, y, x]
        k = rs.choice(1500, 200, replace=False)
        centre = s['c2w'][f[k], :, 3]
        far_pts = centre + 1.3 * (near_pts[k] - centre)
        bad = np.zeros((50, 3))
        bad[:15] = np.nan
        bad[15:30] = (1.0, 0.0, -5.0)                                 # behind every camera
        bad[30:] = (1.0, 0.0, 500.0)                                  # beyond far
        xyz = np.concatenate([near_pts, far_pts, bad], 0)
        xyz = xyz[rs.permutation(len(xyz))]
        points = np.concatenate([xyz, rs.uniform(0.001, 0.01, (len(xyz), 1))], 1)
        obs = []
        with np.errstate(all='ignore'):
            for i in range(F):
                c = s['cams'][i]
                Pc = np.stack(R.to_cam(c, (xyz[:, 0], xyz[:, 1], xyz[:, 2])), 1)
                u, v = c[0] * Pc[:, 0] / Pc[:, 2] + c[2], c[1] * Pc[:, 1] / Pc[:, 2] + c[3]
                ok = (Pc[:, 2] > 0) & (u >= 0) & (u < W) & (v >= 0) & (v < H)
                px, py = np.where(ok, np.floor(u), 0).astype(int), np.where(ok, np.floor(v), 0).astype(int)
                ok &= np.abs(s['depth'][i][py, px] - Pc[:, 2]) <= 0.01 * Pc[:, 2]
                obs += [(int(p), i) for p in np.nonzero(ok)[0]]
        obs = np.array(sorted(obs, key=lambda r: (r[1], r[0])), np.int32)
        for a in (points, obs):
            a.setflags(write=False)
        _clouds[key] = dict(points=points, obs=obs, cams=s['cams'], shape=tuple(shape))
    return _clouds[key]


# ------------------------------------------------------------------------------------------------ 1. the readers
XYZ = np.array([[0.5, -0.25, 4.0], [1.0, 2.0, 8.0], [-3.0, 0.125, 16.0]])
ERR = np.array([0.5, 1.25, 3.0])
TRACKS = [[1, 2, 3], [2, 4], [1, 2, 3, 4]]


def test_text_and_binary_readers_agree(tmp_path):
    write_points3d_txt(str(tmp_path / 'points3D.txt'), XYZ, ERR, TRACKS)
    write_points3d_bin(str(tmp_path / 'points3D.bin'), XYZ, ERR, TRACKS)
    txt, binary = D.read_points3d_txt(str(tmp_path / 'points3D.txt')), D.read_points3d_bin(str(tmp_path / 'points3D.bin'))
    for a, b, dtype in zip(txt, binary, (np.float64, np.float64, np.int64, np.int32)):
        assert a.dtype == b.dtype == dtype
        np.testing.assert_array_equal(a, b)
    xyz, error, off, image_id = D.read_points3d(str(tmp_path))                                 # binary preferred
    np.testing.assert_array_equal(xyz, XYZ)
    np.testing.assert_array_equal(error, ERR)
    assert off.tolist() == [0, 3, 5, 9] and image_id.tolist() == [1, 2, 3, 2, 4, 1, 2, 3, 4]
    os.remove(str(tmp_path / 'points3D.bin'))
    assert D.read_points3d(str(tmp_path))[2].tolist() == [0, 3, 5, 9]                          # text otherwise
    os.remove(str(tmp_path / 'points3D.txt'))
    with pytest.raises(FileNotFoundError, match='points3D.bin / points3D.txt'):
        D.read_points3d(str(tmp_path))


def test_readers_refuse_empty_and_truncated_files_by_name(tmp_path):
    empty = tmp_path / 'points3D.txt'
    empty.write_text('# 3D point list with one line of data per point:\n# Number of points: 0, mean track length: 0\n')
    with pytest.raises(ValueError, match=r'points3D.txt holds no 3D point'):
        D.read_points3d_txt(str(empty))
    write_points3d_bin(str(tmp_path / 'none.bin'), [], [], [])
    with pytest.raises(ValueError, match=r'none.bin holds no 3D point'):
        D.read_points3d_bin(str(tmp_path / 'none.bin'))
    write_points3d_bin(str(tmp_path / 'full.bin'), XYZ, ERR, TRACKS)
    data = (tmp_path / 'full.bin').read_bytes()
    for cut, point in ((4, 0), (8 + 20, 0), (8 + 51 + 8 * 3 + 51 + 4, 1), (len(data) - 1, 2)):
        (tmp_path / 'cut.bin').write_bytes(data[:cut])
        with pytest.raises(ValueError, match=r'cut.bin is truncated: it ends before point %d is complete' % point):
            D.read_points3d_bin(str(tmp_path / 'cut.bin'))
    (tmp_path / 'cut.txt').write_text('1 0.5 -0.25 4.0 128 128 128 0.5 1 0 2 1\n2 1.0 2.0 8.0 128 128\n')
    with pytest.raises(ValueError, match=r'cut.txt is truncated: data line 2 has 6 fields'):
        D.read_points3d_txt(str(tmp_path / 'cut.txt'))
    (tmp_path / 'odd.txt').write_text('1 0.5 -0.25 4.0 128 128 128 0.5 1 0 2\n')
    with pytest.raises(ValueError, match=r'odd.txt is truncated: data line 1 has 11 fields'):
        D.read_points3d_txt(str(tmp_path / 'odd.txt'))


# ------------------------------------------------------------------------------------------------ 2. scene_points
def _model(tmp_path, F=6, tracks=None, xyz=None, error=None):
    """A COLMAP model of the analytic cameras (image ids 1 .. F) with the given points, and what scene_points reads of a Scene"""
    from tests.test_mip360_scene import write_colmap
    K, c2w = analytic_cameras(F, 24, 32)
    names = ['frame_%03d.png' % i for i in range(F)]
    sparse = str(tmp_path / 'sparse' / '0')
    write_colmap(sparse, 'PINHOLE', [30.0, 30.0, 16.0, 12.0], 32, 24, [(p[:, :3].T, -p[:, :3].T @ p[:, 3]) for p in c2w], names)
    if xyz is not None:
        write_points3d_txt(os.path.join(sparse, 'points3D.txt'), xyz, error, tracks)
    got, poses, _, _ = D.load_colmap_poses(sparse)
    assert got == names
    poses, transform = D.transform_poses_pca(poses)
    return SimpleNamespace(sparse_dir=sparse, names=names, poses=poses, transform=transform), c2w


def test_scene_points_selects_transforms_and_sorts(tmp_path):
    rs = np.random.RandomState(0)
    xyz = rs.uniform(-2, 2, (40, 3)) + (0, 0, 6)
    error = rs.uniform(0.1, 1.9, 40)
    tracks = [sorted(rs.choice(6, rs.randint(3, 6), replace=False) + 1) for _ in range(40)]
    error[0] = 2.5                                                                              # over max_error
    error[1] = -0.1                                                                             # a negative error
    tracks[2] = [1, 5]                                                                          # under min_track
    tracks[3] = [4, 4, 4]                                                                       # its cameras coincide: B = 0
    xyz[4, 1] = np.inf                                                                          # not finite
    tracks[5] = [2, 4, 6]                                                                       # no entry in the split below ...
    tracks[6] = [1, 2, 4, 6]                                                                    # ... and one
    error[7] = 0.2                                                                              # under err_floor
    scene, c2w = _model(tmp_path, 6, tracks, xyz, error)
    idx = np.array([0, 2, 4])                                                                   # image ids 1, 3, 5
    points, obs = P.scene_points(scene, idx, max_error=2.0, min_track=3, err_floor=0.5)
    assert points.dtype == np.float64 and obs.dtype == np.int32 and points.shape == (35, 4) and obs.shape[1] == 2
    # the reference's loop on the same cloud in the scene's frame
    T = scene.transform
    in_scene = xyz @ T[:3, :3].T + T[:3, 3]
    off = np.concatenate([[0], np.cumsum([len(t) for t in tracks])])
    track_pos = np.concatenate(tracks) - 1
    frame_of = np.array([0, -1, 1, -1, 2, -1])
    ref_points, ref_obs, kept = R.select(in_scene, error, off, track_pos, scene.poses[:, :3, 3], frame_of, 2.0, 3, 0.5)
    assert kept.tolist() == [False] * 5 + [True] * 35
    np.testing.assert_array_equal(points, ref_points)
    np.testing.assert_array_equal(obs, ref_obs)
    # entries outside the split are no observation, but count towards min_track and B
    assert not (obs[:, 0] == 0).any() and obs[obs[:, 0] == 1].tolist() == [[1, 0]]              # points 5 and 6 are 0 and 1 now
    scale = float(np.sqrt((T[:3, :3] @ T[:3, :3].T)[0, 0]))
    c = scene.poses[[1, 3, 5], :3, 3]                                                           # (the box is the scene frame's)
    B5 = np.sqrt(((c.max(0) - c.min(0)) ** 2).sum())
    assert abs(points[0, 3] - error[5] / B5) < 1e-12 * points[0, 3]
    assert abs(points[2, 3] * (error[7] / 0.5) - P.scene_points(scene, idx, err_floor=0.1)[0][2, 3]) < 1e-12      # the floor held
    # sorted by (frame, point), every row inside the tables
    assert (np.lexsort((obs[:, 0], obs[:, 1])) == np.arange(len(obs))).all()
    assert obs[:, 0].max() < 35 and set(obs[:, 1].tolist()) == {0, 1, 2}
    # the points are in the scene's frame: a kept point's depth in an observing frame is positive and scene-sized
    cams = DC.pack_cams(np.array([[30.0, 0, 16], [0, 30.0, 12], [0, 0, 1]]), scene.poses[idx] * np.array([1., -1., -1., 1.]))
    z = np.array([R.to_cam(cams[f], points[p, :3])[2] for p, f in obs])
    assert (z > 0).all() and abs(np.median(z) / scale - 6.0) < 1.5
    # all frames: None
    assert len(P.scene_points(scene)[1]) == sum(len(t) for k, t in enumerate(tracks) if kept[k])
    # a stricter selection
    assert len(P.scene_points(scene, idx, max_error=1.0)[0]) == int((kept & (error <= 1.0)).sum())
    assert len(P.scene_points(scene, idx, min_track=5)[0]) == int((kept & (np.array([len(t) for t in tracks]) >= 5)).sum())


def test_scene_points_refuses_an_image_id_outside_the_model_and_an_empty_cloud(tmp_path):
    scene, _ = _model(tmp_path / 'a', 4, [[1, 2, 3], [2, 3, 9]], XYZ[:2], ERR[:2])
    with pytest.raises(P.DepthPointsError, match=r'a track names image id 9, which is not among the model\'s images'):
        P.scene_points(scene)
    scene, _ = _model(tmp_path / 'b', 4)
    with pytest.raises(FileNotFoundError, match='no 3D points'):
        P.scene_points(scene)
    open(os.path.join(scene.sparse_dir, 'points3D.txt'), 'w').close()                           # what a run from known poses leaves
    with pytest.raises(ValueError, match='points3D.txt holds no 3D point'):
        P.scene_points(scene)


# ------------------------------------------------------------------------------------------------ 3. the reference, exactly
EYE = DC.pack_cams(np.array([[32.0, 0, 16], [0, 32.0, 12], [0, 0, 1]]), np.eye(4)[None, :3])
SHAPE = (1, 24, 32)


def at(u, v, d, coef=0.01):
    return ((u + 0.5 - 16) / 32 * d, (v + 0.5 - 12) / 32 * d, d, coef)


def bits(a):
    return np.asarray(a, np.float32).view(np.uint32)


def test_reference_on_exactly_representable_geometry():
    pts = np.array([at(3, 5, 4.0), at(20, 7, 8.0), at(20, 7, 2.0), at(9, 9, 16.0), at(9, 9, 16.0), at(31, 23, 1.0), at(0, 0, 64.0)])
    out = R.splat(EYE, pts, None, SHAPE)
    assert out['rows'].tolist() == [[7, 7, 5, 0]]
    for (u, v), d, idx in (((3, 5), 4.0, 0), ((20, 7), 2.0, 2), ((9, 9), 16.0, 3), ((31, 23), 1.0, 5), ((0, 0), 64.0, 6)):
        assert bits(out['depth_out'][0, v, u]) == bits(d) and out['point'][0, v, u] == idx and out['origin'][0, v, u] == R.ORIGIN_POINT
    assert (out['origin'] == R.ORIGIN_POINT).sum() == 5 and (out['depth_out'] > 0).sum() == 5 and (out['point'] >= 0).sum() == 5
    # the nearer of two wins whatever their order; equal depths go to the lower index
    assert R.splat(EYE, pts[[2, 1]], None, SHAPE)['point'][0, 7, 20] == 0
    assert R.splat(EYE, pts[[1, 2]], np.array([[1, 0], [0, 0]]), SHAPE)['point'][0, 7, 20] == 1
    # behind the camera, outside the frame, nearer than near, farther than far: nothing, and not counted as projected
    out_of = np.array([at(3, 5, -4.0), at(32, 5, 4.0), at(-1, 5, 4.0), at(3, 24, 4.0), at(3, -1, 4.0), at(3, 5, 0.25), at(3, 5, 256.0),
                       (np.nan, 0, 4.0, 0.01), (0, 0, np.inf, 0.01)])
    out = R.splat(EYE, out_of, None, SHAPE)
    assert out['rows'].tolist() == [[9, 0, 0, 0]] and not out['depth_out'].any() and (out['point'] == -1).all() and not out['origin'].any()
    assert R.splat(EYE, out_of[5:7], None, SHAPE, near=0.25, far=256.0)['rows'].tolist() == [[2, 2, 1, 0]]      # the range is closed
    # obs rows outside the tables are skipped
    out = R.splat(EYE, pts, np.array([[0, 0], [1, -1], [1, 1], [7, 0], [-1, 0]]), SHAPE)
    assert out['rows'].tolist() == [[1, 1, 1, 0]] and out['point'][0, 5, 3] == 0
    # a far point next to a near one: hidden at radius 1, a point at radius 0; within the tolerance it stays
    pair = np.array([at(10, 10, 2.0), at(11, 10, 8.0), at(11, 11, 2.0625)])
    r0, r1 = R.splat(EYE, pair, None, SHAPE, occl_radius=0), R.splat(EYE, pair, None, SHAPE, occl_radius=1)
    assert r0['origin'][0, 10, 11] == R.ORIGIN_POINT and r0['rows'].tolist() == [[3, 3, 3, 0]]
    assert r1['origin'][0, 10, 11] == R.ORIGIN_HIDDEN and r1['depth_out'][0, 10, 11] == 0 and r1['point'][0, 10, 11] == -1
    assert r1['std_out'][0, 10, 11] == 0 and r1['rows'].tolist() == [[3, 3, 2, 1]] and r1['origin'][0, 11, 11] == R.ORIGIN_POINT
    assert R.splat(EYE, pair, None, SHAPE, occl_radius=1, occl_tol=0.03)['rows'].tolist() == [[3, 3, 1, 2]]
    assert R.splat(EYE, pair, None, SHAPE, occl_radius=1, occl_tol=3.0)['rows'].tolist() == [[3, 3, 3, 0]]      # 8 <= 2 * (1 + 3)
    # the standard deviation: std_scale * coef * z * z / fx, floored, rounded once
    one = np.array([at(3, 5, 4.0, 0.01), at(4, 5, 8.0, 0.003)])
    s = R.splat(EYE, one, None, SHAPE, std_scale=2.0)['std_out']
    assert bits(s[0, 5, 3]) == bits(np.float32(2.0 * 0.01 * 4.0 * 4.0 / 32.0)) and bits(s[0, 5, 4]) == bits(np.float32(2.0 * 0.003 * 8.0 * 8.0 / 32.0))
    s = R.splat(EYE, one, None, SHAPE, std_floor=0.0055)['std_out']
    assert bits(s[0, 5, 3]) == bits(np.float32(0.0055)) and bits(s[0, 5, 4]) == bits(np.float32(0.003 * 64.0 / 32.0))
    assert (s > 0).sum() == 2


def test_reference_track_and_all_modes_on_the_cloud():
    shape = (6, 24, 32)
    c = cloud(shape)
    track, every = R.splat(c['cams'], c['points'], c['obs'], shape, far=12.0), R.splat(c['cams'], c['points'], None, shape, far=12.0, occl_radius=2)
    assert (track['rows'][:, 0] == np.bincount(c['obs'][:, 1], minlength=6)).all() and (every['rows'][:, 0] == 1750).all()
    assert (track['rows'][:, 1] <= track['rows'][:, 0]).all() and (every['rows'][:, 1] >= track['rows'][:, 1]).all()
    assert track['rows'][:, 2].sum() > 500 and every['rows'][:, 3].sum() > 20 and track['rows'][:, 3].sum() == 0
    # a tracked point is visible where it was matched: against the analytic depth the track mode is right to 1 %
    d = analytic_scene(shape, box=True)['depth']
    kept = track['origin'] == R.ORIGIN_POINT
    assert (np.abs(track['depth_out'][kept] - d[kept]) <= 0.011 * d[kept]).all()


# ------------------------------------------------------------------------------------------------ 4. the fit of a shift and a scale
def test_similarity_fit_recovers_a_shift_and_a_scale_and_refuses_anything_else(tmp_path):
    _, c2w = analytic_cameras(8, 24, 32)
    c = c2w[:, :, 3]
    names = ['%06d' % i for i in range(8)]
    s, t = P.fit_similarity(c, 0.05 * c + (0.3, -0.2, 0.1), names)
    assert abs(s - 0.05) <= 1e-12 and np.abs(t - (0.3, -0.2, 0.1)).max() <= 1e-12
    rot = axis_angle((0.2, 1.0, 0.1), 0.05)
    with pytest.raises(P.DepthPointsError, match=r'the pose files are not a shifted, scaled copy of the model\'s cameras: .* frame 00000\d is off'):
        P.fit_similarity(c, 0.05 * c @ rot.T + (0.3, -0.2, 0.1), names)
    with pytest.raises(P.DepthPointsError, match='not a shifted, scaled copy'):
        P.fit_similarity(c, -0.05 * c, names)                                                   # a mirrored copy
    with pytest.raises(P.DepthPointsError, match='at least two frames'):
        P.fit_similarity(c[:1], c[:1], names[:1])
    # through a model on disk: frames matched by file stem, a frame the model lacks is named
    scene, c2w = _model(tmp_path, 6, TRACKS, XYZ, ERR)
    stems = ['frame_004', 'frame_001', 'frame_003']
    points, obs, s = P.model_points(scene.sparse_dir, stems, 0.05 * c2w[[4, 1, 3], :, 3] + 1.0, max_error=2.0, min_track=3)
    assert abs(s - 0.05) <= 1e-12 and np.abs(points[:, :3] - (0.05 * XYZ[:1] + 1.0)).max() <= 1e-12
    assert obs.tolist() == [[0, 1]]                                                             # of ids 1, 2, 3 only id 2 is a frame: position 1
    with pytest.raises(P.DepthPointsError, match=r'frame frame_017 is missing from the model in .* \(1 of 3 frames are'):
        P.model_points(scene.sparse_dir, ['frame_001', 'frame_017', 'frame_003'], c2w[[1, 2, 3], :, 3])


# ------------------------------------------------------------------------------------------------ 5. the binding without a device
def test_check_params_defaults_and_refusals():
    assert P.check_params() == dict(vis='track', max_error=2.0, min_track=3, err_floor=0.5, near=0.5, far=200.0, occl_radius=0, occl_tol=0.05,
                                    std_scale=1.0, std_floor=0.0)
    assert P.check_params('all')['occl_radius'] == 4 and P.check_params('all', occl_radius=0)['occl_radius'] == 0
    assert P.check_params('track', occl_radius=8)['occl_radius'] == 8
    for kw, text in ((dict(vis='some'), "vis = 'some': expected 'track' or 'all'"), (dict(max_error=-1.0), 'max_error = -1.0'),
                     (dict(max_error=float('nan')), 'max_error = nan'), (dict(min_track=0), 'min_track = 0'), (dict(min_track=2.5), 'min_track = 2.5'),
                     (dict(err_floor=-0.5), 'err_floor = -0.5'), (dict(near=0.0), 'near = 0.0, far = 200.0'), (dict(near=3.0, far=2.0), 'near = 3.0, far = 2.0'),
                     (dict(far=float('inf')), 'far = inf'), (dict(occl_radius=9), 'occl_radius = 9: expected an integer 0 .. 8'),
                     (dict(occl_radius=-1), 'occl_radius = -1'), (dict(occl_radius=1.5), 'occl_radius = 1.5'), (dict(occl_tol=-0.1), 'occl_tol = -0.1'),
                     (dict(std_scale=0.0), 'std_scale = 0.0'), (dict(std_scale=float('inf')), 'std_scale = inf'), (dict(std_floor=-1.0), 'std_floor = -1.0')):
        with pytest.raises(P.DepthPointsError, match=text):
            P.check_params(**kw)


def test_host_checks_name_the_argument_before_the_device_is_asked():
    pts = np.array([at(3, 5, 4.0)])
    for args, text in (((EYE[:, :15], pts, None, SHAPE), r'cams: expected float64 \[F, 16\]'), ((EYE, pts, None, (2, 24, 32)), 'cams: 1 cameras for 2 frames'),
                       ((EYE, pts[:, :3], None, SHAPE), r'points: expected float64 \[P, 4\]'), ((EYE, pts, None, (24, 32)), r'shape: expected \(F, H, W\)'),
                       ((EYE, pts, np.zeros((1, 2)), SHAPE), 'obs: expected an integer array'), ((EYE, pts, np.zeros((2, 3), int), SHAPE), r'obs: expected \[T, 2\]'),
                       ((EYE, pts, np.array([[0, 0], [0, 5], [1, 0]]), SHAPE), 'obs: row 2 names point 1, but the table holds 1 points'),
                       ((EYE, pts, np.array([[-1, 0]]), SHAPE), 'obs: row 0 names point -1')):
        with pytest.raises(P.DepthPointsError, match=text):
            P.splat_async(*args, device='cuda:0')
    with pytest.raises(P.DepthPointsError, match='occl_radius = 9'):
        P.splat_async(EYE, pts, None, SHAPE, device='cuda:0', occl_radius=9)
    with pytest.raises(P.DepthPointsError, match='expected a CUDA/HIP device'):
        P.splat_async(EYE, pts, None, SHAPE, device='cpu')


def test_workspace_bytes_limits():
    assert P.workspace_bytes(1, 1, 1) == 256 * 3                                            # one key, one tile's partials, one frame's counters
    n, tiles = 295 * 375 * 1242, 47 * 39
    assert P.workspace_bytes(295, 375, 1242) == (8 * n + 255) // 256 * 256 + (295 * tiles * 8 + 255) // 256 * 256 + (295 * 16 + 255) // 256 * 256
    assert P.workspace_bytes(65535, 8, 32) > 0 and P.workspace_bytes(1, 1 << 14, 1 << 14) > 0
    for args, text in (((0, 4, 4), 'n_frames = 0, expected 1 .. 65535'), ((65536, 4, 4), 'n_frames = 65536'),
                       ((1, 0, 4), 'a frame has at least one pixel'), ((1, 4, -1), 'a frame has at least one pixel'),
                       ((1, (1 << 14) + 1, 1 << 14), 'exceeds 2\\^28 pixels per frame')):
        with pytest.raises(P.DepthPointsError, match=text):
            P.workspace_bytes(*args)


def test_binding_declares_the_headers_symbols_and_constants():
    import re
    header = open(os.path.join(ROOT, 'include', 'depthpoints_hip.h')).read()
    declared = set(re.findall(r'^(?:const char\*|int64_t|int) (depthpoints_\w+)\(', header, re.M))
    assert declared == set(P.SYMBOLS) and len(declared) == 4
    const = dict((k, v) for k, v in re.findall(r'#define DEPTHPOINTS_(\w+) \(?(\d+)', header))
    assert tuple(int(const[k]) for k in ('ABI_VERSION', 'MAX_FRAMES', 'MAX_POINTS', 'MAX_RADIUS', 'CAM', 'POINT', 'OBS', 'ROW')) == \
        (P.ABI_VERSION, P.MAX_FRAMES, P.MAX_POINTS, P.MAX_RADIUS, DC.CAM, 4, 2, len(P.ROW_NAMES))
    assert [int(const['ORIGIN_' + k]) for k in ('NONE', 'POINT', 'HIDDEN')] == [P.ORIGIN_NONE, P.ORIGIN_POINT, P.ORIGIN_HIDDEN] \
        == [R.ORIGIN_NONE, R.ORIGIN_POINT, R.ORIGIN_HIDDEN]
    assert [int(const[k.upper()]) for k in P.ROW_NAMES] == [0, 1, 2, 3]
    assert len(P.SYMBOLS['depthpoints_splat'][1]) == header.split('int depthpoints_splat(')[1].split(');')[0].count(',') + 1


def test_library_argument_checks_need_no_gpu():
    import ctypes as C
    lib = P.lib()
    assert lib.depthpoints_abi_version() == P.ABI_VERSION
    buf = (C.c_double * 16384)()                                                 # host memory: every call below fails before any launch
    base = (C.addressof(buf) + 255) // 256 * 256
    at_ = lambda k: C.c_void_p(base + 4096 * k)

    def call(F=1, H=2, W=2, cams=at_(0), P_=4, points=at_(1), T=4, obs=at_(2), near=0.5, far=200.0, radius=0, tol=0.05, scale=1.0, floor=0.0,
             ws=at_(12), depth=at_(4), std=None, point=None, origin=None, rows=None):
        return lib.depthpoints_splat(None, F, H, W, cams, P_, points, T, obs, near, far, radius, tol, scale, floor, ws, depth, std, point,
                                     origin, rows)
    for kw, text in ((dict(F=0), 'n_frames = 0'), (dict(F=65536), 'n_frames = 65536'), (dict(H=0), 'at least one pixel'),
                     (dict(H=1 << 15, W=1 << 14), 'exceeds 2^28 pixels'), (dict(P_=-1), 'n_points = -1, expected 0 .. 2^31 - 1'),
                     (dict(P_=1 << 31), 'n_points = 2147483648'), (dict(T=-1), 'n_obs = -1, expected 0 .. 2^40'), (dict(T=(1 << 40) + 1), 'n_obs = 1099511627777'),
                     (dict(near=0.0), 'near = 0, far = 200'), (dict(near=5.0, far=5.0), 'near = 5, far = 5'), (dict(far=float('inf')), 'far = inf'),
                     (dict(near=float('nan')), 'near = nan'), (dict(radius=-1), 'occl_radius = -1, expected 0 .. 8'), (dict(radius=9), 'occl_radius = 9'),
                     (dict(tol=-0.5), 'occl_tol = -0.5'), (dict(tol=float('nan')), 'occl_tol = nan'), (dict(scale=0.0), 'std_scale = 0'),
                     (dict(scale=float('inf')), 'std_scale = inf'), (dict(floor=-1.0), 'std_floor = -1'), (dict(floor=float('nan')), 'std_floor = nan'),
                     (dict(cams=None), 'non-null cams, depth_out, workspace'), (dict(depth=None), 'non-null cams, depth_out, workspace'),
                     (dict(ws=None), 'non-null cams, depth_out, workspace'), (dict(points=None), 'non-null points when n_points > 0'),
                     (dict(obs=None), 'n_obs = 0 when obs is null'), (dict(ws=C.c_void_p(base + 4096 * 12 + 8)), 'workspace aligned to 256 bytes'),
                     (dict(depth=C.c_void_p(base + 4096 * 4 + 2)), 'aligned to 4 bytes'), (dict(cams=C.c_void_p(base + 4)), 'aligned to 8 bytes'),
                     (dict(obs=C.c_void_p(base + 4096 * 2 + 4)), 'aligned to 8 bytes'), (dict(points=C.c_void_p(base + 4096 + 8)), 'points aligned to 16 bytes')):
        assert call(**kw) == 1, kw
        assert text in P.last_error(), (kw, P.last_error())


def test_png_encoding_and_report(tmp_path):
    enc = P.encode(np.array([[6.0, 9.0, 0.001, 10.009765625], [300.0, 0.0, 7.0, 2.5]]), np.array([[1, 0, 1, 1], [1, 0, 0, 1]], bool))
    assert enc.dtype == np.uint16
    np.testing.assert_array_equal(enc, [[1536, 0, 2, 2562], [65535, 0, 0, 640]])                  # no point is 0; half to even; clamp
    rows = np.array([[5, 4, 2, 1], [3, 1, 1, 0]])
    depth = np.array([[[1.0, 2.2, 0.0, 0.0]], [[3.0, 0.0, 0.0, 0.0]]], np.float32)
    gt = np.array([[[1.0, 2.0, 2.0, 4.0]], [[2.0, 2.0, 1.0, -1.0]]], np.float32)
    P.write_report(str(tmp_path / 'points.txt'), ['a.png', 'b.png'], rows, depth, gt)
    lines = (tmp_path / 'points.txt').read_text().splitlines()
    assert lines[0].split() == ['#', 'frame'] + list(P.ROW_NAMES) + ['coverage', 'absrel']
    a, b, tot = (l.split() for l in lines[1:])
    assert a[:5] == ['a.png', '5', '4', '2', '1'] and tot[:5] == ['total', '8', '5', '3', '1'] and float(a[5]) == 0.5 and float(tot[5]) == 0.375
    assert abs(float(a[6]) - 0.05) < 1e-6 and abs(float(b[6]) - 0.5) < 1e-6 and abs(float(tot[6]) - 0.2) < 1e-6
    P.write_report(str(tmp_path / 'n.txt'), ['a.png', 'b.png'], rows, depth)
    assert (tmp_path / 'n.txt').read_text().splitlines()[-1] == 'total 8 5 3 1 0.375000'
    assert P.totals_line(rows, 'track') == ('sparse-point depth prior (track): 2 frames, 8 observations, 5 projected, 3 pixels kept (1.5 per frame), '
                                            '1 hidden')
    assert P.totals_line(np.array([[5, 0, 0, 0]]), 'all').endswith('0 hidden -- 1 frames are left without a point')


# ------------------------------------------------------------------------------------------------ 6. both flag surfaces
def test_mip360_config_keys_parse_and_refusals(tmp_path):
    cfg = D.parse_gin(bindings=[])
    assert cfg['depth_points_vis'] == '' and cfg['depth_points_occl_radius'] == -1
    assert P.check_params('track', **P.scene_params(cfg)) == P.check_params() and P.check_params('all', **P.scene_params(cfg))['occl_radius'] == 4
    cfg = D.parse_gin(bindings=["Config.depth_points_vis = 'all'", 'Config.depth_points_near = 1.5', 'Config.depth_points_far = 50.0',
                                'Config.depth_points_occl_radius = 2', 'Config.depth_points_std_floor = 0.5', 'Config.depth_points_min_track = 2'])
    assert P.scene_params(cfg, 0.1) == dict(max_error=2.0, min_track=2, err_floor=0.5, near=0.15000000000000002, far=5.0, occl_radius=2, occl_tol=0.05,
                                           std_scale=1.0, std_floor=0.05)
    write_colmap_scene(str(tmp_path), F=10, H=8, W=10)
    base = ["Config.data_dir = '%s'" % tmp_path]
    prior = ["Config.depth_sup_type = 'points'", "Config.depth_points_vis = 'track'"]
    s = D.Scene(D.parse_gin(bindings=base + prior))                                             # no depths_points/ on disk
    assert s.depth_points_vis == 'track' and s.depth_points_target == 'prior' and not s.depths_sup.any() and s.depth_std_source is None
    assert s.depth_points_prm['near'] == 0.5 * s.scale and s.depth_points_prm['far'] == 200.0 * s.scale and s.depth_points_prm['occl_radius'] == 0
    a = D.Scene(D.parse_gin(bindings=base + ["Config.depth_sup_type = 'noisy'", "Config.depth_align_anchor = 'points'", "Config.depth_points_vis = 'all'"]))
    assert a.depth_points_target == 'anchor' and a.depths_anchor is None and a.depth_points_prm['occl_radius'] == 4 and (a.depths_sup > 0).any()
    plain = D.Scene(D.parse_gin(bindings=base + ["Config.depth_sup_type = 'noisy'"]))
    assert plain.depth_points_vis == '' and plain.depth_points_target is None
    with pytest.raises(ValueError, match='Depth folder .*depths_points does not exist'):          # without the flag the type is a folder like any other
        D.Scene(D.parse_gin(bindings=base + ["Config.depth_sup_type = 'points'"]))
    for extra, text in ((["Config.depth_sup_type = 'noisy'", "Config.depth_points_vis = 'track'"],
                         r"Config.depth_points_vis = 'track' computes .* Config.depth_sup_type = 'points' or .* Config.depth_align_anchor = 'points'"),
                        (["Config.depth_sup_type = 'noisy'", "Config.depth_align_anchor = 'lidar'", "Config.depth_points_vis = 'track'"], 'it needs one of them'),
                        (prior + ['Config.compute_disp_metrics = False'], "Config.depth_points_vis = 'track' .* Config.compute_disp_metrics = True"),
                        (["Config.depth_sup_type = 'points'", "Config.depth_points_vis = 'most'"], r"Config.depth_points_vis = 'most': expected '' \(off\), 'track' or 'all'"),
                        (prior + ['Config.depth_points_occl_radius = 9'], r'Config.depth_points_\*: occl_radius = 9'),
                        (prior + ['Config.depth_points_near = 300.0'], r'Config.depth_points_\*: near = ')):
        with pytest.raises(D.ConfigError, match=text):
            D.Scene(D.parse_gin(bindings=base + extra))
    # a gnll run without a folder or a constant takes its standard deviation from the points when they are the prior; a constant comes
    # first; as the anchor they give none, the alignment does
    g = D.Scene(D.parse_gin(bindings=base + prior + ["Config.depth_loss_type = 'gnll'"]))
    assert g.depth_std_source == 'points'
    g = D.Scene(D.parse_gin(bindings=base + prior + ["Config.depth_loss_type = 'gnll'", 'Config.depth_gnll_std = 0.1']))
    assert g.depth_std_source == 'constant'
    g = D.Scene(D.parse_gin(bindings=base + ["Config.depth_sup_type = 'noisy'", "Config.depth_align_anchor = 'points'", "Config.depth_points_vis = 'track'",
                                             "Config.depth_loss_type = 'gnll'"]))
    assert g.depth_std_source == 'alignment'


def test_nerfpp_flags_parse_and_refusals():
    pytest.importorskip('torch')
    from outdoor_nerf_depth_amd import ddp_train_nerf as T_
    base = ['--expname', 'x', '--synthetic']
    args = T_.config_parser().parse_args(base)
    assert args.depth_points_model == '' and args.depth_points_vis == 'track'
    assert P.check_params(args.depth_points_vis, **P.args_params(args)) == P.check_params()
    args = T_.config_parser().parse_args(base + ['--depth_points_model', 'm', '--depth_points_vis', 'all', '--depth_points_far', '80',
                                                 '--depth_points_std_floor', '0.5', '--depth_points_max_error', '1'])
    assert P.args_params(args, 0.1) == dict(max_error=1.0, min_track=3, err_floor=0.5, near=0.05, far=8.0, occl_radius=None, occl_tol=0.05,
                                           std_scale=1.0, std_floor=0.05)
    cli = P.make_parser().parse_args(['--data_dir', 'd', '--vis', 'all', '--occl_radius', '2', '--gin_bindings', 'Config.factor = 2'])
    assert cli.vis == 'all' and P.args_params(cli, 1.0, '')['occl_radius'] == 2 and cli.gin_bindings == ['Config.factor = 2']
    assert P.make_parser().parse_args(['--datadir', 'd', '--scene', 's', '--points_model', 'm']).vis == 'track'
    T_.validate_args(T_.config_parser().parse_args(base + ['--use_depth', '--depth_sup_type', 'points', '--depth_points_model', 'm']))
    T_.validate_args(T_.config_parser().parse_args(base + ['--use_depth', '--depth_sup_type', 'mono', '--depth_align_anchor', 'points',
                                                           '--depth_points_model', 'm']))
    for bad, text in ((['--depth_sup_type', 'points', '--depth_points_model', 'm'], '--depth_points_model .* needs --use_depth'),
                      (['--use_depth', '--depth_sup_type', 'gt', '--depth_points_model', 'm'],
                       '--depth_points_model .* --depth_sup_type points or .* --depth_align_anchor points'),
                      (['--use_depth', '--depth_sup_type', 'points', '--depth_points_model', 'm', '--depth_points_occl_radius', '9'],
                       r'--depth_points_\*: occl_radius = 9'),
                      (['--use_depth', '--depth_sup_type', 'points', '--depth_points_model', 'm', '--depth_points_near', '300'], r'--depth_points_\*: near = ')):
        with pytest.raises(SystemExit, match=text):
            T_.validate_args(T_.config_parser().parse_args(base + bad))
    with pytest.raises(SystemExit):
        T_.config_parser().parse_args(base + ['--depth_points_vis', 'most'])
    with pytest.raises(SystemExit, match='give either --data_dir'):
        P.main([])
    with pytest.raises(P.DepthPointsError, match='name the COLMAP model with --points_model'):
        P.main(['--datadir', 'd', '--scene', 's'])


def test_trainers_without_the_flags_import_neither_the_binding_nor_the_library():
    code = ("import sys; from outdoor_nerf_depth_amd import mip360_data, ddp_train_nerf; ddp_train_nerf.config_parser(); "
            "assert 'outdoor_nerf_depth_amd.depth_points_flags' in sys.modules; "
            "assert 'outdoor_nerf_depth_amd.depth_points' not in sys.modules; "
            "assert not [l for l in open('/proc/self/maps') if 'libdepthpoints_hip' in l]; print('clean')")
    out = subprocess.run([sys.executable, '-c', code], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and out.stdout.strip().endswith('clean'), out.stderr[-2000:]

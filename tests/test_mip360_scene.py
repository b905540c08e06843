"""CPU (no GPU): the MipNeRF-360 front end's host side -- COLMAP reader, pose conventions, transform_poses_pca against
upstream's own outputs (tests/golden/mip360_rays.npz), split indices, depth conventions, the gin-binding parser -- and the
argument checks of the new libmip360_hip.so entry points."""
import os
import struct

import numpy as np
import pytest

from outdoor_nerf_depth_amd import mip360_data as D

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'mip360_rays.npz')


def rotmat_to_qvec(R):
    """unit quaternion (w, x, y, z) of a rotation matrix (trace > 0 branch suffices for the small rotations used here)"""
    w = np.sqrt(1 + np.trace(R)) / 2
    return np.array([w, (R[2, 1] - R[1, 2]) / (4 * w), (R[0, 2] - R[2, 0]) / (4 * w), (R[1, 0] - R[0, 1]) / (4 * w)])


def small_rotation(rs):
    a = rs.randn(3)
    a = a / np.linalg.norm(a) * rs.uniform(0.05, 0.5)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    th = np.linalg.norm(a)
    Kn = K / th
    return np.eye(3) + np.sin(th) * Kn + (1 - np.cos(th)) * Kn @ Kn


def write_colmap(sparse, model, params, width, height, w2c, names, binary=True):
    """A COLMAP model with one camera and the given world-to-camera poses (R [3,3], t [3]), written from the format."""
    os.makedirs(sparse, exist_ok=True)
    mid = D.MODEL_IDS[model]
    if binary:
        with open(os.path.join(sparse, 'cameras.bin'), 'wb') as f:
            f.write(struct.pack('<Q', 1))
            f.write(struct.pack('<iiQQ', 1, mid, width, height))
            f.write(struct.pack('<%dd' % len(params), *params))
        with open(os.path.join(sparse, 'images.bin'), 'wb') as f:
            f.write(struct.pack('<Q', len(names)))
            for i, ((R, t), name) in enumerate(zip(w2c, names)):
                f.write(struct.pack('<idddddddi', i + 1, *rotmat_to_qvec(R), *t, 1))
                f.write(name.encode() + b'\x00')
                f.write(struct.pack('<Q', 2))
                f.write(struct.pack('<ddq', 1.0, 2.0, -1) * 2)
    else:
        with open(os.path.join(sparse, 'cameras.txt'), 'w') as f:
            f.write('# Camera list\n1 %s %d %d %s\n' % (model, width, height, ' '.join(repr(float(p)) for p in params)))
        with open(os.path.join(sparse, 'images.txt'), 'w') as f:
            f.write('# Image list\n')
            for i, ((R, t), name) in enumerate(zip(w2c, names)):
                f.write('%d %s %s 1 %s\n' % (i + 1, ' '.join(repr(float(v)) for v in rotmat_to_qvec(R)),
                                             ' '.join(repr(float(v)) for v in t), name))
                f.write('1.0 2.0 -1\n' if i % 2 else '\n')


def write_scene(root, n_frames=12, H=32, W=40, seed=0, sup_type='mono_crop', model='PINHOLE'):
    """A small COLMAP-format "DTU_format" scene: sparse/0 (binary), images/, depths_gt/, depths_{sup_type}/ (16-bit PNG,
    metres x 256, 0 = invalid).  Cameras on a line looking down +z at a tilted plane; names deliberately not in pose order."""
    from PIL import Image
    rs = np.random.RandomState(seed)
    names = ['frame_%03d.png' % i for i in range(n_frames)][::-1]
    w2c = []
    for i in range(n_frames):
        R = small_rotation(rs) if i % 3 else np.eye(3)
        c = np.array([0.3 * i, 0.05 * rs.randn(), 0.02 * i])
        w2c.append((R, -R @ c))
    f = 30.0
    params = {'PINHOLE': [f, f, W / 2, H / 2], 'SIMPLE_RADIAL': [f, W / 2, H / 2, -0.05]}[model]
    write_colmap(os.path.join(root, 'sparse', '0'), model, params, W, H, w2c, names)
    for d in ('images', 'depths_gt', 'depths_' + sup_type):
        os.makedirs(os.path.join(root, d), exist_ok=True)
    yy, xx = np.mgrid[0:H, 0:W]
    for i, name in enumerate(names):
        img = np.stack([(xx * 6 + 10 * i) % 256, (yy * 8) % 256, ((xx + yy) * 3) % 256], -1).astype(np.uint8)
        Image.fromarray(img).save(os.path.join(root, 'images', name))
        depth = 5.0 + 0.1 * yy + 0.05 * xx
        gt = np.round(depth * 256).astype(np.uint16)
        gt[rs.rand(H, W) < 0.3] = 0
        sup = gt.copy()
        sup[rs.rand(H, W) < 0.5] = 0
        Image.fromarray(gt).save(os.path.join(root, 'depths_gt', name))
        Image.fromarray(sup).save(os.path.join(root, 'depths_' + sup_type, name))
    return names, w2c, params


@pytest.mark.parametrize('binary', [True, False])
@pytest.mark.parametrize('model', ['SIMPLE_PINHOLE', 'PINHOLE', 'SIMPLE_RADIAL', 'RADIAL', 'OPENCV'])
def test_colmap_reader_and_pose_conventions(tmp_path, binary, model):
    rs = np.random.RandomState(3)
    params = {'SIMPLE_PINHOLE': [50., 20., 12.], 'PINHOLE': [50., 48., 20., 12.], 'SIMPLE_RADIAL': [50., 20., 12., -0.1],
              'RADIAL': [50., 20., 12., -0.1, 0.02], 'OPENCV': [50., 48., 20., 12., -0.1, 0.02, 0.001, -0.002]}[model]
    w2c = [(small_rotation(rs), rs.randn(3)) for _ in range(5)]
    names = ['c.png', 'a.png', 'e.png', 'b.png', 'd.png']
    write_colmap(str(tmp_path), model, params, 40, 24, w2c, names, binary)
    got_names, poses, pixtocam, dist = D.load_colmap_poses(str(tmp_path))
    assert got_names == sorted(names)
    order = np.argsort(names)
    for k, j in enumerate(order):
        R, t = w2c[j]
        c2w = np.linalg.inv(np.vstack([np.hstack([R, t[:, None]]), [0, 0, 0, 1]]))[:3]
        np.testing.assert_allclose(poses[k], c2w @ np.diag([1., -1., -1., 1.]), atol=1e-12)
    fx, fy, cx, cy = (params[0], params[0], params[1], params[2]) if model in ('SIMPLE_PINHOLE', 'SIMPLE_RADIAL', 'RADIAL') \
        else params[:4]
    np.testing.assert_allclose(pixtocam, [[1 / fx, 0, -cx / fx], [0, 1 / fy, -cy / fy], [0, 0, 1]], atol=1e-15)
    want = {'SIMPLE_PINHOLE': None, 'PINHOLE': None, 'SIMPLE_RADIAL': dict(k1=-0.1, k2=0., k3=0., p1=0., p2=0.),
            'RADIAL': dict(k1=-0.1, k2=0.02, k3=0., p1=0., p2=0.),
            'OPENCV': dict(k1=-0.1, k2=0.02, k3=0., p1=0.001, p2=-0.002)}[model]
    assert dist == want


def test_fisheye_is_rejected(tmp_path):
    write_colmap(str(tmp_path), 'OPENCV_FISHEYE', [50., 50., 20., 12., .1, .01, 0., 0.], 40, 24, [(np.eye(3), np.zeros(3))], ['a.png'])
    with pytest.raises(ValueError, match='OPENCV_FISHEYE'):
        D.load_colmap_poses(str(tmp_path))


def test_transform_poses_pca_matches_upstream():
    z = np.load(GOLDEN)
    flips = []
    for s in range(3):
        poses, tf = D.transform_poses_pca(z['pca%d_in' % s])
        np.testing.assert_allclose(poses, z['pca%d_poses' % s], rtol=1e-12, atol=1e-12)
        np.testing.assert_allclose(tf, z['pca%d_transform' % s], rtol=1e-12, atol=1e-12)
        # the y-flip branch is taken when the mean camera y axis has a negative z component after the alignment
        aligned, _ = D.pca_align(z['pca%d_in' % s])
        flips.append(bool(aligned.mean(0)[2, 1] < 0))
    assert flips == [True, False, False]                  # both branches of the flip are pinned by upstream's numbers


def test_split_indices():
    tr, te = D.split_indices(25, 1, 8)
    assert te.tolist() == [9, 19] and tr.tolist() == [i for i in range(25) if i not in (9, 19)]
    tr, te = D.split_indices(25, 4, 8)
    rest = [i for i in range(25) if i not in (9, 19)]
    assert te.tolist() == [9, 19] and tr.tolist() == rest[::4]
    tr, te = D.split_indices(20, 0, 8)
    assert te.tolist() == [0, 8, 16] and tr.tolist() == [i for i in range(20) if i % 8]


def test_depth_conventions():
    raw = np.array([[0, 1, 2, 256], [512, 2560, 25600, 65535]], np.float32)
    d = D.convert_depth(raw)
    np.testing.assert_array_equal(d, np.where(raw < 2, -1., raw / 256.).astype(np.float32))
    c = D.convert_depth(raw, crop_range=50.)
    assert c[1, 1] == 10. and c[1, 2] == -256. and c[1, 3] == -256. and c[0, 0] == -1.
    sup = np.where(np.random.RandomState(7).rand(3, 20, 30) < 0.5, 4.0, -1.0).astype(np.float32)
    kept = D.keep_ratio_mask(sup, 0.1)
    assert ((kept > 0) <= (sup > 0)).all()
    assert abs(np.mean(kept > 0) - 0.1) < 0.03
    with pytest.raises(ValueError):
        D.keep_ratio_mask(sup, 0.9)


def test_scene_loader(tmp_path):
    pytest.importorskip('PIL')
    names, w2c, params = write_scene(str(tmp_path), n_frames=12)
    cfg = D.parse_gin(bindings=["Config.data_dir = '%s'" % tmp_path, "Config.depth_sup_type = 'mono_crop'",
                                'Config.depth_crop_range = 6.0'])
    sc = D.Scene(cfg)
    assert sc.names == sorted(names) and sc.images.shape == (12, 32, 40, 3) and sc.images.dtype == np.uint8
    assert sc.test.tolist() == [9] and sc.train.tolist() == [i for i in range(12) if i != 9]
    np.testing.assert_allclose(sc.scale, np.sqrt((sc.transform[:3, :3] @ sc.transform[:3, :3].T)[0, 0]))
    assert sc.near == pytest.approx(0.2 * sc.scale) and sc.far == pytest.approx(1e6 * sc.scale)
    from PIL import Image
    raw = np.asarray(Image.open(os.path.join(str(tmp_path), 'depths_mono_crop', sc.names[3])), np.float32)
    want = D.convert_depth(raw, 6.0) * sc.scale
    np.testing.assert_allclose(sc.depths_sup[3], want.astype(np.float32), rtol=1e-6)
    assert (sc.depths_sup[3][raw / 256. > 6.0] < 0).all()
    t = sc.camera_table('test')
    assert t.shape == (1, 28) and t[0, 27] == 0
    np.testing.assert_allclose(t[0, 9:21].reshape(3, 4), sc.poses[9], rtol=1e-6, atol=1e-6)


def test_scene_loads_depths_without_disp_metrics(tmp_path):
    pytest.importorskip('PIL')
    write_scene(str(tmp_path), n_frames=12)
    base = ["Config.data_dir = '%s'" % tmp_path, "Config.depth_sup_type = 'mono_crop'"]
    on = D.Scene(D.parse_gin(bindings=base))
    off = D.Scene(D.parse_gin(bindings=base + ['Config.compute_disp_metrics = False']))
    np.testing.assert_array_equal(off.depths_gt, on.depths_gt)        # the depth metrics score rgb-only runs as well
    np.testing.assert_array_equal(off.depths_sup, on.depths_sup)
    assert ((off.depths_gt > 0).mean() > 0.5)


def test_empty_split_and_bad_step_counts_are_errors(tmp_path):
    pytest.importorskip('PIL')
    write_scene(str(tmp_path), n_frames=6)                             # sample_every 1: test frames 9, 19, ... -> none
    sc = D.Scene(D.parse_gin(bindings=["Config.data_dir = '%s'" % tmp_path, "Config.depth_sup_type = 'mono_crop'"]))
    with pytest.raises(ValueError, match='test split of 6 frames is empty'):
        sc.camera_table('test')
    from outdoor_nerf_depth_amd import mip360_train as T
    with pytest.raises(D.ConfigError, match='max_steps'):
        T.make_trainer(D.parse_gin(bindings=['Config.max_steps = 1']), 'cpu')


TRAIN_KITTI = ['Config.max_steps = 75000', 'Config.sample_every = 1', "Config.data_dir = '/data/kitti/DTU_format'",
               'Config.compute_disp_metrics = True', "Config.depth_loss_type = 'mse'",
               "Config.checkpoint_dir = '/data/kitti/DTU_format/logs/checkpoints-1-7.5w-mse'"]


def test_gin_comments_outside_quotes_only(tmp_path):
    gin = tmp_path / 'c.gin'
    gin.write_text("Config.data_dir = '/data/run#2'  # a comment\nConfig.eval_suffix = \"a#b\" # another\n# whole line\n")
    cfg = D.parse_gin([str(gin)], ["Config.checkpoint_dir = '/ckpt/#3' # trailing"])
    assert cfg['data_dir'] == '/data/run#2' and cfg['eval_suffix'] == 'a#b' and cfg['checkpoint_dir'] == '/ckpt/#3'
    assert D.strip_comment("x = 'it\\'s # in' # out") == "x = 'it\\'s # in' "


def test_gin_bindings(tmp_path):
    cfg = D.parse_gin(bindings=TRAIN_KITTI)
    assert cfg['max_steps'] == 75000 and cfg['data_dir'] == '/data/kitti/DTU_format' and cfg['compute_disp_metrics'] is True
    assert cfg['batch_size'] == 4096 and cfg['near'] == 0.2 and cfg['far'] == 1e6 and cfg['auto_adjust_near_far'] is True
    gin = tmp_path / 'x.gin'
    gin.write_text("Config.dataset_loader = 'llff'\nConfig.near = 0.2  # comment\n\nModel.raydist_fn = @jnp.reciprocal\n"
                   'NerfMLP.net_width = 1024\nPropMLP.disable_rgb = True\n')
    cfg = D.parse_gin([str(gin)], ['Config.lambda_depth = 10', "Config.eval_suffix = 'left'"])
    assert cfg['lambda_depth'] == 10 and cfg['eval_suffix'] == 'left'
    with pytest.raises(D.ConfigError, match='NerfMLP.net_width'):
        D.parse_gin(bindings=['NerfMLP.net_width = 512'])
    with pytest.raises(D.ConfigError, match='Model.num_levels'):
        D.parse_gin(bindings=['Model.num_levels = 2'])
    with pytest.raises(D.ConfigError, match='Config.no_such_key'):
        D.parse_gin(bindings=['Config.no_such_key = 1'])


def test_new_entry_points_validate_arguments_without_a_gpu():
    from outdoor_nerf_depth_amd import mip360 as M
    lib = M.lib()
    assert lib.mip360_abi_version() == M.ABI_VERSION == 9
    assert lib.mip360_frame_rays(None, None, 1, 0, 40, 0, 16, 0.2, 1e6, None, None, None, None, None, None) == 1
    assert b'non-null' in lib.mip360_last_error()
    dummy = 16
    assert lib.mip360_frame_rays(None, dummy, 1, 1, 40, 0, 16, 0.2, 1e6, dummy, dummy, dummy, dummy, dummy, dummy) == 1
    assert b'cam < n_frames' in lib.mip360_last_error()
    assert lib.mip360_sample_batch(None, None, 2, 8, 8, 0, 0, 64, None, None, None, 0.2, 1e6, 3, *([None] * 11)) == 1
    assert b'non-null' in lib.mip360_last_error()
    assert lib.mip360_distance_percentiles(None, 4, 64, dummy, dummy, dummy, dummy) == 1
    assert b'S <= 62' in lib.mip360_last_error()
    assert lib.mip360_distance_percentiles(None, 4, 32, None, None, None, None) == 1
    assert b'non-null' in lib.mip360_last_error()

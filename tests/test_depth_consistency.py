"""No GPU: the multi-view consistency check of depth priors -- the reference on the analytic scene, the host side of
outdoor_nerf_depth_amd/depth_consistency.py (neighbours, argument checks, PNG encoding), both flag surfaces and the precedence of
the sources of the prior's standard deviation.  The analytic scene and the writers of both on-disk layouts live here and are
shared with tests/test_gpu_depth_consistency.py.

The analytic scene: f = 30, principal point at the frame centre; camera i at (0.3 i, 0.05 randn, 0.02 i), identity rotation when
i % 3 == 0, else an axis-angle of 0.01 .. 0.06 rad (RandomState(0)); the world is the plane z = 6 + 0.1 x + 0.05 y and, when asked, a
box face at z = 3, |x - 0.8| < 0.5, |y| < 0.4 in front of it (occlusion edges); depth by analytic ray intersection at pixel centres,
stored float32; neighbours: the 4 nearest.  The conditions asserted on the reference's output are conditions on these inputs (a
scene on which the check has something to decide), not tolerances of the kernel.
"""
import os

import numpy as np
import pytest

from outdoor_nerf_depth_amd import depth_consistency as DC
from outdoor_nerf_depth_amd import mip360_data as D
from tests import depth_consistency_reference as R

SHAPES = [(6, 24, 32), (5, 33, 47), (8, 48, 64)]      # one tile not full; odd sizes with partial tiles; several workgroups per frame
FOCAL = 30.0


def axis_angle(axis, angle):
    a = np.asarray(axis, np.float64)
    a = a / np.linalg.norm(a)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * (K @ K)


def analytic_cameras(F, H, W):
    """(K [3, 3], c2w [F, 3, 4]) of the analytic scene, OpenCV axes"""
    rs = np.random.RandomState(0)
    c2w = np.zeros((F, 3, 4))
    for i in range(F):
        c2w[i, :, 3] = (0.3 * i, 0.05 * rs.randn(), 0.02 * i)
        c2w[i, :, :3] = np.eye(3) if i % 3 == 0 else axis_angle(rs.randn(3), rs.uniform(0.01, 0.06))
    return np.array([[FOCAL, 0, W / 2.0], [0, FOCAL, H / 2.0], [0, 0, 1.0]]), c2w


def analytic_depth(K, c2w, H, W, box=False):
    """float32 [F, H, W]: z-depth of the plane (and the box face in front of it) at the pixel centres"""
    yy, xx = np.mgrid[0:H, 0:W]
    dc = np.stack([(xx + 0.5 - K[0, 2]) / K[0, 0], (yy + 0.5 - K[1, 2]) / K[1, 1], np.ones((H, W))], -1)
    n = np.array([-0.1, -0.05, 1.0])                                             # the plane: n . p = 6
    out = []
    for pose in c2w:
        dw, c = dc @ pose[:, :3].T, pose[:, 3]
        t = (6.0 - n @ c) / (dw @ n)
        if box:
            tb = (3.0 - c[2]) / dw[..., 2]
            p = c + tb[..., None] * dw
            hit = (tb > 0) & (np.abs(p[..., 0] - 0.8) < 0.5) & (np.abs(p[..., 1]) < 0.4) & (tb < t)
            t = np.where(hit, tb, t)
        out.append(t)
    return np.stack(out, 0).astype(np.float32)


_scenes = {}


def analytic_scene(shape, box=False):
    """{'cams' [F, 16], 'nbr' [F, 4], 'depth' float32 [F, H, W], 'K', 'c2w'} of one shape, built once and shared (read-only)"""
    key = (tuple(shape), box)
    if key not in _scenes:
        F, H, W = shape
        K, c2w = analytic_cameras(F, H, W)
        depth = analytic_depth(K, c2w, H, W, box)
        depth.setflags(write=False)
        _scenes[key] = dict(K=K, c2w=c2w, cams=DC.pack_cams(K, c2w), nbr=DC.neighbours(c2w[:, :, 3], 4), depth=depth)
    return _scenes[key]


def corrupted(depth, share=0.1, factor=1.2, seed=1):
    """(depth with `share` of its pixels multiplied by `factor`, the mask of those pixels)"""
    mask = np.random.RandomState(seed).rand(*depth.shape) < share
    return np.where(mask, depth * np.float32(factor), depth).astype(np.float32), mask


def sparse(depth, share=0.05, seed=2):
    return np.where(np.random.RandomState(seed).rand(*depth.shape) < share, depth, np.float32(0)).astype(np.float32)


def with_invalids(depth, seed=3):
    """a tenth of the pixels each 0, negative and NaN"""
    u = np.random.RandomState(seed).rand(*depth.shape)
    out = depth.copy()
    out[u < 0.1] = 0.0
    out[(u >= 0.1) & (u < 0.2)] = -1.5
    out[(u >= 0.2) & (u < 0.3)] = np.nan
    return out


def prior_of(kind, shape):
    if kind == 'exact':
        return analytic_scene(shape, box=True)['depth']
    base = analytic_scene(shape)['depth']
    return {'corrupted': lambda: corrupted(base)[0], 'sparse': lambda: sparse(base), 'invalids': lambda: with_invalids(base)}[kind]()


_refs = {}


def reference(kind, shape):
    """The reference's outputs for prior_of(kind, shape) with the defaults, computed once and shared (read-only)"""
    if (kind, shape) not in _refs:
        s = analytic_scene(shape)
        _refs[kind, shape] = R.check(prior_of(kind, shape), s['cams'], s['nbr'])
    return _refs[kind, shape]


# ---------------------------------------------------------------------------------------------------- on-disk scenes
def write_colmap_scene(root, F=12, H=32, W=40, sup_type='noisy', share=0.15, factor=1.5, box=False):
    """The analytic scene as a COLMAP-format scene: sparse/0, images/, depths_gt/ (exact) and depths_{sup_type}/ (`share` of the pixels
    multiplied by `factor`), 16-bit PNG of metres x 256.  Returns (names, corrupted mask [F, H, W] in file order)."""
    from PIL import Image
    from tests.test_mip360_scene import write_colmap
    K, c2w = analytic_cameras(F, H, W)
    depth = analytic_depth(K, c2w, H, W, box)
    bad, mask = corrupted(depth, share, factor, seed=5)
    names = ['frame_%03d.png' % i for i in range(F)]
    w2c = [(p[:, :3].T, -p[:, :3].T @ p[:, 3]) for p in c2w]
    write_colmap(os.path.join(root, 'sparse', '0'), 'PINHOLE', [FOCAL, FOCAL, W / 2.0, H / 2.0], W, H, w2c, names)
    for d in ('images', 'depths_gt', 'depths_' + sup_type):
        os.makedirs(os.path.join(root, d), exist_ok=True)
    yy, xx = np.mgrid[0:H, 0:W]
    for i, name in enumerate(names):
        world_x = (c2w[i, 0, 3] + (xx + 0.5 - W / 2.0) / FOCAL * depth[i])                     # a texture fixed in the world
        img = np.stack([(world_x * 40) % 256, (yy * 8) % 256, (depth[i] * 30) % 256], -1).astype(np.uint8)
        Image.fromarray(img).save(os.path.join(root, 'images', name))
        Image.fromarray(np.round(depth[i] * 256.0).astype(np.uint16)).save(os.path.join(root, 'depths_gt', name))
        Image.fromarray(np.round(bad[i] * 256.0).astype(np.uint16)).save(os.path.join(root, 'depths_' + sup_type, name))
    return names, mask


def write_nerfpp_scene(root, scene='scene', F=6, H=24, W=32, sup_type='noisy', scale=0.05, share=0.15, factor=1.5):
    """The analytic scene in the NeRF++ layout: even frames are train/, odd ones test/; camera centres and depths in scene units
    (metres x scale), PNGs in metres x 256.  Returns the scale."""
    from PIL import Image
    K, c2w = analytic_cameras(F, H, W)
    depth = analytic_depth(K, c2w, H, W)
    bad, _ = corrupted(depth, share, factor, seed=5)
    base = os.path.join(root, scene)
    os.makedirs(base, exist_ok=True)
    with open(os.path.join(base, 'scale'), 'w') as f:
        f.write('%r\n' % scale)
    K4 = np.eye(4)
    K4[:3, :3] = K
    for split, frames in (('train', range(0, F, 2)), ('test', range(1, F, 2))):
        for d in ('rgb', 'pose', 'intrinsics', 'depth', 'depth_' + sup_type):
            os.makedirs(os.path.join(base, split, d), exist_ok=True)
        for i in frames:
            name = '%06d' % i
            pose = np.eye(4)
            pose[:3] = c2w[i]
            pose[:3, 3] *= scale
            for d, m in (('pose', pose), ('intrinsics', K4)):
                with open(os.path.join(base, split, d, name + '.txt'), 'w') as f:
                    f.write(' '.join(repr(float(v)) for v in m.reshape(-1)))
            img = np.stack([(depth[i] * 30) % 256, (depth[i] * 7) % 256, (depth[i] * 3) % 256], -1).astype(np.uint8)
            Image.fromarray(img).save(os.path.join(base, split, 'rgb', name + '.png'))
            Image.fromarray(np.round(depth[i] * 256.0).astype(np.uint16)).save(os.path.join(base, split, 'depth', name + '.png'))
            Image.fromarray(np.round(bad[i] * 256.0).astype(np.uint16)).save(os.path.join(base, split, 'depth_' + sup_type, name + '.png'))
    return scale


# -------------------------------------------------------------------------------------------- 1. the reference on the scene
@pytest.mark.parametrize('shape', SHAPES)
def test_reference_keeps_exact_priors_and_drops_corrupted_ones(shape):
    s = analytic_scene(shape)
    plain = R.check(s['depth'], s['cams'], s['nbr'])
    n_valid, n_ver, n_kept, _ = plain['rows'].sum(0)
    ver = plain['counts'][..., 0] >= 2
    print('%s: verifiable %.1f %%; exact, no box: %.2f %% of the verifiable kept' % (shape, 100.0 * n_ver / n_valid, 100.0 * plain['keep'][ver].mean()))
    assert n_valid == np.prod(shape) and n_ver > 0.5 * n_valid

    box = reference('exact', shape)
    ver = box['counts'][..., 0] >= 2
    kept_box = box['keep'][ver].mean()
    print('%s: exact, with the box: %.2f %% of the verifiable kept' % (shape, 100.0 * kept_box))
    assert kept_box >= 0.97

    bad, mask = corrupted(s['depth'])
    got = reference('corrupted', shape)
    ver = got['counts'][..., 0] >= 2
    dropped_bad, kept_clean = 1.0 - got['keep'][ver & mask].mean(), got['keep'][ver & ~mask].mean()
    print('%s: 10 %% x 1.2: %.2f %% of the corrupted verifiable dropped, %.2f %% of the clean verifiable kept'
          % (shape, 100.0 * dropped_bad, 100.0 * kept_clean))
    assert dropped_bad >= 0.93 and kept_clean >= 0.94
    # the outputs hang together
    valid = bad > 0
    np.testing.assert_array_equal(got['depth_out'], np.where(got['keep'], bad, np.float32(0)))
    assert ((got['std_out'] > 0) == got['keep']).all() and valid.all()
    np.testing.assert_array_equal(got['rows'][:, 2], got['keep'].reshape(shape[0], -1).sum(1))
    np.testing.assert_array_equal(got['rows'][:, 3], got['rows'][:, 0] - got['rows'][:, 2])


def test_reference_vectorised_and_scalar_forms_agree():
    shape = SHAPES[0]
    s = analytic_scene(shape)
    prior = with_invalids(corrupted(analytic_scene(shape, box=True)['depth'])[0])
    got = R.check(prior, s['cams'], s['nbr'], std_floor=0.003)
    rs = np.random.RandomState(9)
    for _ in range(200):
        i, y, x = rs.randint(shape[0]), rs.randint(shape[1]), rs.randint(shape[2])
        d, sd, n_seen, n_ok = R.check_pixel(prior, s['cams'], s['nbr'], i, y, x, std_floor=0.003)
        assert np.array_equal(np.float32(d).view(np.int32), got['depth_out'][i, y, x].view(np.int32)), (i, y, x)
        assert sd == got['std_out'][i, y, x] and (n_seen, n_ok) == tuple(got['counts'][i, y, x]), (i, y, x)


def test_reference_invalid_pixels_pass_through_and_unverified_follow_the_switch():
    shape = SHAPES[0]
    s = analytic_scene(shape)
    prior = prior_of('invalids', shape)
    got = reference('invalids', shape)
    invalid = ~(prior > 0)
    np.testing.assert_array_equal(got['depth_out'][invalid].view(np.int32), prior[invalid].view(np.int32))
    assert (got['std_out'][invalid] == 0).all() and (got['counts'][invalid] == 0).all()
    assert got['rows'][:, 0].sum() == (~invalid).sum()
    for keep_unverified in (True, False):
        none = R.check(prior, s['cams'], s['nbr'], min_views=5, keep_unverified=keep_unverified)      # 4 neighbours: nothing verifiable
        assert none['rows'][:, 1].sum() == 0 and none['keep'][~invalid].all() == keep_unverified
        assert (none['rows'][:, 2].sum() == (~invalid).sum()) == keep_unverified
    floor = R.check(prior, s['cams'], s['nbr'], std_floor=0.5)
    assert (floor['std_out'][floor['keep']] >= 0.5).all() and (floor['std_out'][~floor['keep']] == 0).all()


# ------------------------------------------------------------------------------------------------------- 2. neighbours
def test_neighbours_order_ties_and_padding():
    c = np.array([[0, 0, 0], [1, 0, 0], [-1, 0, 0], [2, 0, 0], [0, 3, 0.]])
    np.testing.assert_array_equal(DC.neighbours(c, 3), [[1, 2, 3], [0, 3, 2], [0, 1, 3], [1, 0, 2], [0, 1, 2]])   # ties: lower index
    got = DC.neighbours(c, 6)
    assert got.dtype == np.int32 and got.shape == (5, 6) and (got[:, 4:] == -1).all() and (got[:, :4] >= 0).all()
    np.testing.assert_array_equal(DC.neighbours(np.zeros((1, 3)), 2), [[-1, -1]])
    assert DC.neighbours(c, 0).shape == (5, 0)
    np.testing.assert_array_equal(DC.neighbours(np.zeros((3, 3)), 2), [[1, 2], [0, 2], [0, 1]])                  # all tied
    with pytest.raises(DC.DepthConsError, match='0 .. 16'):
        DC.neighbours(c, 17)
    with pytest.raises(DC.DepthConsError, match=r'centres: expected \[F, 3\]'):
        DC.neighbours(np.zeros((3, 2)), 1)


# ------------------------------------------------------------------------------------------ 3. argument errors, no device
def test_host_checks_name_the_argument():
    s = analytic_scene(SHAPES[0])
    cams, nbr = s['cams'], s['nbr']
    DC.validate(cams, nbr)
    for col, text in ((0, 'cams: frame 2 has focal lengths'), (5, None)):
        bad = cams.copy()
        bad[2, col] = -1.0 if col == 0 else bad[2, col] + 1e-3
        with pytest.raises(DC.DepthConsError, match=text or r'cams: the rotation of frame 2 is not orthonormal'):
            DC.validate(bad, nbr)
    bad = cams.copy()
    bad[1, 9] = np.nan
    with pytest.raises(DC.DepthConsError, match='cams: frame 1 has a value that is not finite'):
        DC.validate(bad, nbr)
    with pytest.raises(DC.DepthConsError, match=r'cams: expected float64 \[F, 16\]'):
        DC.validate(cams[:, :15], nbr)
    for row, text in (([0, 1, 2, 3], 'nbr: frame 0 lists itself'), ([1, 2, 1, -1], 'nbr: frame 0 lists a neighbour twice'),
                      ([1, 6, -1, -1], 'nbr: frame 0 lists frame 6, but there are 6 frames')):
        bad = nbr.copy()
        bad[0] = row
        with pytest.raises(DC.DepthConsError, match=text):
            DC.validate(cams, bad)
    with pytest.raises(DC.DepthConsError, match=r'nbr: expected \[6, K\]'):
        DC.validate(cams, nbr[:5])
    with pytest.raises(DC.DepthConsError, match='nbr: expected an integer array'):
        DC.validate(cams, nbr.astype(np.float32))
    with pytest.raises(DC.DepthConsError, match='nbr: 17 neighbours per frame, at most 16'):
        DC.validate(cams, np.full((6, 17), -1))
    K = s['K'].copy()
    K[0, 1] = 0.25
    with pytest.raises(DC.DepthConsError, match='frame 0 has skew 0.25'):
        DC.pack_cams(K, s['c2w'])
    for kw, text in ((dict(min_views=0), 'min_views = 0'), (dict(pix_tol=-1), 'pix_tol = -1.0'), (dict(rel_tol=float('nan')), 'rel_tol = nan'),
                     (dict(std_floor=float('inf')), 'std_floor = inf')):
        with pytest.raises(DC.DepthConsError, match=text):
            DC.check_params(**kw)


def test_tensor_checks_name_the_tensor():
    torch = pytest.importorskip('torch')
    s = analytic_scene(SHAPES[0])
    with pytest.raises(DC.DepthConsError, match='depth: expected a CUDA/HIP float32 tensor'):
        DC.check_async(torch.zeros(6, 24, 32), s['cams'], s['nbr'])
    with pytest.raises(DC.DepthConsError, match='depth: expected a CUDA/HIP float32 tensor'):
        DC.check_async(np.zeros((6, 24, 32), np.float32), s['cams'], s['nbr'])
    # dtype, shape, contiguity and aliasing are answered before the device is asked for
    prior = torch.zeros(6, 24, 32)
    for bad, text in ((prior.double(), r'depth: expected torch.float32, got torch.float64'), (prior[0], r'depth: expected \[F, H, W\]'),
                      (prior[:, :, ::2], 'depth: expected a contiguous tensor')):
        with pytest.raises(DC.DepthConsError, match=text):
            DC.check_async(bad, s['cams'], s['nbr'])
    for out, text in ((prior, 'depth_out overlaps depth'), (prior[1:], r'depth_out \(5, 24, 32\)'), (prior.int(), 'depth_out: expected torch.float32'),
                      (torch.zeros(6, 24, 64)[:, :, ::2], 'depth_out: expected a contiguous tensor')):
        with pytest.raises(DC.DepthConsError, match=text):
            DC.check_async(prior, s['cams'], s['nbr'], depth_out=out)
    with pytest.raises(DC.DepthConsError, match='depth_out overlaps depth'):
        DC.check_async(prior[1:], s['cams'][1:], np.full((5, 1), -1), depth_out=prior[:5])
    with pytest.raises(DC.DepthConsError, match=r'views = 17: expected 0 \(off\) .. 16'):
        DC.filter_priors(prior, s['cams'], 17)


def test_scene_with_distortion_is_refused_by_name(tmp_path):
    from tests.test_mip360_scene import write_scene
    write_scene(str(tmp_path), n_frames=10, H=8, W=10, model='SIMPLE_RADIAL')
    scene = D.Scene(D.parse_gin(bindings=["Config.data_dir = '%s'" % tmp_path, "Config.depth_sup_type = 'mono_crop'"]))
    with pytest.raises(D.ConfigError, match='pinhole-only .* the scene\'s camera is SIMPLE_RADIAL'):
        DC.cams_from_scene(scene)
    write_colmap_scene(str(tmp_path / 'pinhole'), F=10, H=8, W=10)
    scene = D.Scene(D.parse_gin(bindings=["Config.data_dir = '%s'" % (tmp_path / 'pinhole'), "Config.depth_sup_type = 'noisy'"]))
    cams = DC.cams_from_scene(scene, scene.train)
    DC.validate(cams, DC.neighbours(cams[:, [7, 11, 15]], 4))
    np.testing.assert_allclose(cams[:, :4], [[FOCAL, FOCAL, 5.0, 4.0]] * len(scene.train), rtol=1e-6)


def test_scene_adapter_reprojects_the_scene_onto_itself(tmp_path):
    """The adapter's cameras and the Scene's depths (scene units) describe one geometry: the reference keeps the exact depths_gt"""
    write_colmap_scene(str(tmp_path), F=10, H=24, W=32)
    scene = D.Scene(D.parse_gin(bindings=["Config.data_dir = '%s'" % tmp_path, "Config.depth_sup_type = 'noisy'"]))
    cams = DC.cams_from_scene(scene)
    got = R.check(scene.depths_gt, cams, DC.neighbours(cams[:, [7, 11, 15]], 4))
    ver = got['counts'][..., 0] >= 2
    print('scene units: %.1f %% verifiable, %.2f %% of them kept' % (100.0 * ver.mean(), 100.0 * got['keep'][ver].mean()))
    assert ver.mean() > 0.8 and got['keep'][ver].mean() >= 0.97


def test_sampler_adapter_reads_intrinsics_and_poses(tmp_path):
    from outdoor_nerf_depth_amd.data_loader_split import load_data_split
    scale = write_nerfpp_scene(str(tmp_path))
    samplers = load_data_split(str(tmp_path), 'scene', 'train', depth_sup_type='noisy')
    cams = DC.cams_from_samplers(samplers)
    K, c2w = analytic_cameras(6, 24, 32)
    np.testing.assert_allclose(cams[:, :4], [[FOCAL, FOCAL, 16.0, 12.0]] * 3)
    np.testing.assert_allclose(cams[:, 4:].reshape(3, 3, 4)[:, :, 3], c2w[0::2, :, 3] * scale, rtol=1e-6, atol=1e-8)
    DC.validate(cams, DC.neighbours(cams[:, [7, 11, 15]], 2))
    gt = np.stack([s.depth_gt.reshape(24, 32) for s in samplers], 0)
    got = R.check(gt, cams, DC.neighbours(cams[:, [7, 11, 15]], 2), min_views=1)
    ver = got['counts'][..., 0] >= 1
    assert ver.mean() > 0.5 and got['keep'][ver].mean() >= 0.97
    samplers[0].intrinsics = samplers[0].intrinsics.copy()
    samplers[0].intrinsics[0, 1] = 0.5
    with pytest.raises(DC.DepthConsError, match='ray samplers: frame 0 has skew 0.5'):
        DC.cams_from_samplers(samplers)


# --------------------------------------------------------------------------------------------------- 4. the library, no GPU
def test_workspace_bytes_limits():
    assert DC.workspace_bytes(1, 1, 1) == 256
    assert DC.workspace_bytes(295, 375, 1242) == (295 * 39 * 47 * 16 + 255) // 256 * 256
    assert DC.workspace_bytes(65535, 8, 32) > 0 and DC.workspace_bytes(1, 1 << 14, 1 << 14) > 0
    for args, text in (((0, 4, 4), 'n_frames = 0, expected 1 .. 65535'), ((65536, 4, 4), 'n_frames = 65536'),
                       ((1, 0, 4), 'a frame has at least one pixel'), ((1, 4, -1), 'a frame has at least one pixel'),
                       ((1, (1 << 14) + 1, 1 << 14), 'exceeds 2\\^28 pixels per frame')):
        with pytest.raises(DC.DepthConsError, match=text):
            DC.workspace_bytes(*args)


def test_binding_declares_the_headers_symbols_and_constants():
    import re
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, 'include', 'depthcons_hip.h')).read()
    declared = set(re.findall(r'^(?:const char\*|int64_t|int) (depthcons_\w+)\(', header, re.M))
    assert declared == set(DC.SYMBOLS) and len(declared) == 4
    const = dict((k, v) for k, v in re.findall(r'#define DEPTHCONS_(\w+) \(?(\d+)', header))
    assert (int(const['ABI_VERSION']), int(const['MAX_FRAMES']), int(const['MAX_VIEWS']), int(const['CAM']), int(const['ROW'])) == \
        (DC.ABI_VERSION, DC.MAX_FRAMES, DC.MAX_VIEWS, DC.CAM, len(DC.ROW_NAMES))
    assert len(DC.SYMBOLS['depthcons_check'][1]) == header.split('int depthcons_check(')[1].split(');')[0].count(',') + 1


def test_library_argument_checks_need_no_gpu():
    import ctypes as C
    lib = DC.lib()
    assert lib.depthcons_abi_version() == DC.ABI_VERSION
    buf = (C.c_double * 1024)()                                                  # host memory: every call below fails before any launch
    p = C.c_void_p(C.addressof(buf))
    q = C.c_void_p(C.addressof(buf) + 4096)

    def call(F=1, H=2, W=2, K=1, depth=p, cams=p, nbr=p, pix=1.0, rel=0.01, mv=2, ku=1, floor=0.0, ws=None, out=q, std=None, cnt=None, rows=None):
        return lib.depthcons_check(None, F, H, W, K, depth, cams, nbr, pix, rel, mv, ku, floor, ws, out, std, cnt, rows)
    for kw, text in ((dict(F=0), 'n_frames = 0'), (dict(K=17), 'n_views = 17, expected 0 .. 16'), (dict(K=-1), 'n_views = -1'),
                     (dict(pix=-1.0), 'pix_tol = -1'), (dict(rel=float('nan')), 'rel_tol = nan'), (dict(floor=float('inf')), 'std_floor = inf'),
                     (dict(mv=0), 'min_views = 0'), (dict(ku=2), 'keep_unverified = 2'), (dict(depth=None), 'non-null depth, cams, depth_out'),
                     (dict(nbr=None), 'non-null nbr when n_views > 0'), (dict(rows=q), 'non-null workspace when rows is given'),
                     (dict(out=p), 'depth_out overlaps depth'), (dict(std=C.c_void_p(C.addressof(buf) + 8)), 'std_out overlaps depth'),
                     (dict(cnt=C.c_void_p(C.addressof(buf) + 12)), 'counts overlaps depth'),
                     (dict(out=C.c_void_p(C.addressof(buf) + 4097)), 'aligned to 4 bytes')):
        assert call(**kw) == 1, kw
        assert text in DC.last_error(), (kw, DC.last_error())


# ----------------------------------------------------------------------------------------------------- 5. PNG encoding
def test_png_encoding_round_trip(tmp_path):
    from PIL import Image
    raw = np.array([[0, 1, 2, 1536], [65535, 300, 7, 40000]], np.uint16)
    dropped = np.array([[0, 0, 1, 0], [1, 0, 0, 0]], bool)
    enc = DC.encode_prior(raw, dropped)
    assert enc.dtype == np.uint16
    np.testing.assert_array_equal(enc, [[0, 1, 0, 1536], [0, 300, 7, 40000]])
    std_m = np.array([[0.0, 0.001, 0.5, 1.0 / 256 * 2.5], [300.0, 0.01, 0.0117, 3.0]])
    kept = np.array([[1, 1, 1, 1], [1, 0, 1, 1]], bool)
    s16 = DC.encode_std(std_m, kept)
    np.testing.assert_array_equal(s16, [[2, 2, 128, 2], [65535, 0, 3, 768]])                   # round half to even; clamp; 0 where not kept
    for name, a in (('p.png', enc), ('s.png', s16)):
        DC._write_png16(str(tmp_path / name), a)
        back = np.asarray(Image.open(str(tmp_path / name)))
        assert back.dtype == np.uint16 or back.dtype == np.int32
        np.testing.assert_array_equal(back, a)
    # what the loaders make of it: a kept pixel's standard deviation is valid (> 0), everything else is not
    assert ((D.convert_depth(s16) > 0) == kept).all()
    assert ((D.convert_depth(enc) > 0) == (~dropped & (raw >= 2))).all()


def test_report_totals(tmp_path):
    rows = np.array([[10, 8, 7, 3], [12, 12, 12, 0]])
    prior = np.array([[[1.0, 2.2, 0.0]], [[4.0, 4.0, 3.0]]], np.float32)
    gt = np.array([[[1.0, 2.0, 5.0]], [[4.0, 0.0, 2.0]]], np.float32)
    valid = prior > 0
    kept = np.array([[[1, 0, 0]], [[1, 1, 0]]], bool)
    DC.write_report(str(tmp_path / 'r.txt'), ['a.png', 'b.png'], rows, prior, gt, valid, kept)
    lines = (tmp_path / 'r.txt').read_text().splitlines()
    assert lines[0].split() == ['#', 'frame', 'n_valid', 'n_verifiable', 'n_kept', 'n_dropped', 'absrel_kept', 'absrel_dropped']
    assert lines[1].split()[:5] == ['a.png', '10', '8', '7', '3'] and lines[-1].split()[:5] == ['total', '22', '20', '19', '3']
    assert float(lines[1].split()[5]) == 0.0 and abs(float(lines[1].split()[6]) - 0.1) < 1e-6
    assert abs(float(lines[-1].split()[6]) - 0.3) < 1e-6                                       # (0.1 + 0.5) / 2
    DC.write_report(str(tmp_path / 'n.txt'), ['a.png', 'b.png'], rows)
    assert (tmp_path / 'n.txt').read_text().splitlines()[-1] == 'total 22 20 19 3'


# ------------------------------------------------------------------------------------------------- 6. both flag surfaces
def test_mip360_config_keys_parse():
    cfg = D.parse_gin(bindings=[])
    assert (cfg['depth_cons_views'], cfg['depth_cons_min_views'], cfg['depth_cons_pix_tol'], cfg['depth_cons_rel_tol'],
            cfg['depth_cons_keep_unverified'], cfg['depth_cons_std_floor']) == (0, 2, 1.0, 0.01, True, 0.0)
    cfg = D.parse_gin(bindings=['Config.depth_cons_views = 4', 'Config.depth_cons_min_views = 3', 'Config.depth_cons_pix_tol = 1.5',
                                'Config.depth_cons_rel_tol = 0.02', 'Config.depth_cons_keep_unverified = False',
                                'Config.depth_cons_std_floor = 0.05'])
    assert DC.scene_params(cfg, 0.5) == dict(min_views=3, pix_tol=1.5, rel_tol=0.02, keep_unverified=False, std_floor=0.025)
    assert DC.scene_params(D.parse_gin(bindings=[]), 2.0) == dict(R.DEFAULTS)


def test_nerfpp_flags_parse():
    pytest.importorskip('torch')
    from outdoor_nerf_depth_amd import ddp_train_nerf as T_
    base = ['--expname', 'x', '--synthetic']
    args = T_.config_parser().parse_args(base)
    assert args.depth_cons_views == 0 and DC.args_params(args, 3.0) == dict(R.DEFAULTS)
    args = T_.config_parser().parse_args(base + ['--depth_cons_views', '4', '--depth_cons_min_views', '3', '--depth_cons_pix_tol', '2',
                                                 '--depth_cons_rel_tol', '0.05', '--depth_cons_keep_unverified', '0',
                                                 '--depth_cons_std_floor', '0.1'])
    assert args.depth_cons_views == 4
    assert DC.args_params(args, 0.5) == dict(min_views=3, pix_tol=2.0, rel_tol=0.05, keep_unverified=False, std_floor=0.05)
    cli = DC.make_parser().parse_args(['--data_dir', 'd', '--depth_sup_type', 'lidar', '--std_floor', '0.02', '--views', '6',
                                       '--gin_bindings', 'Config.factor = 2'])
    assert cli.views == 6 and DC.args_params(cli, 1.0, '')['std_floor'] == 0.02 and cli.gin_bindings == ['Config.factor = 2']
    with pytest.raises(DC.DepthConsError, match=r'0 \(off\) .. 16'):
        DC.check_views(17, '--depth_cons_views')
    T_.validate_args(T_.config_parser().parse_args(base + ['--use_depth', '--depth_cons_views', '16']))
    for bad, text in ((['--use_depth', '--depth_cons_views', '17'], r'--depth_cons_views = 17: expected 0 \(off\) .. 16'),
                      (['--use_depth', '--depth_cons_views', '-1'], '--depth_cons_views = -1'), (['--depth_cons_views', '4'], 'it needs --use_depth')):
        with pytest.raises(SystemExit, match=text):
            T_.validate_args(T_.config_parser().parse_args(base + bad))


# --------------------------------------------------------------------------- 7. where the standard deviation comes from
def _gnll_scene(root, extra):
    return D.Scene(D.parse_gin(bindings=["Config.data_dir = '%s'" % root, "Config.depth_sup_type = 'noisy'",
                                         "Config.depth_loss_type = 'gnll'"] + extra))


def test_std_precedence_folder_then_constant_then_the_check(tmp_path):
    import shutil
    write_colmap_scene(str(tmp_path), F=10, H=8, W=10)
    views = ['Config.depth_cons_views = 4']
    s = _gnll_scene(tmp_path, views)
    assert s.depth_std_source == 'consistency' and s.depths_std is None and s.depth_std_const is None and s.depth_cons_views == 4
    s = _gnll_scene(tmp_path, views + ['Config.depth_gnll_std = 0.25'])
    assert s.depth_std_source == 'constant' and s.depth_std_const == float(np.float32(s.scale * 0.25))
    shutil.copytree(str(tmp_path / 'depths_noisy'), str(tmp_path / 'depths_noisy_std'))
    s = _gnll_scene(tmp_path, views + ['Config.depth_gnll_std = 0.25'])
    assert s.depth_std_source == 'folder' and s.depths_std is not None and s.depth_std_const is None
    s = D.Scene(D.parse_gin(bindings=["Config.data_dir = '%s'" % tmp_path, "Config.depth_sup_type = 'noisy'"] + views))
    assert s.depth_std_source is None and s.depth_cons_views == 4                              # 'mse' reads no standard deviation
    with pytest.raises(D.ConfigError, match=r'Config.depth_cons_views = 17: expected 0 \(off\) .. 16'):
        _gnll_scene(tmp_path, ['Config.depth_cons_views = 17'])


def test_missing_std_errors_are_unchanged_with_the_flag_off(tmp_path):
    from outdoor_nerf_depth_amd.data_loader_split import load_data_split
    write_colmap_scene(str(tmp_path / 'c'), F=10, H=8, W=10)
    std_dir = os.path.join(str(tmp_path / 'c'), 'depths_noisy_std')
    with pytest.raises(ValueError) as e:
        _gnll_scene(tmp_path / 'c', [])
    assert str(e.value) == ('the gnll depth loss needs the standard deviation of the prior: Depth folder %s does not exist and '
                            'Config.depth_gnll_std = 0.0 (write the maps there, encoded like the prior, or bind a constant in metres)' % std_dir)
    write_nerfpp_scene(str(tmp_path / 'n'))
    std_dir = '%s/scene/train/depth_noisy_std' % (tmp_path / 'n')
    with pytest.raises(ValueError) as e:
        load_data_split(str(tmp_path / 'n'), 'scene', 'train', depth_sup_type='noisy', depth_std=0.0)
    assert str(e.value) == ('the gnll depth loss needs the standard deviation of the prior: no maps in %s and --depth_gnll_std = 0 '
                            '(write the maps there, uint16 / 256 like the prior, or pass a constant in metres)' % std_dir)
    samplers = load_data_split(str(tmp_path / 'n'), 'scene', 'train', depth_sup_type='noisy', depth_std=0.0, depth_std_optional=True)
    assert all(s.depth_std is None and s.depth_sup is not None for s in samplers)
    samplers = load_data_split(str(tmp_path / 'n'), 'scene', 'train', depth_sup_type='noisy', depth_std=0.5, depth_std_optional=True)
    assert all(s.depth_std is not None for s in samplers)                                      # the constant comes before the check

"""No GPU: the plane-sweep multi-view stereo depth prior -- the reference on the textured box scene and on hand-built
cases, the host side of outdoor_nerf_depth_amd/depth_mvs.py (parameter, table, tensor and camera checks, PNG encoding, mvs.txt),
the library's argument checks and both flag surfaces.  The textured scene and the hand-built cases live here and are shared with
tests/test_gpu_depth_mvs.py.

The scene: the analytic box scene and cameras of tests/test_depth_consistency.py; every pixel's world point is quantised to a 0.25 m
lattice and hashed to a grey level, a texture fixed in the world; planes uniform in inverse depth from 12 m to 2 m.  The conditions
asserted on the reference's output are conditions on these inputs (a scene on which the sweep has something to find), not tolerances
of the kernel.
"""
import os

import numpy as np
import pytest

from outdoor_nerf_depth_amd import depth_consistency as DC
from outdoor_nerf_depth_amd import depth_mvs as M
from outdoor_nerf_depth_amd import mip360_data as D
from tests import depth_mvs_reference as R
from tests.test_depth_consistency import SHAPES as _SHAPES, analytic_cameras, analytic_depth

SHAPES = tuple(_SHAPES)
assert SHAPES == ((6, 24, 32), (5, 33, 47), (8, 48, 64))
PLANES = {SHAPES[0]: 12, SHAPES[1]: 12, SHAPES[2]: 16}
NEAR, FAR, LATTICE = 2.0, 12.0, 0.25


def world_points(K, c2w, depth):
    """float64 [F, H, W, 3]: the world point of every pixel centre at its z-depth"""
    F, H, W = depth.shape
    yy, xx = np.mgrid[0:H, 0:W]
    dc = np.stack([(xx + 0.5 - K[0, 2]) / K[0, 0], (yy + 0.5 - K[1, 2]) / K[1, 1], np.ones((H, W))], -1)
    return np.stack([c2w[i, :, 3] + depth[i].astype(np.float64)[..., None] * (dc @ c2w[i, :, :3].T) for i in range(F)], 0)


def textured_images(K, c2w, depth, lattice=LATTICE):
    """uint8 [F, H, W, 3]: a texture fixed in the world -- the world point of every pixel quantised to `lattice` metres and hashed to
    a grey level"""
    q = np.floor(world_points(K, c2w, depth) / lattice).astype(np.int64)
    h = (q[..., 0] * 73856093) ^ (q[..., 1] * 19349663) ^ (q[..., 2] * 83492791)
    h = (h ^ (h >> 13)) * 1274126177
    grey = ((h >> 16) & 255).astype(np.uint8)
    return np.ascontiguousarray(np.repeat(grey[..., None], 3, -1))


_scenes = {}


def scene(shape):
    """{'rgb' uint8 [F, H, W, 3], 'cams' [F, 16], 'depth' float32 [F, H, W] (true), 'inv_depth' [D], 'K', 'c2w'} of one shape, built
    once and shared (read-only)"""
    shape = tuple(shape)
    if shape not in _scenes:
        F, H, W = shape
        K, c2w = analytic_cameras(F, H, W)
        depth = analytic_depth(K, c2w, H, W, box=True)
        rgb = textured_images(K, c2w, depth)
        for a in (depth, rgb):
            a.setflags(write=False)
        _scenes[shape] = dict(K=K, c2w=c2w, cams=DC.pack_cams(K, c2w), depth=depth, rgb=rgb,
                              inv_depth=M.planes_table(NEAR, FAR, PLANES[shape]))
    return _scenes[shape]


def nbr_of(shape, views):
    return DC.neighbours(scene(shape)['c2w'][:, :, 3], views)


_refs = {}


def reference(shape, views=4, best_views=None, agg_radius=2, **kw):
    """The reference's outputs for scene(shape), computed once and shared (read-only)"""
    key = (tuple(shape), views, best_views, agg_radius, tuple(sorted(kw.items())))
    if key not in _refs:
        s = scene(shape)
        table = kw.pop('inv_depth', None)
        _refs[key] = R.sweep(s['rgb'], s['cams'], nbr_of(shape, views), s['inv_depth'] if table is None else np.asarray(table),
                             best_views, agg_radius, **kw)
    return _refs[key]


def within_two_steps(ref, s):
    """bool over the accepted pixels: the inverse of the depth lies within two plane steps of the true inverse depth"""
    acc = ref['status'] == R.ACCEPTED
    step = s['inv_depth'][1] - s['inv_depth'][0]
    return np.abs(1.0 / ref['depth'][acc].astype(np.float64) - 1.0 / s['depth'][acc].astype(np.float64)) <= 2 * step


# ------------------------------------------------------------------------------------------------ hand-built cases
def _texture(H, W, seed=0):
    grey = np.random.RandomState(seed).randint(0, 256, (H, W)).astype(np.uint8)
    return np.repeat(grey[..., None], 3, -1)


def _eye_cams(F, focal, H, W, shifts):
    c2w = np.tile(np.eye(4)[:3], (F, 1, 1))
    for i, t in enumerate(shifts):
        c2w[i, :, 3] = t
    return DC.pack_cams([[focal, 0, W / 2.0], [0, focal, H / 2.0], [0, 0, 1.0]], c2w)


TABLE8 = np.arange(1, 9, dtype=np.float64) / 16.0             # planes at 16 / k m: disparities of 1 .. 8 pixels at f = 32, 0.5 m apart
# the planes of the sideways shift, as disparities of 0, 1, 4, 9, 10 and 11 pixels: plane 2 is exactly 4 m, and under a texture of
# period 8 its two neighbours (3 pixels less, 5 pixels more) see the same pixels, so the parabola's offset is exactly 0
TABLE_SHIFT = np.array([0, 1, 4, 9, 10, 11], np.float64) / 16.0


def hand_case(name):
    """(rgb, cams, nbr, inv_depth, params) of a hand-built case"""
    H, W = 20, 40
    if name == 'identical':                                   # two cameras at one place see one image: every plane matches alike
        img = _texture(H, W)
        return np.stack([img, img], 0), _eye_cams(2, 32.0, H, W, [(0, 0, 0), (0, 0, 0)]), np.array([[1], [0]]), TABLE8, {}
    if name == 'lone':                                        # one frame, no neighbour
        return _texture(H, W)[None], _eye_cams(1, 32.0, H, W, [(0, 0, 0)]), np.array([[-1, -1]]), TABLE8, {}
    if name == 'no_neighbours':                               # frame 1 lists nobody
        img = _texture(H, W)
        return np.stack([img, img], 0), _eye_cams(2, 32.0, H, W, [(0, 0, 0), (0.5, 0, 0)]), np.array([[1], [-1]]), TABLE8, {}
    if name == 'behind':                                      # the source camera looks the other way: nothing is in front of it
        img = _texture(H, W)
        cams = _eye_cams(2, 32.0, H, W, [(0, 0, 0), (0.5, 0, 0)])
        cams[1, 4:] = np.array([[-1.0, 0, 0, 0.5], [0, 1.0, 0, 0], [0, 0, -1.0, 0]]).reshape(-1)      # a half turn about y
        return np.stack([img, img], 0), cams, np.array([[1], [-1]]), TABLE8, {}
    if name == 'shift':                                       # a fronto-parallel plane at 4 m = plane 2; 0.5 m sideways is 4 pixels there
        wide = np.tile(_texture(H, 8, seed=1), (1, 6, 1))[:, :W + 4]
        return (np.stack([wide[:, 4:], wide[:, :W]], 0), _eye_cams(2, 32.0, H, W, [(0, 0, 0), (-0.5, 0, 0)]), np.array([[1], [0]]), TABLE_SHIFT,
                dict(agg_radius=1))
    if name == 'tie':                                         # flat images: every plane costs 0 and the lowest wins
        flat = np.full((2, H, W, 3), 90, np.uint8)
        return flat, _eye_cams(2, 32.0, H, W, [(0, 0, 0), (0.5, 0, 0)]), np.array([[1], [0]]), TABLE8, {}
    raise KeyError(name)


HAND_CASES = ('identical', 'lone', 'no_neighbours', 'behind', 'shift', 'tie')


def check_hand_case(name, out):
    """what the definition says of a hand-built case, of the reference's outputs or the device's"""
    status, plane = out['status'], out['plane']
    if name == 'identical':
        assert (status == R.END).all() and (plane == 0).all() and (out['cost'] == 0).all()
    elif name == 'lone':
        assert (status == R.UNSEEN).all() and out['rows'].tolist() == [[0, 0, 0, status[0].size]]
    elif name == 'no_neighbours':
        assert (status[1] == R.UNSEEN).all() and (status[0] != R.UNSEEN).any()
    elif name == 'behind':
        assert (status[0] == R.UNSEEN).all() and (out['cost'][0] == 24 * 25).all() and (plane[0] == 0).all()
    elif name == 'shift':
        # the interior: every census tap of pixel x + 9 of frame 1 and of the window around it lies inside the frame
        inner = (slice(0, 1), slice(3, -3), slice(3, 28))
        assert (status[inner] == R.ACCEPTED).all() and (plane[inner] == 2).all() and (out['cost'][inner] == 0).all()
        assert (out['second'][inner] > 0).all()
        assert (out['depth'][inner] == 4.0).all()              # off = 0: exactly the plane
        if 'off' in out:
            assert not out['off'][inner].any()
        np.testing.assert_array_equal(out['std'][inner], np.float32(0.5 * 4.0 * 4.0 * 5.0 / 16.0))    # the step to the next plane
    elif name == 'tie':
        inner = (slice(None), slice(None), slice(10, -10))      # every plane's pixel and window lie inside the other frame
        assert (plane == 0).all() and (status[inner] == R.END).all() and (out['second'][inner] == 0).all()
        assert ((status == R.END) | (status == R.UNSEEN)).all()
    assert (out['rows'].sum(1) == status[0].size).all()
    assert not out['depth'][status != R.ACCEPTED].any() and not out['std'][status != R.ACCEPTED].any()


# ------------------------------------------------------------------------------------------------ 1. the reference
@pytest.mark.parametrize('shape', SHAPES)
def test_reference_finds_the_scene_at_the_defaults(shape):
    """At the defaults (4 views, best_views 2, agg_radius 2, uniqueness 0.9) at least 60 % of the pixels are accepted and at least
    95 % of those lie within two plane steps of the true inverse depth.  Measured with this reference (UNSEEN rule, edge-replicated
    aggregation) on the CPU, against the true depth of the analytic scene: 82.5 / 88.5 / 87.8 % accepted and 98.1 / 99.2 / 99.6 % of
    those within two steps, for the three shapes in order."""
    s, ref = scene(shape), reference(shape)
    acc = ref['status'] == R.ACCEPTED
    good = within_two_steps(ref, s)
    print('%s: accepted %.1f %%, within two steps %.1f %%, rows %s' % (shape, 100 * acc.mean(), 100 * good.mean(), ref['rows'].sum(0)))
    assert acc.mean() >= 0.60 and good.mean() >= 0.95
    assert (ref['rows'].sum(1) == shape[1] * shape[2]).all()
    assert (ref['std'][acc] > 0).all() and not ref['depth'][~acc].any()


def test_reference_vectorised_and_scalar_forms_agree():
    rs = np.random.RandomState(4)
    for shape, views, best, radius in ((SHAPES[0], 4, None, 2), (SHAPES[1], 2, 2, 1), (SHAPES[0], 1, 1, 0)):
        s, ref = scene(shape), reference(shape, views, best, radius)
        cen = R.census(s['rgb'])
        F, H, W = shape
        picks = [(0, 0, 0), (F - 1, H - 1, W - 1), (1, 0, W - 1)] + [(rs.randint(F), rs.randint(H), rs.randint(W)) for _ in range(9)]
        for i, y, x in picks:
            z, sd, status, k, c, sec = R.sweep_pixel(s['rgb'], s['cams'], nbr_of(shape, views), s['inv_depth'], i, y, x, best, radius, cen=cen)
            got = tuple(ref[n][i, y, x] for n in ('depth', 'std', 'status', 'plane', 'cost', 'second'))
            assert (z.view(np.int32), sd.view(np.int32), status, k, c, sec) == (got[0].view(np.int32), got[1].view(np.int32)) + got[2:], (i, y, x)


@pytest.mark.parametrize('name', HAND_CASES)
def test_reference_hand_built_cases(name):
    rgb, cams, nbr, table, prm = hand_case(name)
    check_hand_case(name, R.sweep(rgb, cams, nbr, table, **prm))


def test_every_parametrised_case_has_accepted_and_rejected_pixels():
    """The cases of the GPU test's parametrisation.  Measured with this reference: the weakest, 1 view at agg_radius 1 on the largest
    shape, accepts 16.4 % (4032 of 24576 pixels); the strongest, 4 views, best_views 2, agg_radius 4 on the largest shape, 89.5 %."""
    for shape in SHAPES:
        for views in (1, 2, 4):
            for best in sorted(set((1, (views + 1) // 2, views))):
                for radius in (0, 1, 4):
                    rows = reference(shape, views, best, radius)['rows'].sum(0)
                    assert rows[0] > 0 and rows[1:].sum() > 0, (shape, views, best, radius, rows)


def test_census_bits_and_luma():
    rgb = np.zeros((1, 5, 5, 3), np.uint8)
    rgb[0, 2, 2] = (10, 20, 30)
    assert R.luma(rgb)[0, 2, 2] == (770 + 3000 + 870 + 128) >> 8
    cen = R.census(rgb)
    assert cen[0, 2, 2] == (1 << 24) - 1 and cen[0, 0, 0] == 0        # every tap is below the centre; nothing is below 0
    assert cen[0, 2, 1] == 0 and cen[0, 0, 4] == 0
    rgb[0, 0, 0] = 255                                                 # the corner's own replicated taps are not below it
    assert R.census(rgb)[0, 0, 0] == sum(1 << t for t, (dy, dx) in enumerate((a, b) for a in range(-2, 3) for b in range(-2, 3) if (a, b) != (0, 0))
                                          if (max(dy, 0), max(dx, 0)) != (0, 0))


# ------------------------------------------------------------------------------------------------ 2. the host side
def test_parameter_and_table_checks_name_the_argument():
    p = M.check_params()
    assert p == dict(views=4, planes=64, near=2.0, far=100.0, best_views=2, agg_radius=2, uniqueness=0.9, std_planes=0.5, std_floor=0.0)
    assert M.check_params(views=5)['best_views'] == 3 and M.check_params(views=16, best_views=16, far=float('inf'))['far'] == float('inf')
    assert {k: v[0] for k, v in M.PARAMS.items() if k in R.DEFAULTS and k != 'best_views'} == {k: v for k, v in R.DEFAULTS.items() if k != 'best_views'}
    assert [R.best_default(v) for v in range(1, 6)] == [M.check_params(views=v)['best_views'] for v in range(1, 6)]
    for kw, text in ((dict(views=0), r'views = 0: expected an integer 1 .. 16'), (dict(views=17), 'views = 17'),
                     (dict(planes=3), r'planes = 3: expected an integer 4 .. 256'), (dict(planes=257), 'planes = 257'), (dict(planes=8.5), 'planes = 8.5'),
                     (dict(best_views=5), r'best_views = 5: expected an integer 1 .. 4'), (dict(best_views=-1), 'best_views = -1'),
                     (dict(agg_radius=5), r'agg_radius = 5: expected an integer 0 .. 4'), (dict(agg_radius=-1), 'agg_radius = -1'),
                     (dict(uniqueness=0.0), r'uniqueness = 0.0: expected a number in \(0, 1\]'), (dict(uniqueness=1.5), 'uniqueness = 1.5'),
                     (dict(uniqueness=float('nan')), 'uniqueness = nan'), (dict(std_planes=0.0), 'std_planes = 0.0: expected a finite number > 0'),
                     (dict(std_planes=float('inf')), 'std_planes = inf'), (dict(near=0.0), 'near = 0.0: expected a finite depth > 0'),
                     (dict(near=float('inf')), 'near = inf'), (dict(far=1.0), 'far = 1.0: expected a depth above near = 2.0'),
                     (dict(far=float('nan')), 'far = nan'), (dict(std_floor=-1.0), 'std_floor = -1.0')):
        with pytest.raises(M.DepthMvsError, match=text):
            M.check_params(**kw)
    t = M.planes_table(2.0, 12.0, 12)
    assert t.shape == (12,) and t[0] == 1.0 / 12.0 and t[-1] == 0.5 and (np.diff(t) > 0).all()
    assert M.planes_table(2.0, float('inf'), 4).tolist() == [0.0, 0.5 / 3, 0.5 * (2 / 3), 0.5]
    assert M.check_table(list(t)).dtype == np.float64
    for bad, text in ((t[:3], r'inv_depth: 3 planes, expected 4 .. 256'), (np.linspace(0, 1, 257), 'inv_depth: 257 planes'),
                      (-t[::-1], 'inv_depth: every entry must be finite and >= 0'), (np.where(np.arange(12) == 5, np.nan, t), 'must be finite'),
                      (np.where(np.arange(12) == 11, np.inf, t), 'must be finite'), (t[::-1], r'strictly increasing \(entry 1 '),
                      (np.where(np.arange(12) == 5, t[4], t), r'strictly increasing \(entry 5 ')):
        with pytest.raises(M.DepthMvsError, match=text):
            M.check_table(bad)


def test_tensor_and_camera_checks_name_the_argument_before_the_device_is_asked():
    torch = pytest.importorskip('torch')
    rgb = torch.zeros(2, 6, 8, 3, dtype=torch.uint8)
    cams, nbr = _eye_cams(2, 10.0, 6, 8, [(0, 0, 0), (1, 0, 0)]), np.array([[1], [0]])
    for bad in (np.zeros((2, 6, 8, 3), np.uint8), rgb):                                         # no tensor; a host tensor, asked last
        with pytest.raises(M.DepthMvsError, match='rgb: expected a CUDA/HIP uint8 tensor .* no CPU path'):
            M.sweep_async(bad, cams, nbr)
    for t, text in ((rgb.float(), 'rgb: expected torch.uint8, got torch.float32'), (rgb[0], r'rgb: expected \[F, H, W, 3\] \(frames of one size\)'),
                    (rgb[..., :2], r'rgb: expected \[F, H, W, 3\]'), (torch.zeros(2, 6, 16, 3, dtype=torch.uint8)[:, :, ::2], 'rgb: expected a contiguous tensor')):
        with pytest.raises(M.DepthMvsError, match=text):
            M.sweep_async(t, cams, nbr)
    with pytest.raises(M.DepthMvsError, match='cams: 2 cameras for 1 frames of rgb'):
        M.sweep_async(rgb[:1], cams, nbr)
    with pytest.raises(M.DepthMvsError, match='neighbours per frame = 0: expected an integer 1 .. 16'):
        M.sweep_async(rgb, cams, np.zeros((2, 0), np.int32))
    with pytest.raises(M.DepthMvsError, match='neighbours per frame = 17'):
        M.sweep_async(rgb, cams, np.full((2, 17), -1))
    for kw, text in ((dict(planes=2), 'planes = 2'), (dict(inv_depth=[0.1, 0.2, 0.3]), 'inv_depth: 3 planes'), (dict(best_views=2), 'best_views = 2'),
                     (dict(agg_radius=9), 'agg_radius = 9'), (dict(near=5.0, far=4.0), 'far = 4.0')):
        with pytest.raises(M.DepthMvsError, match=text):
            M.sweep_async(rgb, cams, nbr, **kw)
    skew = cams.copy()
    skew[1, 4] = 2.0
    for c, n, text in ((skew, nbr, 'cams: the rotation of frame 1 is not orthonormal'), (cams, np.array([[0], [0]]), 'nbr: frame 0 lists itself'),
                       (cams, np.array([[5], [0]]), 'nbr: frame 0 lists frame 5'), (cams[:, :15], nbr, r'cams: expected float64 \[F, 16\]')):
        with pytest.raises(DC.DepthConsError, match=text):
            M.sweep_async(rgb, c, n)
    with pytest.raises(DC.DepthConsError, match='has skew'):
        DC.pack_cams([[10.0, 0.5, 4], [0, 10.0, 3], [0, 0, 1]], np.tile(np.eye(4)[:3], (2, 1, 1)))


def test_scene_with_distortion_is_refused_by_name(tmp_path):
    from tests.test_mip360_scene import write_scene
    write_scene(str(tmp_path), n_frames=10, H=8, W=10, model='SIMPLE_RADIAL')
    s = D.Scene(D.parse_gin(bindings=["Config.data_dir = '%s'" % tmp_path, "Config.depth_sup_type = 'mvs'", 'Config.depth_mvs_views = 2']))
    with pytest.raises(D.ConfigError, match='pinhole-only .* the scene\'s camera is SIMPLE_RADIAL'):
        DC.cams_from_scene(s, s.train)                         # what device_frames and the CLI call first


# ------------------------------------------------------------------------------------------------ 3. the library, no GPU
def test_workspace_bytes_limits():
    assert M.workspace_bytes(1, 1, 1) == 256 + 256                                # one census word, one tile's partials
    n, tiles = 295 * 375 * 1242, 24 * 39
    assert M.workspace_bytes(295, 375, 1242) == (4 * n + 255) // 256 * 256 + (295 * tiles * 16 + 255) // 256 * 256     # nothing per plane
    assert M.workspace_bytes(65535, 8, 32) > 0 and M.workspace_bytes(1, 1 << 14, 1 << 14) > 0
    for args, text in (((0, 4, 4), 'n_frames = 0, expected 1 .. 65535'), ((65536, 4, 4), 'n_frames = 65536'),
                       ((1, 0, 4), 'a frame has at least one pixel'), ((1, 4, -1), 'a frame has at least one pixel'),
                       ((1, (1 << 14) + 1, 1 << 14), 'exceeds 2\\^28 pixels per frame')):
        with pytest.raises(M.DepthMvsError, match=text):
            M.workspace_bytes(*args)


def test_binding_declares_the_headers_symbols_and_constants():
    import re
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, 'include', 'depthmvs_hip.h')).read()
    declared = set(re.findall(r'^(?:const char\*|int64_t|int) (depthmvs_\w+)\(', header, re.M))
    assert declared == set(M.SYMBOLS) and len(declared) == 4
    const = dict((k, v) for k, v in re.findall(r'#define DEPTHMVS_(\w+) \(?(\d+)', header))
    assert tuple(int(const[k]) for k in ('ABI_VERSION', 'MAX_FRAMES', 'MAX_VIEWS', 'MIN_PLANES', 'MAX_PLANES', 'MAX_RADIUS', 'CAM', 'CENSUS_BITS', 'ROW')) == \
        (M.ABI_VERSION, M.MAX_FRAMES, M.MAX_VIEWS, M.MIN_PLANES, M.MAX_PLANES, M.MAX_RADIUS, DC.CAM, R.OUT, len(M.ROW_NAMES))
    assert M.MAX_VIEWS == DC.MAX_VIEWS
    assert [int(const[k]) for k in ('ACCEPTED', 'END', 'AMBIGUOUS', 'UNSEEN')] == [M.ACCEPTED, M.END, M.AMBIGUOUS, M.UNSEEN] \
        == [R.ACCEPTED, R.END, R.AMBIGUOUS, R.UNSEEN]
    assert [int(const['N_' + k.upper()[2:]]) for k in M.ROW_NAMES] == [0, 1, 2, 3]
    assert len(M.SYMBOLS['depthmvs_sweep'][1]) == header.split('int depthmvs_sweep(')[1].split(');')[0].count(',') + 1


def test_library_argument_checks_need_no_gpu():
    import ctypes as C
    lib = M.lib()
    assert lib.depthmvs_abi_version() == M.ABI_VERSION
    buf = (C.c_double * 16384)()                                                 # host memory: every call below fails before any launch
    base = (C.addressof(buf) + 255) // 256 * 256
    at = lambda k: C.c_void_p(base + 4096 * k)

    def call(F=1, H=2, W=2, V=2, Dn=8, rgb=at(0), cams=at(1), nbr=at(2), inv=at(3), best=1, radius=2, uniq=0.9, stdp=0.5, ws=at(12),
             depth=at(4), std=at(5), status=at(6), plane=None, cost=None, second=None, census=None, rows=None):
        return lib.depthmvs_sweep(None, F, H, W, V, Dn, rgb, cams, nbr, inv, best, radius, uniq, stdp, ws, depth, std, status, plane, cost,
                                  second, census, rows)
    for kw, text in ((dict(F=0), 'n_frames = 0'), (dict(F=65536), 'n_frames = 65536'), (dict(H=0), 'at least one pixel'),
                     (dict(V=0), 'n_views = 0, expected 1 .. 16'), (dict(V=17), 'n_views = 17'), (dict(Dn=3), 'n_planes = 3, expected 4 .. 256'),
                     (dict(Dn=257), 'n_planes = 257'), (dict(best=0), 'best_views = 0, expected 1 .. n_views = 2'), (dict(best=3), 'best_views = 3'),
                     (dict(radius=-1), 'agg_radius = -1, expected 0 .. 4'), (dict(radius=5), 'agg_radius = 5'), (dict(uniq=0.0), 'uniqueness = 0'),
                     (dict(uniq=1.5), 'uniqueness = 1.5'), (dict(uniq=float('nan')), 'uniqueness = nan'), (dict(stdp=0.0), 'std_planes = 0'),
                     (dict(stdp=float('inf')), 'std_planes = inf'), (dict(rgb=None), 'non-null rgb, cams, nbr, inv_depth, workspace'),
                     (dict(inv=None), 'non-null rgb, cams, nbr, inv_depth, workspace'), (dict(status=None), 'non-null depth, std, status'),
                     (dict(depth=at(0)), 'depth overlaps rgb'), (dict(std=at(1)), 'std overlaps cams'), (dict(status=at(2)), 'status overlaps nbr'),
                     (dict(plane=at(3)), 'plane overlaps inv_depth'), (dict(cost=at(0)), 'cost overlaps rgb'), (dict(second=at(1)), 'second overlaps cams'),
                     (dict(census=at(0)), 'census overlaps rgb'), (dict(rows=at(0)), 'rows overlaps rgb'), (dict(ws=at(0)), 'workspace overlaps rgb'),
                     (dict(plane=at(4)), 'depth overlaps plane'), (dict(cost=at(6)), 'status overlaps cost'), (dict(depth=at(12)), 'depth overlaps workspace'),
                     (dict(ws=C.c_void_p(base + 4096 * 12 + 8)), 'workspace aligned to 256 bytes'),
                     (dict(depth=C.c_void_p(base + 4096 * 4 + 2)), 'aligned to 4 bytes'), (dict(cost=C.c_void_p(base + 4096 * 7 + 1)), 'aligned to 2 bytes'),
                     (dict(cams=C.c_void_p(base + 4096 + 4)), 'aligned to 8 bytes')):
        assert call(**kw) == 1, kw
        assert text in M.last_error(), (kw, M.last_error())


# ------------------------------------------------------------------------------------------------ 4. PNG encoding and the report
def test_png_encoding_round_trip(tmp_path):
    from PIL import Image
    metres = np.array([[6.0, 9.0, 0.001, 10.009765625], [300.0, 0.0, 7.0, 2.5]])
    acc = np.array([[1, 0, 1, 1], [1, 0, 0, 1]], bool)
    enc = M.encode_prior(metres, acc)
    assert enc.dtype == np.uint16
    np.testing.assert_array_equal(enc, [[1536, 0, 2, 2562], [65535, 0, 0, 640]])                  # refused pixels are 0; half to even; clamp
    M._write_png16(str(tmp_path / 'p.png'), enc)
    np.testing.assert_array_equal(np.asarray(Image.open(str(tmp_path / 'p.png'))), enc)
    assert ((D.convert_depth(enc) > 0) == acc).all()                                            # what the loaders make of it
    np.testing.assert_array_equal(M.encode_std(np.array([0.0, 0.5, 0.001, 9.0]), np.array([1, 1, 1, 0], bool)), [2, 128, 2, 0])


def test_report_and_totals_line(tmp_path):
    rows = np.array([[3, 1, 1, 1], [1, 0, 1, 4]])
    status = np.array([[[0, 0, 0, 1, 2, 3]], [[0, 2, 3, 3, 3, 3]]], np.uint8)
    out = np.array([[[1.0, 2.0, 2.2, 0.0, 0.0, 0.0]], [[3.0, 0.0, 0.0, 0.0, 0.0, 0.0]]], np.float32)
    gt = np.array([[[1.0, 2.0, 2.0, 4.0, 5.0, 1.0]], [[2.0, 2.0, 1.0, 1.0, 1.0, 0.0]]], np.float32)
    M.write_report(str(tmp_path / 'mvs.txt'), ['a.png', 'b.png'], rows, status, out, gt)
    lines = (tmp_path / 'mvs.txt').read_text().splitlines()
    assert lines[0].split() == ['#', 'frame'] + list(M.ROW_NAMES) + ['coverage', 'absrel_accepted']
    a, tot = lines[1].split(), lines[-1].split()
    assert a[:5] == ['a.png', '3', '1', '1', '1'] and tot[:5] == ['total', '4', '1', '2', '5']
    assert float(a[5]) == 0.5 and float(tot[5]) == round(4 / 12, 6)
    assert abs(float(a[6]) - 0.1 / 3) < 1e-6 and abs(float(lines[2].split()[6]) - 0.5) < 1e-6 and abs(float(tot[6]) - 0.15) < 1e-6
    M.write_report(str(tmp_path / 'n.txt'), ['a.png', 'b.png'], rows, status)
    assert (tmp_path / 'n.txt').read_text().splitlines()[-1] == 'total 4 1 2 5 0.333333'
    assert M.totals_line(rows, 4, 64) == ('depth plane sweep (4 views, 64 planes): 2 frames, 4 pixels accepted, 1 at an end of the table, '
                                          '2 ambiguous, 5 unseen (coverage 33.3 %)')


# ------------------------------------------------------------------------------------------------ 5. both flag surfaces
def _colmap(tmp_path, **kw):
    from tests.test_depth_consistency import write_colmap_scene
    write_colmap_scene(str(tmp_path), **kw)
    return ["Config.data_dir = '%s'" % tmp_path]


def test_mip360_config_keys_parse_and_refusals(tmp_path):
    cfg = D.parse_gin(bindings=[])
    assert cfg['depth_mvs_views'] == 0 and cfg['depth_mvs_std_floor'] == 0.0
    assert M.check_params(4, **M.scene_params(cfg)) == M.check_params()
    cfg = D.parse_gin(bindings=['Config.depth_mvs_views = 3', 'Config.depth_mvs_planes = 32', 'Config.depth_mvs_near = 1.5', 'Config.depth_mvs_far = 50.0',
                                'Config.depth_mvs_agg_radius = 1', 'Config.depth_mvs_std_floor = 0.5'])
    assert M.scene_params(cfg, 0.1) == dict(planes=32, near=0.15000000000000002, far=5.0, best_views=0, agg_radius=1, uniqueness=0.9,
                                           std_planes=0.5, std_floor=0.05)
    base = _colmap(tmp_path, F=10, H=8, W=10)
    s = D.Scene(D.parse_gin(bindings=base + ["Config.depth_sup_type = 'mvs'", 'Config.depth_mvs_views = 4']))     # no depths_mvs/ on disk
    assert s.depth_mvs_views == 4 and s.depth_mvs_prm['best_views'] == 2 and not s.depths_sup.any()
    assert s.depth_mvs_prm['near'] == 2.0 * s.scale and s.depth_mvs_prm['far'] == 100.0 * s.scale
    assert D.Scene(D.parse_gin(bindings=base + ["Config.depth_sup_type = 'noisy'"])).depth_mvs_views == 0
    for extra, text in ((["Config.depth_sup_type = 'noisy'", 'Config.depth_mvs_views = 4'], r"Config.depth_mvs_views = 4 .* Config.depth_sup_type = 'mvs'"),
                        (["Config.depth_sup_type = 'mvs'", 'Config.depth_mvs_views = 4', 'Config.compute_disp_metrics = False'],
                         'Config.depth_mvs_views = 4 .* Config.compute_disp_metrics = True'),
                        (["Config.depth_sup_type = 'mvs'", 'Config.depth_mvs_views = 17'], r'Config.depth_mvs_views = 17: expected 0 \(off\) .. 16'),
                        (["Config.depth_sup_type = 'mvs'", 'Config.depth_mvs_views = 2', 'Config.depth_mvs_planes = 2'], r'Config.depth_mvs_\*: planes = 2'),
                        (["Config.depth_sup_type = 'mvs'", 'Config.depth_mvs_views = 2', 'Config.depth_mvs_best_views = 3'], r'Config.depth_mvs_\*: best_views = 3')):
        with pytest.raises(D.ConfigError, match=text):
            D.Scene(D.parse_gin(bindings=base + extra))
    # a gnll run without a folder or a constant takes its standard deviation from the sweep; a constant comes first
    g = D.Scene(D.parse_gin(bindings=base + ["Config.depth_sup_type = 'mvs'", 'Config.depth_mvs_views = 4', "Config.depth_loss_type = 'gnll'"]))
    assert g.depth_std_source == 'mvs'
    g = D.Scene(D.parse_gin(bindings=base + ["Config.depth_sup_type = 'mvs'", 'Config.depth_mvs_views = 4', "Config.depth_loss_type = 'gnll'",
                                             'Config.depth_gnll_std = 0.1']))
    assert g.depth_std_source == 'constant'


def test_nerfpp_flags_parse_and_refusals():
    pytest.importorskip('torch')
    from outdoor_nerf_depth_amd import ddp_train_nerf as T_
    base = ['--expname', 'x', '--synthetic']
    args = T_.config_parser().parse_args(base)
    assert args.depth_mvs_views == 0 and M.check_params(4, **M.args_params(args)) == M.check_params()
    args = T_.config_parser().parse_args(base + ['--depth_mvs_views', '3', '--depth_mvs_planes', '32', '--depth_mvs_far', 'inf',
                                                 '--depth_mvs_std_floor', '0.5'])
    assert M.args_params(args, 0.1) == dict(planes=32, near=0.2, far=float('inf'), best_views=0, agg_radius=2, uniqueness=0.9, std_planes=0.5,
                                           std_floor=0.05)
    cli = M.make_parser().parse_args(['--data_dir', 'd', '--views', '2', '--planes', '16', '--gin_bindings', 'Config.factor = 2'])
    assert cli.views == 2 and M.args_params(cli, 1.0, '')['planes'] == 16 and cli.gin_bindings == ['Config.factor = 2']
    assert M.make_parser().parse_args(['--datadir', 'd', '--scene', 's']).views == 4
    T_.validate_args(T_.config_parser().parse_args(base + ['--use_depth', '--depth_sup_type', 'mvs', '--depth_mvs_views', '16']))
    for bad, text in ((['--use_depth', '--depth_sup_type', 'mvs', '--depth_mvs_views', '17'], r'--depth_mvs_views = 17: expected 0 \(off\) .. 16'),
                      (['--use_depth', '--depth_sup_type', 'mvs', '--depth_mvs_views', '-1'], '--depth_mvs_views = -1'),
                      (['--depth_sup_type', 'mvs', '--depth_mvs_views', '4'], '--depth_mvs_views .* needs --use_depth'),
                      (['--use_depth', '--depth_sup_type', 'gt', '--depth_mvs_views', '4'], '--depth_mvs_views .* needs --depth_sup_type mvs'),
                      (['--use_depth', '--depth_sup_type', 'mvs', '--depth_mvs_views', '2', '--depth_mvs_planes', '2'], r'--depth_mvs_\*: planes = 2')):
        with pytest.raises(SystemExit, match=text):
            T_.validate_args(T_.config_parser().parse_args(base + bad))
    for bad in (['--planes', '3'], ['--views', '0'], ['--uniqueness', '2'], ['--near', '5', '--far', '4']):
        with pytest.raises(SystemExit, match='expected'):
            M.main(['--data_dir', 'd'] + bad)

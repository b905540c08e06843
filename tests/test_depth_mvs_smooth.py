"""No GPU: semi-global smoothing of the plane-sweep depth prior -- the reference's two forms against each other, on
hand-built cases and on the textured box scene with a band of the world painted one grey, the host side (parameters, flags, Config
keys, the dictionaries with smoothing off and on), the header against the binding, and the library's argument checks and workspace.

The band scene: scene((8, 48, 64)) of tests/test_depth_mvs.py, where the lattice cells with q_x in [-4, 4) -- 16.3 % of the pixels --
are painted grey 128: the census is flat there and the plain sweep's cost curves tie.  The conditions asserted on it are conditions
on the reference (what smoothing has to buy to be worth having), not tolerances of the kernel.
"""
import os
import re

import numpy as np
import pytest

from outdoor_nerf_depth_amd import depth_mvs as M
from outdoor_nerf_depth_amd import depth_mvs_flags as FL
from outdoor_nerf_depth_amd import mip360_data as D
from tests import depth_mvs_reference as R
from tests import depth_mvs_smooth_reference as SR
from tests.test_depth_mvs import LATTICE, SHAPES, hand_case, nbr_of, scene, world_points, _eye_cams, _texture, TABLE8

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAND_SHAPE = SHAPES[2]
GREY = 128

_band = {}


def band_scene():
    """scene(BAND_SHAPE) with the band painted: {'rgb', 'band' bool [F, H, W], ...the scene's own keys}; built once, read-only"""
    if not _band:
        s = dict(scene(BAND_SHAPE))
        q = np.floor(world_points(s['K'], s['c2w'], s['depth']) / LATTICE).astype(np.int64)
        band = (q[..., 0] >= -4) & (q[..., 0] < 4)
        rgb = s['rgb'].copy()
        rgb[band] = GREY
        for a in (rgb, band):
            a.setflags(write=False)
        s.update(rgb=rgb, band=band)
        _band.update(s)
    return _band


_refs = {}


def smooth_reference(key, rgb, cams, nbr, table, **kw):
    """SR.sweep computed once per key and shared (read-only) with tests/test_gpu_depth_mvs_smooth.py"""
    if key not in _refs:
        _refs[key] = SR.sweep(rgb, cams, nbr, table, **kw)
    return _refs[key]


def scene_reference(shape, views, agg_radius, paths, edge):
    s = scene(shape)
    return smooth_reference(('scene', tuple(shape), views, agg_radius, paths, edge), s['rgb'], s['cams'], nbr_of(shape, views), s['inv_depth'],
                            agg_radius=agg_radius, smooth_paths=paths, smooth_edge=edge)


def shares(out, s, mask=None):
    """(share of pixels accepted within two plane steps of the truth, share accepted farther off), over the pixels of mask"""
    acc = out['status'] == R.ACCEPTED
    step = s['inv_depth'][1] - s['inv_depth'][0]
    with np.errstate(divide='ignore'):
        near = np.abs(1.0 / out['depth'].astype(np.float64) - 1.0 / s['depth'].astype(np.float64)) <= 2 * step
    good, bad = acc & near, acc & ~near
    if mask is not None:
        good, bad = good[mask], bad[mask]
    return good.mean(), bad.mean()


# ------------------------------------------------------------------------------------------------ 1. the reference's two forms
@pytest.mark.parametrize('paths', (4, 8))
@pytest.mark.parametrize('edge', (0, 8))
def test_reference_vectorised_and_scalar_forms_agree(paths, edge):
    rs = np.random.RandomState(7 + paths + edge)
    shape, views, radius = SHAPES[0], 2, 1
    s, nbr = scene(shape), nbr_of(shape, views)
    ref = scene_reference(shape, views, radius, paths, edge)
    F, H, W = shape
    for i in (0, F - 1):
        vol = SR.volumes(s['rgb'], s['cams'], nbr, s['inv_depth'], i, R.best_default(views), radius)
        picks = [(0, 0), (H - 1, W - 1), (0, W - 1), (H - 1, 0)] + [(rs.randint(H), rs.randint(W)) for _ in range(8)]
        for y, x in picks:
            z, sd, status, k, c, sec = SR.sweep_pixel(s['rgb'], s['cams'], nbr, s['inv_depth'], i, y, x, None, radius, smooth_paths=paths,
                                                      smooth_edge=edge, vol=vol)
            got = tuple(ref[n][i, y, x] for n in ('depth', 'std', 'status', 'plane', 'cost', 'second'))
            assert (z.view(np.int32), sd.view(np.int32), status, k, c, sec) == (got[0].view(np.int32), got[1].view(np.int32)) + got[2:], (i, y, x)
    assert (ref['rows'].sum(1) == H * W).all() and (ref['status'] == R.ACCEPTED).any() and (ref['status'] != R.ACCEPTED).any()


# ------------------------------------------------------------------------------------------------ 2. hand-built cases
def _volume(D, H, W, seed=0, hi=600):
    rs = np.random.RandomState(seed)
    return rs.randint(0, hi, (D, H, W)).astype(np.int64), rs.randint(0, 256, (H, W)).astype(np.int64)


def test_costs_equal_in_k_are_only_multiplied():
    C, Y = _volume(1, 9, 13)
    C = np.repeat(C, 6, 0)                                                     # every plane of a pixel costs the same
    for n in (4, 8):
        for edge in (0, 8):
            S = np.sum(SR.paths(C, Y, n, 5, 40, edge), 0)
            np.testing.assert_array_equal(S, n * C)
    rgb, cams, nbr, table, prm = hand_case('identical')                          # ... and the sweep ends as the plain one does
    plain, smooth = R.sweep(rgb, cams, nbr, table, **prm), SR.sweep(rgb, cams, nbr, table, **prm)
    assert (smooth['status'] == R.END).all() and (smooth['plane'] == 0).all()
    np.testing.assert_array_equal(smooth['status'], plain['status'])
    np.testing.assert_array_equal(smooth['cost'], 8 * plain['cost'].astype(np.uint32))


@pytest.mark.parametrize('hw', ((1, 1), (1, 9), (9, 1)))
def test_a_frame_of_one_pixel_row_or_column(hw):
    """the diagonals, and the directions across the frame, have length 1: L = C there"""
    H, W = hw
    C, Y = _volume(5, H, W, seed=3)
    Ls = SR.paths(C, Y, 8, 7, 30, 0)
    along = {(1, 1): (), (1, 9): (0, 1), (9, 1): (2, 3)}[hw]                       # the directions with more than one pixel
    for r, L in enumerate(Ls):
        if r not in along:
            np.testing.assert_array_equal(L, C, err_msg='direction %d' % r)
        for y in range(H):
            for x in range(W):
                assert L[:, y, x].tolist() == SR.path_pixel(C, Y, y, x, SR.DIRS[r][0], SR.DIRS[r][1], 7, 30, 0), (r, y, x)
    if along:
        assert any((Ls[r] != C).any() for r in along)


def test_p1_equal_to_p2():
    """with P1 = P2 a change of one plane costs what a jump costs: L = C + min(L(q, k), M + P) - M"""
    C, Y = _volume(7, 6, 11, seed=5)
    P = 25
    L = SR.path(C, Y, 1, 0, P, P, 0)
    for x in range(1, 11):
        Lq = L[:, :, x - 1]
        Mq = Lq.min(0)
        np.testing.assert_array_equal(L[:, :, x], C[:, :, x] + np.minimum(Lq, Mq + P) - Mq)
    np.testing.assert_array_equal(L[:, :, 0], C[:, :, 0])


def test_a_luma_step_lowers_p2_to_the_written_value():
    C = np.zeros((4, 1, 2), np.int64)
    C[1:, 0, 0] = 1000                                                          # the predecessor: plane 0 costs 0, the others 1000
    P1, P2 = 3, 100
    for step, edge, want in ((0, 8, 100), (7, 8, 100), (8, 8, 50), (40, 8, 100 // 6), (255, 8, 3), (40, 0, 100), (255, 1, 3), (33, 255, 100)):
        Y = np.array([[10, 10 + step]], np.int64) if step <= 245 else np.array([[0, step]], np.int64)
        L = SR.path(C, Y, 1, 0, P1, P2, edge)
        assert L[:, 0, 1].tolist() == [0, P1, want, want], (step, edge)          # plane 3 (and 2) pays the jump: exactly P2'
        assert SR.path_pixel(C, Y, 0, 1, 1, 0, P1, P2, edge) == [0, P1, want, want]
        assert SR.path(C[:, :, ::-1], Y[:, ::-1], -1, 0, P1, P2, edge)[:, 0, 0].tolist() == [0, P1, want, want]      # |dY|, either way


def test_bounds_of_a_path_and_of_the_sum_at_the_largest_cost():
    """agg_radius 4, 16 views, best_views 16: a pixel whose window no view sees at a plane costs C = 24 * 16 * 81 = 31104 there.  At
    the largest P2 the table allows (smooth_p2 = 25: 32400) L <= C + P2 < 2^16 and S < 2^19."""
    H, W = 20, 40
    img = _texture(H, W)
    rgb = np.stack([img, img], 0)
    cams = _eye_cams(2, 32.0, H, W, [(0, 0, 0), (-4.0, 0, 0)])                     # disparities of 8 .. 64 pixels: a part is never seen
    nbr = np.array([[1] * 16, [0] * 16])
    C, n_in, Y = SR.volumes(rgb, cams, nbr, TABLE8, 0, 16, 4)
    assert C.max() == 31104 and C.min() < 31104
    P1, P2 = SR.penalties(16, 4, 1, 25)
    assert (P1, P2) == (1296, 32400)
    with pytest.raises(AssertionError):
        SR.penalties(16, 4, 1, 26)                                              # 33696 > 32767
    for edge in (0, 8):
        Ls = SR.paths(C, Y, 8, P1, P2, edge)
        for L in Ls:
            assert (L >= C).all() and (L <= C + P2).all() and L.max() < 1 << 16
        assert np.sum(Ls, 0).max() < 1 << 19
    out = SR.sweep(rgb, cams, nbr, TABLE8, 16, 4, smooth_p2=25, keep=True)
    assert out['L_max'] <= 31104 + 32400 and out['S'].max() < 1 << 19 and out['cost'].max() > 65535      # the uint32 is needed


# ------------------------------------------------------------------------------------------------ 3. the band scene
def test_smoothing_buys_coverage_on_the_band_scene():
    """8 paths, smooth_p1 1, smooth_p2 8, the defaults otherwise, against the plain reference.  Measured with these references: accepted
    within two plane steps 0.8484 -> 0.9281 over all pixels (+0.080) and 0.6809 -> 0.8530 inside the band (+0.172); accepted
    farther off 0.0108 -> 0.0234 over all pixels (0.0541 -> 0.1036 inside the band).  The gates: +0.05, +0.10 and at most 0.035."""
    s = band_scene()
    assert abs(s['band'].mean() - 0.163) < 0.001
    nbr = nbr_of(BAND_SHAPE, 4)
    plain = R.sweep(s['rgb'], s['cams'], nbr, s['inv_depth'])
    smooth = smooth_reference('band', s['rgb'], s['cams'], nbr, s['inv_depth'], smooth_paths=8, smooth_p1=1, smooth_p2=8)
    (pg, pb), (sg, sb) = shares(plain, s), shares(smooth, s)
    (pgb, pbb), (sgb, sbb) = shares(plain, s, s['band']), shares(smooth, s, s['band'])
    print('all pixels: good %.4f -> %.4f, bad %.4f -> %.4f; band: good %.4f -> %.4f, bad %.4f -> %.4f' % (pg, sg, pb, sb, pgb, sgb, pbb, sbb))
    assert sg >= pg + 0.05
    assert sgb >= pgb + 0.10
    assert sb <= 0.035


# ------------------------------------------------------------------------------------------------ 4. the host side
PLAIN = dict(views=4, planes=64, near=2.0, far=100.0, best_views=2, agg_radius=2, uniqueness=0.9, std_planes=0.5, std_floor=0.0)


def test_parameters_are_checked_by_name():
    assert M.check_params() == PLAIN and M.check_params(smooth_paths=0, smooth_p1=-5, smooth_p2='x', smooth_edge=999) == PLAIN
    on = M.check_params(smooth_paths=8)
    assert on == dict(PLAIN, smooth_paths=8, smooth_p1=1, smooth_p2=8, smooth_edge=0) and M.smooth_penalties(on) == (50, 400)
    assert {k: v[0] for k, v in FL.SMOOTH.items()} == dict(smooth_paths=0, smooth_p1=1, smooth_p2=8, smooth_edge=0)
    assert {k: v[0] for k, v in FL.SMOOTH.items() if k != 'smooth_paths'} == {k: v for k, v in SR.DEFAULTS.items() if k != 'smooth_paths'}
    assert not set(FL.SMOOTH) & set(FL.PARAMS)
    assert M.check_params(smooth_paths=4, smooth_p1=3, smooth_p2=3, smooth_edge=255)['smooth_edge'] == 255
    assert M.smooth_penalties(M.check_params(views=16, best_views=16, agg_radius=4, smooth_paths=8, smooth_p2=25)) == (1296, 32400)
    assert (M.MAX_P2, M.MAX_EDGE) == (SR.MAX_P2, 255)
    for kw, text in ((dict(smooth_paths=3), r'smooth_paths = 3: expected 0 \(off\), 4 or 8'), (dict(smooth_paths=-8), 'smooth_paths = -8'),
                     (dict(smooth_paths=True), 'smooth_paths = True'), (dict(smooth_paths=8.5), 'smooth_paths = 8.5'),
                     (dict(smooth_paths=8, smooth_p1=0), r'smooth_p1 = 0: expected an integer 1 .. 32767'),
                     (dict(smooth_paths=8, smooth_p1=1.5), 'smooth_p1 = 1.5'),
                     (dict(smooth_paths=8, smooth_p2=0), 'smooth_p2 = 0: expected an integer'),
                     (dict(smooth_paths=8, smooth_p1=9), r'smooth_p1 = 9, smooth_p2 = 8: .* P1 = 450, P2 = 400, expected P1 <= P2 <= 32767'),
                     (dict(smooth_paths=4, smooth_p2=700), r'smooth_p1 = 1, smooth_p2 = 700: .*best_views = 2 .* 25 taps.* P1 = 50, P2 = 35000'),
                     (dict(smooth_paths=8, views=16, best_views=16, agg_radius=4, smooth_p2=26), 'P1 = 1296, P2 = 33696'),
                     (dict(smooth_paths=8, smooth_edge=256), r'smooth_edge = 256: expected an integer 0 .. 255'),
                     (dict(smooth_paths=8, smooth_edge=-1), 'smooth_edge = -1')):
        with pytest.raises(M.DepthMvsError, match=text):
            M.check_params(**kw)


def test_dictionaries_are_unchanged_with_smoothing_off_and_extended_with_it_on(tmp_path):
    pytest.importorskip('torch')
    from outdoor_nerf_depth_amd import ddp_train_nerf as T_
    call = dict(planes=64, near=2.0, far=100.0, best_views=0, agg_radius=2, uniqueness=0.9, std_planes=0.5, std_floor=0.0)
    cfg = D.parse_gin(bindings=[])
    assert [cfg['depth_mvs_' + k] for k in ('smooth_paths', 'smooth_p1', 'smooth_p2', 'smooth_edge')] == [0, 1, 8, 0]
    assert M.scene_params(cfg) == call and M.check_params(4, **M.scene_params(cfg)) == PLAIN
    cfg = D.parse_gin(bindings=['Config.depth_mvs_smooth_p1 = 2', 'Config.depth_mvs_smooth_edge = 8'])                # paths 0: still off
    assert M.scene_params(cfg, 0.5) == dict(call, near=1.0, far=50.0)
    cfg = D.parse_gin(bindings=['Config.depth_mvs_smooth_paths = 4', 'Config.depth_mvs_smooth_p2 = 6', 'Config.depth_mvs_planes = 32'])
    assert M.scene_params(cfg, 0.5) == dict(call, planes=32, near=1.0, far=50.0, smooth_paths=4, smooth_p1=1, smooth_p2=6, smooth_edge=0)
    base = ['--expname', 'x', '--synthetic']
    args = T_.config_parser().parse_args(base)
    assert M.args_params(args) == call and M.check_params(4, **M.args_params(args)) == PLAIN
    assert M.args_params(T_.config_parser().parse_args(base + ['--depth_mvs_smooth_p2', '3'])) == call
    args = T_.config_parser().parse_args(base + ['--depth_mvs_smooth_paths', '8', '--depth_mvs_smooth_edge', '16'])
    assert M.args_params(args, 0.1) == dict(call, near=0.2, far=10.0, smooth_paths=8, smooth_p1=1, smooth_p2=8, smooth_edge=16)
    cli = M.make_parser().parse_args(['--data_dir', 'd'])
    assert M.args_params(cli, 1.0, '') == call
    cli = M.make_parser().parse_args(['--data_dir', 'd', '--smooth_paths', '4', '--smooth_p1', '2', '--smooth_p2', '5', '--smooth_edge', '3'])
    assert M.args_params(cli, 1.0, '') == dict(call, smooth_paths=4, smooth_p1=2, smooth_p2=5, smooth_edge=3)


def test_flags_and_config_keys_are_refused_by_name(tmp_path):
    pytest.importorskip('torch')
    from outdoor_nerf_depth_amd import ddp_train_nerf as T_
    from tests.test_depth_consistency import write_colmap_scene
    write_colmap_scene(str(tmp_path), F=10, H=8, W=10)
    base = ["Config.data_dir = '%s'" % tmp_path, "Config.depth_sup_type = 'mvs'", 'Config.depth_mvs_views = 4']
    s = D.Scene(D.parse_gin(bindings=base + ['Config.depth_mvs_smooth_paths = 8']))
    assert s.depth_mvs_prm['smooth_paths'] == 8 and s.depth_mvs_prm['smooth_p2'] == 8
    assert 'smooth_paths' not in D.Scene(D.parse_gin(bindings=base)).depth_mvs_prm
    for extra, text in ((['Config.depth_mvs_smooth_paths = 3'], r'Config.depth_mvs_\*: smooth_paths = 3: expected 0 \(off\), 4 or 8'),
                        (['Config.depth_mvs_smooth_paths = 8', 'Config.depth_mvs_smooth_p1 = 9'], r'Config.depth_mvs_\*: smooth_p1 = 9, smooth_p2 = 8'),
                        (['Config.depth_mvs_smooth_paths = 8', 'Config.depth_mvs_smooth_p2 = 700'], 'P2 = 35000, expected P1 <= P2 <= 32767'),
                        (['Config.depth_mvs_smooth_paths = 4', 'Config.depth_mvs_smooth_edge = 300'], r'Config.depth_mvs_\*: smooth_edge = 300')):
        with pytest.raises(D.ConfigError, match=text):
            D.Scene(D.parse_gin(bindings=base + extra))
    flags = ['--expname', 'x', '--synthetic', '--use_depth', '--depth_sup_type', 'mvs', '--depth_mvs_views', '4']
    T_.validate_args(T_.config_parser().parse_args(flags + ['--depth_mvs_smooth_paths', '8']))
    for bad, text in ((['--depth_mvs_smooth_paths', '5'], r'--depth_mvs_\*: smooth_paths = 5'),
                      (['--depth_mvs_smooth_paths', '4', '--depth_mvs_smooth_p1', '0'], r'--depth_mvs_\*: smooth_p1 = 0'),
                      (['--depth_mvs_smooth_paths', '4', '--depth_mvs_smooth_p2', '700'], 'P2 = 35000')):
        with pytest.raises(SystemExit, match=text):
            T_.validate_args(T_.config_parser().parse_args(flags + bad))
    for bad in (['--smooth_paths', '2'], ['--smooth_paths', '8', '--smooth_p1', '10'], ['--smooth_paths', '8', '--smooth_edge', '256']):
        with pytest.raises(SystemExit, match='expected'):
            M.main(['--data_dir', 'd'] + bad)


# ------------------------------------------------------------------------------------------------ 5. the library, no GPU
def test_binding_declares_the_headers_symbols_and_constants():
    from outdoor_nerf_depth_amd import depth_mvs_smooth as MS
    header = open(os.path.join(ROOT, 'include', 'depthsgm_hip.h')).read()
    declared = set(re.findall(r'^(?:const char\*|int64_t|int) (depthsgm_\w+)\(', header, re.M))
    assert declared == set(MS.SYMBOLS) and len(declared) == 4
    const = dict(re.findall(r'#define DEPTHSGM_(\w+) \(?(\d+)', header))
    assert tuple(int(const[k]) for k in ('ABI_VERSION', 'MAX_P2', 'MAX_EDGE', 'PLANE_ALIGN', 'SLAB_ENTRY_BYTES')) == \
        (MS.ABI_VERSION, M.MAX_P2, M.MAX_EDGE, MS.PLANE_ALIGN, MS.SLAB_ENTRY_BYTES)
    assert [int(const[k]) for k in ('OK', 'ERR_ARG', 'ERR_HIP')] == [0, 1, 2]
    for name in ('depthsgm_sweep', 'depthsgm_workspace_bytes'):
        assert len(MS.SYMBOLS[name][1]) == header.split(' %s(' % name)[1].split(');')[0].count(',') + 1
    plain = open(os.path.join(ROOT, 'include', 'depthmvs_hip.h')).read()
    sweep_args = lambda text, fn: [a.split()[-1].lstrip('*') for a in text.split(' %s(' % fn)[1].split(');')[0].split(',')]
    theirs, ours = sweep_args(plain, 'depthmvs_sweep'), sweep_args(header, 'depthsgm_sweep')
    assert [a for a in ours if a not in theirs] == ['smooth_paths', 'p1', 'p2', 'smooth_edge', 'slab_frames'] and [a for a in ours if a in theirs] == theirs


def test_library_argument_checks_need_no_gpu():
    import ctypes as C
    from outdoor_nerf_depth_amd import depth_mvs_smooth as MS
    lib = MS.lib()
    assert lib.depthsgm_abi_version() == MS.ABI_VERSION
    buf = (C.c_double * 16384)()                                                 # host memory: every call below fails before any launch
    base = (C.addressof(buf) + 255) // 256 * 256
    at = lambda k: C.c_void_p(base + 4096 * k)

    def call(F=1, H=2, W=2, V=2, Dn=8, rgb=at(0), cams=at(1), nbr=at(2), inv=at(3), best=1, radius=2, uniq=0.9, stdp=0.5, paths=8, p1=25,
             p2=200, edge=0, slab=1, ws=at(12), depth=at(4), std=at(5), status=at(6), plane=None, cost=None, second=None, census=None,
             rows=None):
        return lib.depthsgm_sweep(None, F, H, W, V, Dn, rgb, cams, nbr, inv, best, radius, uniq, stdp, paths, p1, p2, edge, slab, ws, depth,
                                  std, status, plane, cost, second, census, rows)
    for kw, text in ((dict(F=0), 'n_frames = 0'), (dict(F=65536), 'n_frames = 65536'), (dict(H=0), 'at least one pixel'),
                     (dict(V=0), 'n_views = 0, expected 1 .. 16'), (dict(V=17), 'n_views = 17'), (dict(Dn=3), 'n_planes = 3, expected 4 .. 256'),
                     (dict(Dn=257), 'n_planes = 257'), (dict(best=0), 'best_views = 0, expected 1 .. n_views = 2'), (dict(best=3), 'best_views = 3'),
                     (dict(radius=-1), 'agg_radius = -1, expected 0 .. 4'), (dict(radius=5), 'agg_radius = 5'), (dict(uniq=0.0), 'uniqueness = 0'),
                     (dict(uniq=1.5), 'uniqueness = 1.5'), (dict(uniq=float('nan')), 'uniqueness = nan'), (dict(stdp=0.0), 'std_planes = 0'),
                     (dict(stdp=float('inf')), 'std_planes = inf'),
                     (dict(paths=0), 'smooth_paths = 0, expected 4 or 8'), (dict(paths=6), 'smooth_paths = 6'), (dict(paths=16), 'smooth_paths = 16'),
                     (dict(p1=0), 'p1 = 0, p2 = 200: expected 1 <= p1 <= p2 <= 32767'), (dict(p1=201), 'p1 = 201, p2 = 200'),
                     (dict(p2=32768), 'p1 = 25, p2 = 32768'), (dict(edge=-1), 'smooth_edge = -1, expected 0 .. 255'), (dict(edge=256), 'smooth_edge = 256'),
                     (dict(slab=0), 'slab_frames = 0, expected at least 1'), (dict(slab=-3), 'slab_frames = -3'),
                     (dict(rgb=None), 'non-null rgb, cams, nbr, inv_depth, workspace'),
                     (dict(inv=None), 'non-null rgb, cams, nbr, inv_depth, workspace'), (dict(status=None), 'non-null depth, std, status'),
                     (dict(depth=at(0)), 'depth overlaps rgb'), (dict(std=at(1)), 'std overlaps cams'), (dict(status=at(2)), 'status overlaps nbr'),
                     (dict(plane=at(3)), 'plane overlaps inv_depth'), (dict(cost=at(0)), 'cost overlaps rgb'), (dict(second=at(1)), 'second overlaps cams'),
                     (dict(census=at(0)), 'census overlaps rgb'), (dict(rows=at(0)), 'rows overlaps rgb'), (dict(ws=at(0)), 'workspace overlaps rgb'),
                     (dict(plane=at(4)), 'depth overlaps plane'), (dict(cost=at(6)), 'status overlaps cost'), (dict(depth=at(12)), 'depth overlaps workspace'),
                     (dict(ws=C.c_void_p(base + 4096 * 12 + 8)), 'workspace aligned to 256 bytes'),
                     (dict(depth=C.c_void_p(base + 4096 * 4 + 2)), 'aligned to 4 bytes'), (dict(cost=C.c_void_p(base + 4096 * 7 + 2)), 'aligned to 4 bytes'),
                     (dict(second=C.c_void_p(base + 4096 * 7 + 1)), 'aligned to 4 bytes'), (dict(cams=C.c_void_p(base + 4096 + 4)), 'aligned to 8 bytes')):
        assert call(**kw) == 1, kw
        assert text in MS.last_error(), (kw, MS.last_error())
    # the slabs are a part of the workspace: an output inside them overlaps it (F 1, 2 x 2, 8 planes: 768 + 256 bytes in all)
    assert MS.workspace_bytes(1, 2, 2, 8, 1) == 1024
    assert call(depth=C.c_void_p(base + 4096 * 12 + 768)) == 1 and 'depth overlaps workspace' in MS.last_error()


def test_workspace_bytes_layout_and_limits():
    from outdoor_nerf_depth_amd import depth_mvs_smooth as MS
    up = lambda n: (n + 255) // 256 * 256
    assert MS.workspace_bytes(1, 1, 1, 4, 1) == 4 * 256                           # census, partials, 8 uint16, 8 uint32
    F, H, W, Dn, s = 295, 375, 1242, 64, 22
    n, tiles = F * H * W, 24 * 39
    entries = s * H * W * Dn
    assert MS.workspace_bytes(F, H, W, Dn, s) == up(4 * n) + up(F * tiles * 16) + up(2 * entries) + up(4 * entries)
    assert MS.workspace_bytes(F, H, W, Dn, s) - M.workspace_bytes(F, H, W) == up(2 * entries) + up(4 * entries)
    assert MS.workspace_bytes(F, H, W, 65, s) == up(4 * n) + up(F * tiles * 16) + up(2 * s * H * W * 72) + up(4 * s * H * W * 72)
    assert MS.workspace_bytes(4, 8, 8, 16, 9) == MS.workspace_bytes(4, 8, 8, 16, 4)                 # no more slab frames than frames
    assert MS.workspace_bytes(65535, 8, 32, 4, 1) > 0 and MS.workspace_bytes(1, 1 << 14, 1 << 14, 256, 1) > 0
    for args, text in (((0, 4, 4, 8, 1), 'n_frames = 0, expected 1 .. 65535'), ((65536, 4, 4, 8, 1), 'n_frames = 65536'),
                       ((1, 0, 4, 8, 1), 'a frame has at least one pixel'), ((1, (1 << 14) + 1, 1 << 14, 8, 1), 'exceeds 2\\^28 pixels per frame'),
                       ((1, 4, 4, 3, 1), 'n_planes = 3, expected 4 .. 256'), ((1, 4, 4, 257, 1), 'n_planes = 257'),
                       ((1, 4, 4, 8, 0), 'slab_frames = 0, expected at least 1')):
        with pytest.raises(M.DepthMvsError, match=text):
            MS.workspace_bytes(*args)
    # the binding's budget: all frames if they fit, at least one; the default of 4 GiB holds 24 of the 295
    assert MS.slab_frames_of(F, H, W, Dn) == (4 << 30) // (6 * Dn * H * W) == 24
    assert MS.slab_frames_of(F, H, W, Dn, slab_bytes=0) == 1 and MS.slab_frames_of(3, 8, 8, 65, slab_bytes=1 << 30) == 3
    assert MS.slab_frames_of(10, 8, 8, 65, slab_bytes=2 * 6 * 72 * 64 + 5) == 2
    with pytest.raises(M.DepthMvsError, match='slab_bytes = -1'):
        MS.slab_frames_of(1, 1, 1, 4, -1)

"""No GPU: completing sparse depth priors by image-guided filtering -- the reference on the analytic scene of
tests/test_depth_consistency.py and on hand-built frames whose outcome is exact, the host side of
outdoor_nerf_depth_amd/depth_complete.py (argument checks, tables, PNG encoding, the report), the library's argument checks and both
flag surfaces.

The hand-built cases are functions of a `run` callable with the reference's signature, so that tests/test_gpu_depth_complete.py runs
the same ones through the device.
"""
import os

import numpy as np
import pytest

from outdoor_nerf_depth_amd import depth_complete as DCP
from outdoor_nerf_depth_amd import mip360_data as D
from tests import depth_complete_reference as R
from tests.test_depth_consistency import SHAPES, analytic_scene
from tests.test_depth_accumulate import prior_of

NONE, OWN, FILLED, REFUSED = R.ORIGIN_NONE, R.ORIGIN_OWN, R.ORIGIN_FILLED, R.ORIGIN_REFUSED
_guides = {}


def guide_of(shape):
    """The guide image of the box scene of `shape`: it follows the true surfaces (read-only, shared)"""
    if shape not in _guides:
        _guides[shape] = R.guide(analytic_scene(shape, box=True)['depth'], seed=shape[1])
        _guides[shape].setflags(write=False)
    return _guides[shape]


def std_of(shape):
    """A standard deviation for every pixel of `shape`, with zeros, negatives and NaN among them (they count as 0)"""
    rs = np.random.RandomState(shape[2])
    std = (0.02 + 0.1 * rs.rand(*shape)).astype(np.float32)
    bad = np.random.RandomState(shape[2] + 1).rand(*shape)
    std = np.where(bad < 0.05, np.float32(0), np.where(bad < 0.1, np.float32(-1), np.where(bad < 0.15, np.float32(np.nan), std)))
    return std.astype(np.float32)


def bits(a):
    return a.view(np.int32) if a.dtype == np.float32 else a


def flat(n):
    return np.ones(n, np.float64)


# ------------------------------------------------------------------------------------------------ the hand-built cases
def two_planes(H=12, W=20):
    """(depth, rgb, side): planes at 4.0 (left, red) and 9.0 (right, blue), measured at every third pixel"""
    yy, xx = np.mgrid[0:H, 0:W]
    side = np.where(xx < W // 2, np.float32(4.0), np.float32(9.0)).astype(np.float32)
    rgb = np.where((xx < W // 2)[..., None], np.array([200, 30, 30]), np.array([30, 30, 200])).astype(np.uint8)
    depth = np.where((xx + yy) % 3 == 0, side, np.float32(0)).astype(np.float32)
    return depth[None], rgb[None], side[None]


def case_two_planes_guided(run):
    """a colour table that is zero beyond 30 levels: nothing crosses the edge (the sides differ by 340), every pixel gets its side"""
    depth, rgb, side = two_planes()
    cut = (np.arange(766) <= 30).astype(np.float64)
    out = run(depth, rgb, None, flat(25), cut, 2, 2, min_points=1, min_conf=0.0, max_rel_spread=0.1, decay=0.5)
    assert (out['origin'] == np.where(depth > 0, OWN, FILLED)).all()
    np.testing.assert_array_equal(out['depth'], side)                           # exact: the mean of equal values rounds back to them
    assert out['std'].max() < 1e-6 and out['rows'].tolist() == [[80, 160, 0, 0]]
    return out


def case_two_planes_unguided(run):
    """the same under a flat colour table: an edge pixel lands in mid-air, and is REFUSED once max_rel_spread is finite"""
    depth, rgb, side = two_planes()
    kw = dict(min_points=1, min_conf=0.0, decay=0.5)
    free = run(depth, rgb, None, flat(25), flat(766), 2, 1, max_rel_spread=float('inf'), **kw)
    mid = (free['depth'] > 4.0) & (free['depth'] < 9.0)
    assert mid.sum() > 0 and (free['origin'][mid] == FILLED).all() and not (free['origin'] == REFUSED).any()
    gated = run(depth, rgb, None, flat(25), flat(766), 2, 1, max_rel_spread=0.1, **kw)
    assert (gated['origin'][mid] == REFUSED).any()
    same = gated['origin'][mid] == FILLED                                       # (a window that passes the gate gives what it gave)
    assert ((gated['origin'][mid] == REFUSED) | same).all()
    np.testing.assert_array_equal(gated['depth'][mid][same], free['depth'][mid][same])
    assert (gated['depth'][gated['origin'] == REFUSED] == 0).all() and gated['rows'][0, 2] == (gated['origin'] == REFUSED).sum()
    return free, gated


def case_window_wider_than_the_frame(run):
    kw = dict(min_points=1, min_conf=0.0, max_rel_spread=0.1, decay=0.5)
    rgb = np.full((1, 1, 1, 3), 7, np.uint8)
    out = run(np.zeros((1, 1, 1), np.float32), rgb, None, flat(289), flat(766), 8, 3, **kw)
    assert out['rows'].tolist() == [[0, 0, 0, 1]] and out['depth'][0, 0, 0] == 0 and out['origin'][0, 0, 0] == NONE
    out = run(np.full((1, 1, 1), 5.0, np.float32), rgb, None, flat(289), flat(766), 8, 3, **kw)
    assert out['rows'].tolist() == [[1, 0, 0, 0]] and out['depth'][0, 0, 0] == 5.0 and out['conf'][0, 0, 0] == 1.0
    depth = np.zeros((1, 5, 7), np.float32)
    depth[0, 2, 3] = 6.0
    out = run(depth, np.full((1, 5, 7, 3), 7, np.uint8), None, flat(289), flat(766), 8, 1, **kw)
    assert out['rows'].tolist() == [[1, 34, 0, 0]] and (out['depth'] == 6.0).all() and (out['pass'].sum() == 34)
    assert (out['conf'][out['origin'] == FILLED] == np.float32(0.5 * (1.0 / 35.0))).all()


def case_thresholds(run):
    """min_points and min_conf at their thresholds, on a row of 7 pixels with flat tables and radius 1: conf = measured taps / taps"""
    depth = np.zeros((1, 1, 7), np.float32)
    depth[0, 0, [0, 2]] = 5.0
    rgb = np.zeros((1, 1, 7, 3), np.uint8)
    kw = dict(max_rel_spread=0.1, decay=1.0)
    out = run(depth, rgb, None, flat(9), flat(766), 1, 1, min_points=2, min_conf=0.0, **kw)
    assert out['origin'][0, 0].tolist() == [OWN, FILLED, OWN, NONE, NONE, NONE, NONE]            # x = 3 sees one tap: one short
    out = run(depth, rgb, None, flat(9), flat(766), 1, 1, min_points=1, min_conf=0.0, **kw)
    assert out['origin'][0, 0].tolist() == [OWN, FILLED, OWN, FILLED, NONE, NONE, NONE] and out['depth'][0, 0, 3] == 5.0
    third = 1.0 / 3.0                                                                           # x = 3: one of three taps
    out = run(depth, rgb, None, flat(9), flat(766), 1, 1, min_points=1, min_conf=third, **kw)
    assert out['origin'][0, 0, 3] == FILLED and out['conf'][0, 0, 3] == np.float32(third)
    out = run(depth, rgb, None, flat(9), flat(766), 1, 1, min_points=1, min_conf=float(np.nextafter(third, 1.0)), **kw)
    assert out['origin'][0, 0].tolist() == [OWN, FILLED, OWN, NONE, NONE, NONE, NONE]


def case_reach(run, radius=2, iters=3):
    """the only measurement at x = 0: the pixel at iters * r is filled by the last pass, the one after it stays NONE"""
    W = iters * radius + 3
    depth = np.zeros((1, 1, W), np.float32)
    depth[0, 0, 0] = 7.0
    side = 2 * radius + 1
    out = run(depth, np.zeros((1, 1, W, 3), np.uint8), None, flat(side * side), flat(766), radius, iters, min_points=1, min_conf=0.0,
              max_rel_spread=0.1, decay=0.5)
    reach = iters * radius
    assert out['pass'][0, 0].tolist() == [0] + [1 + (x - 1) // radius for x in range(1, reach + 1)] + [0, 0]
    assert out['origin'][0, 0, reach] == FILLED and out['pass'][0, 0, reach] == iters and out['depth'][0, 0, reach] == 7.0
    assert out['origin'][0, 0, reach + 1] == NONE and out['depth'][0, 0, reach + 1] == 0 and out['conf'][0, 0, reach + 1] == 0
    return out


CASES = (case_two_planes_guided, case_two_planes_unguided, case_window_wider_than_the_frame, case_thresholds, case_reach)


# ------------------------------------------------------------------------------------------------ 1. the reference
@pytest.mark.parametrize('shape', SHAPES)
def test_reference_forms_agree(shape):
    rgb = guide_of(shape)
    wc = R.tables(2, 1.5, 20.0)[1]
    wide = R.tables(2, 1.5, 300.0)[1]                                          # a guide that barely guides: refusals at the box's edge
    n = 2 if shape == SHAPES[0] else 1                                          # (the scalar form is slow: fewer frames of the larger shapes)
    for kind, std, colour, r in (('sparse', None, wc, 1), ('invalids', std_of(shape), wide, 2)):
        prior = prior_of(kind, shape)[:n]
        std = None if std is None else std[:n]
        w = R.tables(r, 1.5, 20.0)[0]
        a = R.complete(prior, rgb[:n], std, w, colour, r, 2)
        b = R.complete_scalar(prior, rgb[:n], std, w, colour, r, 2)
        assert a['rows'][:, 1].sum() > 0 and a['rows'][:, 2 if colour is wide else 3].sum() > 0, a['rows']
        for k in a:
            np.testing.assert_array_equal(bits(a[k]), bits(b[k]), err_msg='%s %s' % (kind, k))
        snaps = R.complete(prior, rgb[:n], std, w, colour, r, 2, snapshots=(1, 2))
        one = R.complete(prior, rgb[:n], std, w, colour, r, 1)
        for k in a:
            np.testing.assert_array_equal(bits(a[k]), bits(snaps[2][k]))
            np.testing.assert_array_equal(bits(one[k]), bits(snaps[1][k]))


@pytest.mark.parametrize('case', CASES, ids=lambda c: c.__name__)
def test_hand_built_cases_on_the_reference(case):
    case(R.complete)
    case(R.complete_scalar)


def test_invariants_on_the_scene():
    shape = SHAPES[1]
    rgb, true = guide_of(shape), analytic_scene(shape, box=True)['depth']
    ws, wc = R.tables(4, 2.0, 20.0)
    for kind in ('sparse', 'invalids'):
        prior = prior_of(kind, shape)
        out = R.complete(prior, rgb, std_of(shape), ws, wc, 4, 3)
        kept = out['origin'] != FILLED
        np.testing.assert_array_equal(out['depth'].view(np.int32)[kept], prior.view(np.int32)[kept])   # own and invalid pixels: the same bits
        assert (out['rows'].sum(1) == shape[1] * shape[2]).all() and (out['rows'][:, 0] == (prior > 0).reshape(shape[0], -1).sum(1)).all()
        assert ((out['origin'] == OWN) == (prior > 0)).all() and (out['std'][~(out['conf'] > 0)] == 0).all()
        filled = out['origin'] == FILLED
        assert (out['pass'][filled] >= 1).all() and (out['pass'][~filled] == 0).all() and (out['conf'][filled] < 1).all()
        err = np.abs(out['depth'][filled].astype(np.float64) - true[filled]) / true[filled]
        print('%s: coverage %.3f -> %.3f, AbsRel of the filled %.4f' % (kind, (prior > 0).mean(), (out['conf'] > 0).mean(), err.mean()))
        assert filled.sum() > (prior > 0).sum()
    dense = prior_of('exact', shape)
    out = R.complete(dense, rgb, None, ws, wc, 4, 3)
    np.testing.assert_array_equal(out['depth'].view(np.int32), dense.view(np.int32))
    assert out['rows'][:, 1].sum() == 0 and (out['origin'] == OWN).all() and not out['std'].any()


# ------------------------------------------------------------------------------------------------ 2. the host side
def test_parameter_and_table_checks_name_the_argument():
    assert DCP.check_params() == dict(R.DEFAULTS, std_floor=0.0)
    assert DCP.check_params(radius=8, iters=16, min_points=289, min_conf=1, decay=1, max_rel_spread=float('inf'))['max_rel_spread'] == float('inf')
    for kw, text in ((dict(radius=0), r'radius = 0: expected an integer 1 .. 8'), (dict(radius=9), 'radius = 9'), (dict(radius=2.5), 'radius = 2.5'),
                     (dict(iters=0), r'iters = 0: expected an integer 1 .. 16'), (dict(iters=17), 'iters = 17'),
                     (dict(min_points=0), r'min_points = 0: expected an integer 1 .. 289'), (dict(min_points=290), 'min_points = 290'),
                     (dict(decay=0.0), r'decay = 0.0: expected a number in \(0, 1\]'), (dict(decay=1.5), 'decay = 1.5'),
                     (dict(min_conf=-0.1), r'min_conf = -0.1: expected a number in \[0, 1\]'), (dict(min_conf=float('nan')), 'min_conf = nan'),
                     (dict(max_rel_spread=-1.0), 'max_rel_spread = -1.0: expected a number >= 0'), (dict(max_rel_spread=float('nan')), 'max_rel_spread = nan'),
                     (dict(sigma_space=0.0), 'sigma_space = 0.0: expected a finite number > 0'), (dict(sigma_colour=float('inf')), 'sigma_colour = inf'),
                     (dict(std_floor=-1.0), 'std_floor = -1.0')):
        with pytest.raises(DCP.DepthCompError, match=text):
            DCP.check_params(**kw)
    ws, wc = DCP.tables(4, 2.0, 20.0)
    rs, rc = R.tables(4, 2.0, 20.0)
    np.testing.assert_array_equal(ws, rs)
    np.testing.assert_array_equal(wc, rc)
    assert ws.shape == (81,) and wc.shape == (766,) and ws[40] == 1.0 and wc[0] == 1.0 and ws[0] == ws[80] == np.exp(-32.0 / 8.0)
    a, b = DCP.check_tables(ws.reshape(9, 9), list(wc), 4)
    assert a.shape == (81,) and b.dtype == np.float64
    for w_space, w_colour, text in ((ws[:80], wc, r'w_space: 80 entries, expected 81'), (ws, wc[:765], 'w_colour: 765 entries, expected 766'),
                                    (-ws, wc, 'w_space: every entry must be finite and >= 0'),
                                    (ws, np.where(np.arange(766) == 5, np.nan, wc), 'w_colour: every entry must be finite'),
                                    (ws, np.where(np.arange(766) == 5, np.inf, wc), 'w_colour: every entry must be finite')):
        with pytest.raises(DCP.DepthCompError, match=text):
            DCP.check_tables(w_space, w_colour, 4)


def test_tensor_checks_name_the_tensor_before_the_device_is_asked():
    torch = pytest.importorskip('torch')
    depth, rgb = torch.zeros(2, 6, 8), torch.zeros(2, 6, 8, 3, dtype=torch.uint8)
    for bad in (np.zeros((2, 6, 8), np.float32), depth):                                       # no tensor; a host tensor, asked last
        with pytest.raises(DCP.DepthCompError, match='depth: expected a CUDA/HIP float32 tensor .* no CPU path'):
            DCP.complete_async(bad, rgb)
    for d, c, text in ((depth.double(), rgb, 'depth: expected torch.float32, got torch.float64'), (depth[0], rgb, r'depth: expected \[F, H, W\]'),
                       (depth[:, :, ::2], rgb, 'depth: expected a contiguous tensor'), (depth, rgb.float(), 'rgb: expected torch.uint8'),
                       (depth, rgb[..., :2], r'rgb: expected \[F, H, W, 3\], got \(2, 6, 8, 2\)'), (depth, rgb[0], r'rgb: expected \[F, H, W, 3\]'),
                       (depth, rgb[:1], r'rgb \(1, 6, 8, 3\): expected the frames \(2, 6, 8\) of depth'),
                       (depth, torch.zeros(2, 6, 16, 3, dtype=torch.uint8)[:, :, ::2], 'rgb: expected a contiguous tensor')):
        with pytest.raises(DCP.DepthCompError, match=text):
            DCP.complete_async(d, c)
    for std, text in ((depth.half(), 'std_in: expected torch.float32'), (depth[:1], r'std_in \(1, 6, 8\): expected the shape'),
                      (np.zeros((2, 6, 8), np.float32), 'std_in: expected a CUDA/HIP float32 tensor')):
        with pytest.raises(DCP.DepthCompError, match=text):
            DCP.complete_async(depth, rgb, std)
    std, buf = torch.ones(2, 6, 8), torch.zeros(2 * 6 * 8 * 4, dtype=torch.uint8)
    rgb = buf[:2 * 6 * 8 * 3].view(2, 6, 8, 3)
    for out, text in ((depth, 'depth_out overlaps depth'), (std, 'depth_out overlaps std_in'), (depth[1:], r'depth_out \(1, 6, 8\)'),
                      (depth.int(), 'depth_out: expected torch.float32'), (torch.zeros(2, 6, 16)[:, :, ::2], 'depth_out: expected a contiguous tensor'),
                      (buf.view(torch.float32).view(2, 6, 8), 'depth_out overlaps rgb')):
        with pytest.raises(DCP.DepthCompError, match=text):
            DCP.complete_async(depth, rgb, std, depth_out=out)


# ------------------------------------------------------------------------------------------------ 3. the library, no GPU
def test_workspace_bytes_limits():
    assert DCP.workspace_bytes(1, 1, 1) == 4 * 256 + 2 * 256 + 256               # four float planes, two byte planes, one tile's partials
    n, tiles = 295 * 375 * 1242, 24 * 39
    assert DCP.workspace_bytes(295, 375, 1242) == 4 * ((4 * n + 255) // 256 * 256) + 2 * ((n + 255) // 256 * 256) + (295 * tiles * 16 + 255) // 256 * 256
    assert DCP.workspace_bytes(65535, 8, 32) > 0 and DCP.workspace_bytes(1, 1 << 14, 1 << 14) > 0
    for args, text in (((0, 4, 4), 'n_frames = 0, expected 1 .. 65535'), ((65536, 4, 4), 'n_frames = 65536'),
                       ((1, 0, 4), 'a frame has at least one pixel'), ((1, 4, -1), 'a frame has at least one pixel'),
                       ((1, (1 << 14) + 1, 1 << 14), 'exceeds 2\\^28 pixels per frame')):
        with pytest.raises(DCP.DepthCompError, match=text):
            DCP.workspace_bytes(*args)


def test_binding_declares_the_headers_symbols_and_constants():
    import re
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, 'include', 'depthcomp_hip.h')).read()
    declared = set(re.findall(r'^(?:const char\*|int64_t|int) (depthcomp_\w+)\(', header, re.M))
    assert declared == set(DCP.SYMBOLS) and len(declared) == 4
    const = dict((k, v) for k, v in re.findall(r'#define DEPTHCOMP_(\w+) \(?(\d+)', header))
    assert tuple(int(const[k]) for k in ('ABI_VERSION', 'MAX_FRAMES', 'MAX_RADIUS', 'MAX_ITERS', 'MAX_POINTS', 'COLOUR_TABLE', 'ROW')) == \
        (DCP.ABI_VERSION, DCP.MAX_FRAMES, DCP.MAX_RADIUS, DCP.MAX_ITERS, DCP.MAX_POINTS, DCP.N_COLOUR, len(DCP.ROW_NAMES))
    assert DCP.N_COLOUR == R.N_COLOUR and DCP.MAX_POINTS == (2 * DCP.MAX_RADIUS + 1) ** 2
    assert [int(const['ORIGIN_' + k]) for k in ('NONE', 'OWN', 'FILLED', 'REFUSED')] == [DCP.ORIGIN_NONE, DCP.ORIGIN_OWN, DCP.ORIGIN_FILLED, DCP.ORIGIN_REFUSED] \
        == [NONE, OWN, FILLED, REFUSED]
    assert [int(const['N_' + k.upper()[2:]]) for k in DCP.ROW_NAMES] == [0, 1, 2, 3]
    assert len(DCP.SYMBOLS['depthcomp_complete'][1]) == header.split('int depthcomp_complete(')[1].split(');')[0].count(',') + 1
    assert {k: v[0] for k, v in DCP.PARAMS.items()} == {k: v for k, v in R.DEFAULTS.items() if k != 'iters'}


def test_library_argument_checks_need_no_gpu():
    import ctypes as C
    lib = DCP.lib()
    assert lib.depthcomp_abi_version() == DCP.ABI_VERSION
    buf = (C.c_double * 16384)()                                                 # host memory: every call below fails before any launch
    base = (C.addressof(buf) + 255) // 256 * 256
    at = lambda k: C.c_void_p(base + 4096 * k)

    def call(F=1, H=2, W=2, depth=at(0), rgb=at(1), std=None, ws_=at(2), wc=at(3), radius=2, iters=3, points=2, conf_min=0.02, spread=0.1,
             decay=0.5, ws=at(10), out=at(5), std_out=at(6), conf=None, origin=at(7), pas=None, rows=None):
        return lib.depthcomp_complete(None, F, H, W, depth, rgb, std, ws_, wc, radius, iters, points, conf_min, spread, decay, ws, out, std_out,
                                      conf, origin, pas, rows)
    for kw, text in ((dict(F=0), 'n_frames = 0'), (dict(radius=0), 'radius = 0, expected 1 .. 8'), (dict(radius=9), 'radius = 9'),
                     (dict(iters=0), 'iters = 0, expected 1 .. 16'), (dict(iters=17), 'iters = 17'), (dict(points=0), 'min_points = 0, expected 1 .. 289'),
                     (dict(points=290), 'min_points = 290'), (dict(conf_min=1.5), 'min_conf = 1.5'), (dict(conf_min=float('nan')), 'min_conf = nan'),
                     (dict(spread=-1.0), 'max_rel_spread = -1'), (dict(spread=float('nan')), 'max_rel_spread = nan'), (dict(decay=0.0), 'decay = 0'),
                     (dict(decay=1.25), 'decay = 1.25'), (dict(depth=None), 'non-null depth, rgb, w_space, w_colour, workspace'),
                     (dict(wc=None), 'non-null depth, rgb, w_space, w_colour, workspace'), (dict(origin=None), 'non-null depth_out, std_out, origin'),
                     (dict(out=at(0)), 'depth_out overlaps depth'), (dict(std_out=at(1)), 'std_out overlaps rgb'),
                     (dict(std=at(4), conf=at(4)), 'conf overlaps std_in'), (dict(origin=C.c_void_p(base + 4096 * 2 + 100)), 'origin overlaps w_space'),
                     (dict(pas=C.c_void_p(base + 4096 * 3 + 6000)), 'pass overlaps w_colour'), (dict(rows=at(0)), 'rows overlaps depth'),
                     (dict(ws=at(0)), 'workspace overlaps depth'), (dict(conf=at(5)), 'depth_out overlaps conf'), (dict(pas=at(7)), 'origin overlaps pass'),
                     (dict(out=at(10)), 'depth_out overlaps workspace'), (dict(ws=C.c_void_p(base + 4096 * 10 + 8)), 'workspace aligned to 256 bytes'),
                     (dict(out=C.c_void_p(base + 4096 * 5 + 1)), 'aligned to 4 bytes'), (dict(ws_=C.c_void_p(base + 4096 * 2 + 4)), 'aligned to 8 bytes')):
        assert call(**kw) == 1, kw
        assert text in DCP.last_error(), (kw, DCP.last_error())
    assert call(spread=float('inf'), F=0) == 1 and 'n_frames' in DCP.last_error()


# ------------------------------------------------------------------------------------------------ 4. PNG encoding and the report
def test_png_encoding_round_trip(tmp_path):
    from PIL import Image
    raw = np.array([[0, 1, 2, 1536], [65535, 0, 7, 0]], np.uint16)
    filled = np.array([[1, 0, 0, 0], [0, 1, 1, 1]], bool)
    metres = np.array([[6.0, 9.0, 9.0, 9.0], [9.0, 0.001, 10.009765625, 300.0]])
    enc = DCP.encode_prior(raw, metres, filled)
    assert enc.dtype == np.uint16
    np.testing.assert_array_equal(enc, [[1536, 1, 2, 1536], [65535, 2, 2562, 65535]])            # own raw values kept; half to even; clamp
    DCP._write_png16(str(tmp_path / 'p.png'), enc)
    np.testing.assert_array_equal(np.asarray(Image.open(str(tmp_path / 'p.png'))), enc)
    assert ((D.convert_depth(enc) > 0) == (filled | (raw >= 2))).all()                          # what the loaders make of it
    np.testing.assert_array_equal(DCP.encode_std(np.array([0.0, 0.5, 0.001, 9.0]), np.array([1, 1, 1, 0], bool)), [2, 128, 2, 0])


def test_report_and_totals_line(tmp_path):
    rows = np.array([[2, 2, 1, 1], [1, 1, 0, 4]])
    origin = np.array([[[1, 1, 2, 2, 3, 0]], [[1, 2, 0, 0, 0, 0]]], np.uint8)
    out = np.array([[[1.0, 2.0, 2.2, 4.0, 0.0, 0.0]], [[4.0, 3.0, 0.0, 0.0, 0.0, 0.0]]], np.float32)
    gt = np.array([[[1.0, 2.0, 2.0, 4.0, 5.0, 1.0]], [[4.0, 2.0, 1.0, 1.0, 1.0, 0.0]]], np.float32)
    DCP.write_report(str(tmp_path / 'r.txt'), ['a.png', 'b.png'], rows, origin, out, gt)
    lines = (tmp_path / 'r.txt').read_text().splitlines()
    assert lines[0].split() == ['#', 'frame', 'n_own', 'n_filled', 'n_refused', 'n_none', 'coverage_before', 'coverage_after', 'absrel_filled']
    a, tot = lines[1].split(), lines[-1].split()
    assert a[:5] == ['a.png', '2', '2', '1', '1'] and tot[:5] == ['total', '3', '3', '1', '5']
    assert (float(a[5]), float(a[6])) == (round(2 / 6, 6), round(4 / 6, 6)) and (float(tot[5]), float(tot[6])) == (0.25, 0.5)
    assert abs(float(a[7]) - 0.05) < 1e-6 and abs(float(lines[2].split()[7]) - 0.5) < 1e-6 and abs(float(tot[7]) - 0.2) < 1e-6
    DCP.write_report(str(tmp_path / 'n.txt'), ['a.png', 'b.png'], rows, origin)
    assert (tmp_path / 'n.txt').read_text().splitlines()[-1] == 'total 3 3 1 5 0.250000 0.500000'
    assert DCP.totals_line(rows, 3) == ('depth completion (3 passes): 2 frames, 3 own prior pixels, 3 filled, 1 refused, 5 left empty '
                                        '(coverage 25.0 % -> 50.0 %)')


def test_cli_files_of_a_scene_with_a_guide_that_follows_the_surfaces(tmp_path):
    """the PNG and report writers on the reference's own output for a small scene on disk (the device call is the GPU test's)"""
    from PIL import Image
    shape = SHAPES[0]
    true, rgb, prior = analytic_scene(shape, box=True)['depth'], guide_of(shape), prior_of('sparse', shape)
    raw = np.round(prior.astype(np.float64) * 256.0).astype(np.uint16)
    sup = (raw.astype(np.float32) / 256.0).astype(np.float32)
    ws, wc = R.tables(4, 2.0, 20.0)
    ref = R.complete(sup, rgb, None, ws, wc, 4, 3)
    filled = ref['origin'] == FILLED
    names = ['f%02d.png' % i for i in range(shape[0])]
    for i, name in enumerate(names):
        DCP._write_png16(str(tmp_path / name), DCP.encode_prior(raw[i], ref['depth'][i], filled[i]))
        DCP._write_png16(str(tmp_path / ('std_' + name)), DCP.encode_std(ref['std'][i], ref['conf'][i] > 0))
    back = np.stack([np.asarray(Image.open(str(tmp_path / n))) for n in names], 0)
    np.testing.assert_array_equal(back[~filled], raw[~filled])
    assert (back[filled] >= 2).all() and np.abs(back[filled] / 256.0 - ref['depth'][filled]).max() <= 0.5 / 256 + 1e-6
    std = np.stack([np.asarray(Image.open(str(tmp_path / ('std_' + n)))) for n in names], 0)
    assert ((std >= 2) == (ref['conf'] > 0)).all()
    DCP.write_report(str(tmp_path / 'complete_lidar.txt'), names, ref['rows'], ref['origin'], ref['depth'], true)
    tot = (tmp_path / 'complete_lidar.txt').read_text().splitlines()[-1].split()
    assert tot[:5] == ['total'] + [str(v) for v in ref['rows'].sum(0)]
    print('coverage %s -> %s, AbsRel of the filled %s' % tuple(tot[5:]))
    assert float(tot[6]) > 5 * float(tot[5]) and float(tot[7]) < 0.05


# ------------------------------------------------------------------------------------------------ 5. both flag surfaces
def test_mip360_config_keys_parse(tmp_path):
    cfg = D.parse_gin(bindings=[])
    assert cfg['depth_comp_iters'] == 0 and cfg['depth_comp_std_floor'] == 0.0
    assert DCP.check_params(**dict(DCP.scene_params(cfg), iters=3)) == dict(R.DEFAULTS, std_floor=0.0)
    cfg = D.parse_gin(bindings=['Config.depth_comp_iters = 5', 'Config.depth_comp_radius = 6', 'Config.depth_comp_sigma_colour = 12.5',
                                'Config.depth_comp_min_points = 3', 'Config.depth_comp_std_floor = 0.5'])
    assert DCP.scene_params(cfg, 0.1) == dict(R.DEFAULTS, iters=5, radius=6, sigma_colour=12.5, min_points=3, std_floor=0.05)
    from tests.test_depth_consistency import write_colmap_scene
    write_colmap_scene(str(tmp_path), F=10, H=8, W=10)
    base = ["Config.data_dir = '%s'" % tmp_path, "Config.depth_sup_type = 'noisy'"]
    s = D.Scene(D.parse_gin(bindings=base + ['Config.depth_comp_iters = 16']))
    assert s.depth_comp_iters == 16 and s.depth_comp_prm['iters'] == 16 and s.depth_acc_views == 0
    assert D.Scene(D.parse_gin(bindings=base)).depth_comp_iters == 0
    for extra, text in ((['Config.depth_comp_iters = 17'], r'Config.depth_comp_iters = 17: expected 0 \(off\) .. 16'),
                        (['Config.depth_comp_iters = 2', 'Config.depth_comp_radius = 9'], r'Config.depth_comp_\*: radius = 9'),
                        (['Config.depth_comp_iters = 2', 'Config.depth_comp_decay = 0.0'], r'Config.depth_comp_\*: decay = 0.0')):
        with pytest.raises(D.ConfigError, match=text):
            D.Scene(D.parse_gin(bindings=base + extra))
    # a gnll run without another source takes its standard deviation from the completion
    g = D.Scene(D.parse_gin(bindings=base + ["Config.depth_loss_type = 'gnll'", 'Config.depth_comp_iters = 2']))
    assert g.depth_std_source == 'completion'
    g = D.Scene(D.parse_gin(bindings=base + ["Config.depth_loss_type = 'gnll'", 'Config.depth_comp_iters = 2', 'Config.depth_gnll_std = 0.1']))
    assert g.depth_std_source == 'constant'


def test_nerfpp_flags_parse():
    pytest.importorskip('torch')
    from outdoor_nerf_depth_amd import ddp_train_nerf as T_
    base = ['--expname', 'x', '--synthetic']
    args = T_.config_parser().parse_args(base)
    assert args.depth_comp_iters == 0 and DCP.check_params(**dict(DCP.args_params(args), iters=3)) == dict(R.DEFAULTS, std_floor=0.0)
    args = T_.config_parser().parse_args(base + ['--depth_comp_iters', '4', '--depth_comp_radius', '3', '--depth_comp_max_rel_spread', 'inf',
                                                 '--depth_comp_std_floor', '0.5'])
    assert DCP.args_params(args, 0.1) == dict(R.DEFAULTS, iters=4, radius=3, max_rel_spread=float('inf'), std_floor=0.05)
    cli = DCP.make_parser().parse_args(['--data_dir', 'd', '--depth_sup_type', 'lidar', '--radius', '2', '--iters', '6', '--gin_bindings', 'Config.factor = 2'])
    assert cli.iters == 6 and DCP.args_params(cli, 1.0, '')['radius'] == 2 and cli.gin_bindings == ['Config.factor = 2']
    assert DCP.make_parser().parse_args(['--data_dir', 'd', '--depth_sup_type', 'lidar']).iters == 3
    T_.validate_args(T_.config_parser().parse_args(base + ['--use_depth', '--depth_comp_iters', '16']))
    for bad, text in ((['--use_depth', '--depth_comp_iters', '17'], r'--depth_comp_iters = 17: expected 0 \(off\) .. 16'),
                      (['--use_depth', '--depth_comp_iters', '-1'], '--depth_comp_iters = -1'), (['--depth_comp_iters', '4'], 'it needs --use_depth'),
                      (['--use_depth', '--depth_comp_iters', '2', '--depth_comp_radius', '0'], r'--depth_comp_\*: radius = 0')):
        with pytest.raises(SystemExit, match=text):
            T_.validate_args(T_.config_parser().parse_args(base + bad))
    for bad in (['--radius', '9'], ['--iters', '0'], ['--decay', '2']):
        with pytest.raises(SystemExit, match='expected'):
            DCP.main(['--data_dir', 'd', '--depth_sup_type', 'lidar'] + bad)

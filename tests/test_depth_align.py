"""No GPU: aligning relative depth priors to sparse metric depth -- the properties of the reference
(tests/depth_align_reference.py), the tolerance of the GPU gate, the host side of outdoor_nerf_depth_amd/depth_align.py (argument
checks, PNG encoding, the report), the library's argument checks and both flag surfaces.

The GPU gate (tests/test_gpu_depth_align.py) compares s, b, sigma and rms to rtol 1e-9 and the inlier count exactly.  What justifies
that is asserted here on the inputs that test uses (CASES): the fit in float64 in sequential order, in a random permutation and in
longdouble agrees to 1e-11 -- the device's sums differ from numpy's in order alone -- and no residual lies within 1e-6 (relative)
of the 3 sigma inlier bound, so a difference of 1e-9 in the row cannot move a count.
"""
import os

import numpy as np
import pytest

from outdoor_nerf_depth_amd import depth_align as DAL
from outdoor_nerf_depth_amd import mip360_data as D
from tests import depth_align_reference as R

DENSE = -1
# (F, H, W), the pair count of every frame (DENSE: every pixel), seed.  The shapes and counts are the smallest at which each part can go
# wrong: a frame smaller than a wave; several frames in one 2048-pixel tile; a frame of 4120 pixels that crosses a tile with a ragged
# tail and an odd row length, so that 16-byte accesses meet misaligned frame bases; pair counts around min_points and the wave size.
CASES = {
    'tiny': ((1, 7, 13), (64,), 11),
    'tiny_dense': ((1, 7, 13), (DENSE,), 12),
    'few': ((3, 37, 53), (0, 1, 15), 13),
    'wave': ((3, 37, 53), (16, 63, 64), 14),
    'waves': ((3, 37, 53), (65, 255, 256), 15),
    'tile': ((5, 40, 103), (257, 16, 3000, 65, DENSE), 16),
}
_inputs, _refs = {}, {}


def make_frame(rs, H, W, n_pairs, space, outliers=0.3, invalids=True):
    """(prior, anchor, true depth) float32 [H, W]: a random depth map, the prior distorted by a random (alpha, beta) with 0.2 % noise,
    the anchor at n_pairs pixels with 0.2 % noise and `outliers` of them multiplied by 1.3 .. 2.5; a tenth of the other pixels each
    0, negative and NaN in the prior and in the anchor"""
    n = H * W
    z = rs.uniform(2.0, 60.0, n)
    alpha, beta = rs.uniform(0.5, 3.0), rs.uniform(0.0, 0.5)
    if space == 'disparity':
        p = ((1.0 / z) * (1 + 0.002 * rs.randn(n)) + beta * 0.01) / alpha
    else:
        p = (z * (1 + 0.002 * rs.randn(n)) + beta) / alpha
    pick = rs.permutation(n)[:n if n_pairs == DENSE else n_pairs]
    a = np.zeros(n)
    a[pick] = z[pick] * (1 + 0.002 * rs.randn(len(pick)))
    bad = pick[rs.rand(len(pick)) < outliers]
    a[bad] *= rs.uniform(1.3, 2.5, len(bad))
    p, a = p.astype(np.float32), a.astype(np.float32)
    if invalids:
        rest = np.setdiff1d(np.arange(n), pick)
        u = rs.rand(len(rest))
        for arr, lo in ((p, 0.0), (a, 0.3)):
            arr[rest[(u >= lo) & (u < lo + 0.1)]] = 0.0
            arr[rest[(u >= lo + 0.1) & (u < lo + 0.2)]] = -1.5
            arr[rest[(u >= lo + 0.2) & (u < lo + 0.3)]] = np.nan
    return p.reshape(H, W), a.reshape(H, W), z.astype(np.float32).reshape(H, W)


def inputs(case, space):
    """(prior, anchor, true) float32 [F, H, W] of CASES[case] in `space`, built once and shared (read-only)"""
    if (case, space) not in _inputs:
        (F, H, W), counts, seed = CASES[case]
        rs = np.random.RandomState(seed + (100 if space == 'disparity' else 0))
        arrs = [np.stack(x, 0) for x in zip(*[make_frame(rs, H, W, counts[f], space) for f in range(F)])]
        for a in arrs:
            a.setflags(write=False)
        _inputs[case, space] = tuple(arrs)
    return _inputs[case, space]


def reference(case, space, **params):
    """The reference's outputs for inputs(case, space), computed once and shared (read-only)"""
    key = (case, space, tuple(sorted(params.items())))
    if key not in _refs:
        p, a, _ = inputs(case, space)
        _refs[key] = R.align(p, a, space=space, **params)
        for v in _refs[key].values():
            v.setflags(write=False)
    return _refs[key]


def statuses_batch(space='depth'):
    """(prior, anchor) float32 [4, 12, 20]: one frame of each status 0, 1, 2, 3 in one batch"""
    rs = np.random.RandomState(21)
    frames = [make_frame(rs, 12, 20, n, space, invalids=False)[:2] for n in (100, 15, 100, 100)]
    p, a = [np.stack(x, 0).copy() for x in zip(*frames)]
    p[2] = 3.0                                                                   # a constant prior: degenerate
    p[3] = np.float32(100.0) - p[3] if space == 'depth' else np.float32(p[3].max() * 1.5) - p[3]      # an inverted prior: s < 0
    return p, a


def absrel(out, true, mask):
    return float(np.mean(np.abs(out[mask].astype(np.float64) - true[mask]) / true[mask]))


# ------------------------------------------------------------------------------------------------ 1. the reference's properties
@pytest.mark.parametrize('space', R.SPACES)
def test_exact_data_is_recovered_with_sigma_zero_and_an_early_end(space):
    if space == 'depth':                                                         # dyadic values: every product and sum is exact
        x = (0.5 + np.arange(64) / 16.0).astype(np.float32)
        a, s, b = 2.0 * x + 1.0, 2.0, 1.0
    else:                                                                        # t = 1 / a = 1, 2, 4, 8 = 2 x - 1
        a = np.array([1.0, 0.5, 0.25, 0.125] * 16, np.float32)
        x, s, b = np.array([1.0, 1.5, 2.5, 4.5] * 16, np.float32), 2.0, -1.0
    row = R.fit(*R.pairs(x, a, space))
    assert row.tolist() == [s, b, 0.0, 64.0, 64.0, 0.0, 1.0, 0.0]                # one solve, then the exact fit ends the loop
    got = R.align(x.reshape(1, 8, 8), a.reshape(1, 8, 8), space=space)
    np.testing.assert_array_equal(got['depth_out'].reshape(-1), a)
    assert not got['std_out'].any()


def _z64(x, row, space):
    v = row[0] * x + row[1]
    return 1.0 / v if space == 'disparity' else v


@pytest.mark.parametrize('space', R.SPACES)
def test_invariance_to_the_priors_scale_and_shift(space):
    p, a, _ = inputs('waves', space)
    worst = 0.0
    for f in range(p.shape[0]):
        x, t = R.pairs(p[f], a[f], space)
        every = p[f][p[f] > 0].astype(np.float64)
        base = _z64(every, R.fit(x, t), space)
        # The normal equations lose log10(1 + mean^2 / var) digits of x to cancellation, so the (alpha, beta) tried keep that figure
        # within a factor of four of the data's own (3 .. 5 here): a shift of many spreads is a different, ill-conditioned problem.
        for alpha, beta in ((4.0, 0.0), (0.3, 0.0), (1.7, 0.05 * x.mean()), (0.5, 0.5 * x.mean())):
            row = R.fit(alpha * x + beta, t)
            assert row[5] == 0
            moved = np.abs(_z64(alpha * every + beta, row, space) / base - 1.0).max()
            worst = max(worst, moved)
    print('%s: aligning alpha p + beta moves depth_out by at most %.2g (relative)' % (space, worst))
    assert worst <= 1e-12


@pytest.mark.parametrize('space', R.SPACES)
@pytest.mark.parametrize('share', (0.25, 0.40))
def test_gross_outliers_are_resisted_where_least_squares_is_not(space, share):
    rs = np.random.RandomState(5)
    p, a, z = make_frame(rs, 50, 60, 3000, space, outliers=share, invalids=False)
    robust = R.align(p[None], a[None], space=space)
    plain = R.align(p[None], a[None], space=space, iters=0)
    e_r, e_p = absrel(robust['depth_out'][0], z, robust['depth_out'][0] > 0), absrel(plain['depth_out'][0], z, plain['depth_out'][0] > 0)
    print('%s, %d %% outliers: AbsRel %.4f robust (%d solves), %.4f least squares' % (space, 100 * share, e_r, robust['rows'][0, 6], e_p))
    assert robust['rows'][0, 5] == 0 and plain['rows'][0, 6] == 1
    assert e_r < 0.005 and e_p > 0.05


def test_statuses_and_the_min_points_boundary():
    p, a = statuses_batch()
    got = R.align(p, a)
    assert got['rows'][:, 5].tolist() == [0, 1, 2, 3] and got['rows'][:, 3].tolist() == [100, 15, 100, 100]
    assert (got['rows'][1:, [0, 1, 2, 4, 7]] == 0).all() and not got['depth_out'][1:].any() and not got['std_out'][1:].any()
    assert got['rows'][0, 0] > 0 and got['rows'][0, 4] <= 100 and got['rows'][0, 6] == 11
    assert R.align(p[1:2], a[1:2], min_points=15)['rows'][0, 5] == 0              # n_pairs = min_points is fitted
    assert R.align(p[:1], a[:1], min_points=101)['rows'][0, 5] == 1               # n_pairs = min_points - 1 is not
    assert R.align(*statuses_batch('disparity'), space='disparity')['rows'][:, 5].tolist() == [0, 1, 2, 3]
    kept = R.align(p, a, keep_anchor=True, std_floor=0.25)                        # frames that are not fitted give the anchor
    own = a > 0
    np.testing.assert_array_equal(kept['depth_out'][own].view(np.int32), a[own].view(np.int32))
    assert not kept['depth_out'][1:][~own[1:]].any() and (kept['std_out'][own] == 0.25).all()
    assert (kept['std_out'][0][~own[0]] >= 0.25).all() and not kept['std_out'][1:][~own[1:]].any()


def test_apply_step_drops_what_it_must_and_std_has_two_forms():
    p = np.array([[[1.0, 2.0, 4.0, 0.0, -1.0, np.nan, 0.5, 8.0]]], np.float32)
    a = np.zeros_like(p)
    a[0, 0, 1] = 7.0
    rows = np.array([[0.5, -0.5, 0.1, 16, 16, 0, 3, 0.1]])                        # v = 0, 0.5, 1.5, ., ., ., -0.25, 3.5
    d, s = R.apply(p, a, rows, 'disparity')
    np.testing.assert_array_equal(d[0, 0], np.array([0, 2.0, 1 / 1.5, 0, 0, 0, 0, 1 / 3.5], np.float32))     # v <= 0 and invalid p are dropped
    np.testing.assert_array_equal(s[0, 0], np.array([0, (0.1 * 2.0) * 2.0, (0.1 * (1 / 1.5)) * (1 / 1.5), 0, 0, 0, 0, (0.1 * (1 / 3.5)) * (1 / 3.5)], np.float32))
    d, s = R.apply(p, a, rows, 'disparity', max_depth=1.0)
    np.testing.assert_array_equal(d[0, 0] > 0, [0, 0, 1, 0, 0, 0, 0, 1])          # z = 2 > max_depth is dropped
    d, s = R.apply(p, a, rows, 'depth', std_floor=0.25)
    np.testing.assert_array_equal(d[0, 0], np.array([0, 0.5, 1.5, 0, 0, 0, 0, 3.5], np.float32))
    np.testing.assert_array_equal(s[0, 0], np.array([0, 0.25, 0.25, 0, 0, 0, 0, 0.25], np.float32))
    d, s = R.apply(p, a, rows, 'depth')
    np.testing.assert_array_equal(s[0, 0], np.where(d[0, 0] > 0, np.float32(0.1), 0))
    d, s = R.apply(p, a, rows, 'depth', keep_anchor=True, std_floor=0.05)
    assert d[0, 0, 1] == 7.0 and s[0, 0, 1] == np.float32(0.05) and d[0, 0, 2] == 1.5 and s[0, 0, 2] == np.float32(0.1)


# ------------------------------------------------------------------------------------------------ 2. the tolerance of the GPU gate
def _frames_of(case, space, min_points=16):
    p, a = statuses_batch(space) if case == 'statuses' else inputs(case, space)[:2]
    for f in range(1 if case == 'statuses' else p.shape[0]):
        x, t = R.pairs(p[f], a[f], space)
        if len(x) >= min_points:
            yield f, x, t


@pytest.mark.parametrize('space', R.SPACES)
@pytest.mark.parametrize('case', sorted(CASES) + ['statuses'])
def test_order_sensitivity_and_near_ties_of_the_gpu_tests_inputs(case, space):
    rs = np.random.RandomState(3)
    for iters, c, min_points in ((0, 1.0, 16), (10, 1.0, 16), (3, 2.0, 2)):          # the parameter sets the GPU tests run
        for f, x, t in _frames_of(case, space, min_points):
            base = R.fit(x, t, iters=iters, c=c, min_points=min_points)
            assert base[5] == 0, (case, f)
            perm = rs.permutation(len(x))
            seq = _fit_sequential(x, t, iters, c, min_points)
            wide = R.fit(x.astype(np.longdouble), t.astype(np.longdouble), iters=iters, c=c, min_points=min_points, dtype=np.longdouble).astype(np.float64)
            scale = np.array([abs(base[0]), abs(base[1]) + abs(base[0]) * x.max(), base[2]])
            worst = max((np.abs(other[:3] - base[:3]) / scale).max() for other in (R.fit(x[perm], t[perm], iters=iters, c=c, min_points=min_points), seq, wide))
            r = np.abs((base[0] * x + base[1]) - t)
            margin = np.abs(r - 3 * base[2]).min() / (3 * base[2])
            print('%s %s frame %d, n = %d, K = %d: order sensitivity %.2g, 3 sigma near-tie margin %.2g' % (case, space, f, len(x), iters, worst, margin))
            assert worst <= 1e-11 and margin > 1e-6
            assert (seq[3:7] == base[3:7]).all() and (wide[3:7] == base[3:7]).all()


def _fit_sequential(x, t, iters, c, min_points):
    """R.fit with every sum a left-to-right loop"""
    keep = np.sum
    try:
        np.sum = lambda v: float(__import__('functools').reduce(lambda s, e: s + e, v.tolist(), 0.0)) if v.dtype == np.float64 else keep(v)
        return R.fit(x, t, iters=iters, c=c, min_points=min_points)
    finally:
        np.sum = keep


# ------------------------------------------------------------------------------------------------ 3. argument errors, no device
def test_host_checks_name_the_argument():
    assert DAL.check_params() == dict(R.DEFAULTS)
    assert DAL.ROW_NAMES == R.ROW_NAMES and DAL.SPACES == R.SPACES
    assert DAL.check_params(iters=0, c=0.5, min_points=2, max_depth=80.0, keep_anchor=True, space='disparity')['iters'] == 0
    for kw, text in ((dict(space='log'), "space = 'log': expected one of depth, disparity"), (dict(iters=33), 'iters = 33: expected an integer 0 .. 32'),
                     (dict(iters=-1), 'iters = -1'), (dict(iters=1.5), 'iters = 1.5'), (dict(c=0.0), 'c = 0.0: expected a finite number > 0'),
                     (dict(c=float('inf')), 'c = inf'), (dict(c=float('nan')), 'c = nan'), (dict(min_points=1), 'min_points = 1: expected an integer >= 2'),
                     (dict(max_depth=0.0), 'max_depth = 0.0'), (dict(max_depth=float('nan')), 'max_depth = nan'),
                     (dict(std_floor=-1.0), 'std_floor = -1.0'), (dict(std_floor=float('inf')), 'std_floor = inf')):
        with pytest.raises(DAL.DepthAlignError, match=text):
            DAL.check_params(**kw)
    with pytest.raises(DAL.DepthAlignError, match="--anchor_sup_type = 'mono' is the prior itself"):
        DAL.check_anchor('mono', 'mono', '--anchor_sup_type')
    assert DAL.check_anchor('lidar', 'mono', 'x') == 'lidar' and DAL.check_anchor(None, 'mono', 'x') == ''


def test_tensor_checks_name_the_tensor_before_the_device_is_asked():
    torch = pytest.importorskip('torch')
    prior = torch.zeros(2, 6, 8)
    for bad in (prior, np.zeros((2, 6, 8), np.float32)):
        with pytest.raises(DAL.DepthAlignError, match='prior: expected a CUDA/HIP float32 tensor'):
            DAL.align_async(bad, prior)
    with pytest.raises(DAL.DepthAlignError, match='anchor: expected a CUDA/HIP float32 tensor'):
        DAL.align_async(prior, None)
    for bad, text in ((prior.double(), r'prior: expected torch.float32, got torch.float64'), (prior[0], r'prior: expected \[F, H, W\]'),
                      (prior[:, :, ::2], 'prior: expected a contiguous tensor')):
        with pytest.raises(DAL.DepthAlignError, match=text):
            DAL.align_async(bad, prior)
    with pytest.raises(DAL.DepthAlignError, match=r'prior \(2, 6, 8\) and anchor \(1, 6, 8\) differ in shape'):
        DAL.align_async(prior, prior[:1])
    with pytest.raises(DAL.DepthAlignError, match='anchor: expected torch.float32'):
        DAL.align_async(prior, prior.int())


# --------------------------------------------------------------------------------------------------- 4. the library, no GPU
def test_workspace_bytes_limits():
    up = lambda n: (n + 255) // 256 * 256
    assert DAL.workspace_bytes(1, 1, 1) == 5 * 256
    tiles = (375 * 1242 + 2047) // 2048
    assert DAL.workspace_bytes(295, 375, 1242) == up(295 * 375 * 1242 * 8) + up(295 * 375 * 1242 * 4) + 2 * up(295 * tiles * 4) + up(295 * 4)
    assert DAL.workspace_bytes(65535, 8, 32) > 0 and DAL.workspace_bytes(1, 1 << 14, 1 << 14) > 0
    for args, text in (((0, 4, 4), 'n_frames = 0, expected 1 .. 65535'), ((65536, 4, 4), 'n_frames = 65536'),
                       ((1, 0, 4), 'a frame has at least one pixel'), ((1, 4, -1), 'a frame has at least one pixel'),
                       ((1, (1 << 14) + 1, 1 << 14), 'exceeds 2\\^28 pixels per frame')):
        with pytest.raises(DAL.DepthAlignError, match=text):
            DAL.workspace_bytes(*args)


def test_binding_declares_the_headers_symbols_and_constants():
    import re
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, 'include', 'depthalign_hip.h')).read()
    declared = set(re.findall(r'^(?:const char\*|int64_t|int) (depthalign_\w+)\(', header, re.M))
    assert declared == set(DAL.SYMBOLS) and len(declared) == 4
    const = dict((k, v) for k, v in re.findall(r'#define DEPTHALIGN_(\w+) \(?(\d+)', header))
    assert (int(const['ABI_VERSION']), int(const['MAX_FRAMES']), int(const['MAX_ITERS']), int(const['ROW'])) \
        == (DAL.ABI_VERSION, DAL.MAX_FRAMES, DAL.MAX_ITERS, len(DAL.ROW_NAMES))
    assert [int(const['ROW_' + k.upper()]) for k in DAL.ROW_NAMES] == list(range(8))
    assert [int(const['SPACE_' + k.upper()]) for k in DAL.SPACES] == [0, 1]
    assert [int(const['STATUS_' + k]) for k in ('FITTED', 'FEW', 'DEGENERATE', 'INVERTED')] \
        == [DAL.STATUS_FITTED, DAL.STATUS_FEW, DAL.STATUS_DEGENERATE, DAL.STATUS_INVERTED] \
        == [R.STATUS_FITTED, R.STATUS_FEW, R.STATUS_DEGENERATE, R.STATUS_INVERTED]
    assert len(DAL.SYMBOLS['depthalign_fit_apply'][1]) == header.split('int depthalign_fit_apply(')[1].split(');')[0].count(',') + 1
    assert '%.16g' % R.GAUSS in header and R.GAUSS == float(np.sqrt(np.pi / 2))


def test_library_argument_checks_need_no_gpu():
    import ctypes as C
    lib = DAL.lib()
    assert lib.depthalign_abi_version() == DAL.ABI_VERSION
    buf = (C.c_double * 8192)()                                                  # host memory: every call below fails before any launch
    base = (C.addressof(buf) + 255) // 256 * 256
    at = lambda off: C.c_void_p(base + off)
    p, a, out, std, rows, ws = at(0), at(4096), at(8192), at(12288), at(16384), at(20480)

    def call(F=1, H=2, W=2, prior=p, anchor=a, space=0, iters=10, c=1.0, min_points=16, max_depth=float('inf'), keep=0, floor=0.0, ws=ws,
             out=out, std=std, rows=rows):
        return lib.depthalign_fit_apply(None, F, H, W, prior, anchor, space, iters, c, min_points, max_depth, keep, floor, ws, out, std, rows)
    for kw, text in ((dict(F=0), 'n_frames = 0'), (dict(H=0), 'a frame has at least one pixel'), (dict(space=2), 'space = 2, expected 0 (depth) or 1 (disparity)'),
                     (dict(iters=33), 'iters = 33, expected 0 .. 32'), (dict(iters=-1), 'iters = -1'), (dict(c=0.0), 'c = 0'),
                     (dict(c=float('nan')), 'c = nan'), (dict(c=float('inf')), 'c = inf'), (dict(min_points=1), 'min_points = 1, expected at least 2'),
                     (dict(max_depth=0.0), 'max_depth = 0'), (dict(max_depth=float('nan')), 'max_depth = nan'), (dict(keep=2), 'keep_anchor = 2'),
                     (dict(floor=-1.0), 'std_floor = -1'), (dict(floor=float('inf')), 'std_floor = inf'),
                     (dict(prior=None), 'non-null prior, anchor, depth_out, rows, workspace'), (dict(rows=None), 'non-null prior'),
                     (dict(ws=None), 'non-null prior'), (dict(out=p), 'depth_out overlaps prior'), (dict(out=at(4096 + 12)), 'depth_out overlaps anchor'),
                     (dict(std=at(8)), 'std_out overlaps prior'), (dict(std=out), 'std_out overlaps depth_out'), (dict(rows=at(4096 + 8)), 'rows overlaps anchor'),
                     (dict(ws=p), 'workspace overlaps prior'), (dict(ws=at(8192)), 'workspace overlaps depth_out'),
                     (dict(ws=at(20480 + 8)), 'workspace aligned to 256 bytes'), (dict(out=at(8193)), 'aligned to 4 bytes'),
                     (dict(rows=at(16388)), 'rows aligned to 8 bytes')):
        assert call(**kw) == 1, kw
        assert text in DAL.last_error(), (kw, DAL.last_error())


# ----------------------------------------------------------------------------------------------------- 5. PNG encoding, the report
def test_png_encoding_round_trip(tmp_path):
    from PIL import Image
    metres = np.array([[6.0, 0.001, 10.009765625, 300.0], [9.0, np.inf, 0.0, 7.0]])
    valid = np.array([[1, 1, 1, 1], [0, 1, 0, 1]], bool)
    enc = DAL.encode_depth(metres, valid)
    assert enc.dtype == np.uint16
    np.testing.assert_array_equal(enc, [[1536, 2, 2562, 65535], [0, 65535, 0, 1792]])               # half to even; clamped to [2, 65535]; 0 where invalid
    DAL._write_png16(str(tmp_path / 'p.png'), enc)
    np.testing.assert_array_equal(np.asarray(Image.open(str(tmp_path / 'p.png'))), enc)
    back = D.convert_depth(enc)
    assert ((back > 0) == valid).all() and abs(back[0, 0] - 6.0) <= 0.5 / 256 and abs(back[0, 2] - 10.009765625) <= 0.5 / 256


def test_report_and_totals_line(tmp_path):
    rows = np.array([[2.0, 0.5, 0.125, 40, 36, 0, 11, 0.25], [0, 0, 0, 3, 0, 1, 0, 0], [0, 0, 0, 50, 0, 3, 11, 0]])
    prior = np.array([[[1.0, 2.0]], [[1.0, 0.0]], [[1.0, 1.0]]], np.float32)
    out = np.array([[[2.5, 4.5]], [[0.0, 0.0]], [[0.0, 0.0]]], np.float32)
    gt = np.array([[[2.0, 5.0]], [[1.0, 1.0]], [[1.0, 1.0]]], np.float32)
    DAL.write_report(str(tmp_path / 'r.txt'), ['a.png', 'b.png', 'c.png'], rows, prior, out, gt)
    lines = (tmp_path / 'r.txt').read_text().splitlines()
    assert lines[0].split() == ['#', 'frame'] + list(DAL.ROW_NAMES) + ['absrel_before', 'absrel_after']
    a = lines[1].split()
    assert a[:9] == ['a.png', '2', '0.5', '0.125', '40', '36', '0', '11', '0.25']
    assert abs(float(a[9]) - (0.5 + 0.6) / 2) < 1e-6 and abs(float(a[10]) - (0.25 + 0.1) / 2) < 1e-6
    assert lines[2].split()[1:9] == ['0', '0', '0', '3', '0', '1', '0', '0'] and lines[2].split()[10] == 'nan'
    assert lines[4].startswith('total 1 fitted of 3 ')
    assert lines[5:] == ['not fitted: b.png (too few pairs)', 'not fitted: c.png (inverted or non-finite)']
    DAL.write_report(str(tmp_path / 'n.txt'), ['a.png', 'b.png', 'c.png'], rows)
    assert (tmp_path / 'n.txt').read_text().splitlines()[4] == 'total 1 fitted of 3'
    assert DAL.totals_line(rows, 'lidar') == ('depth alignment (anchor lidar): 3 frames, 1 fitted, 1 too few pairs, 0 degenerate, 1 inverted; 40 pairs, '
                                              '90.0 % within 3 sigma, median sigma 0.125')


# ------------------------------------------------------------------------------------------------- 6. both flag surfaces
def test_mip360_config_keys_parse_and_refuse(tmp_path, monkeypatch):
    cfg = D.parse_gin(bindings=[])
    assert cfg['depth_align_anchor'] == '' and DAL.scene_params(cfg) == {k: v for k, v in R.DEFAULTS.items() if k != 'std_floor'}
    cfg = D.parse_gin(bindings=["Config.depth_align_anchor = 'lidar'", "Config.depth_align_space = 'disparity'", 'Config.depth_align_iters = 5',
                                'Config.depth_align_c = 2.0', 'Config.depth_align_min_points = 8', 'Config.depth_align_max_depth = 80.0',
                                'Config.depth_align_keep_anchor = True'])
    assert cfg['depth_align_anchor'] == 'lidar'
    assert DAL.scene_params(cfg, 0.5) == dict(space='disparity', iters=5, c=2.0, min_points=8, max_depth=40.0, keep_anchor=True)
    from tests.test_depth_consistency import write_colmap_scene
    write_colmap_scene(str(tmp_path), F=10, H=8, W=10)
    base = ["Config.data_dir = '%s'" % tmp_path, "Config.depth_sup_type = 'noisy'"]
    monkeypatch.setattr(DAL, '_lib', None)
    monkeypatch.setattr(DAL, 'LIB_PATH', str(tmp_path / 'nowhere.so'))           # no Scene loads the library, with the flag or without
    plain = D.Scene(D.parse_gin(bindings=base))
    assert plain.depth_align_anchor == '' and plain.depths_anchor is None
    s = D.Scene(D.parse_gin(bindings=base + ["Config.depth_align_anchor = 'gt'"]))
    assert s.depth_align_anchor == 'gt' and np.array_equal(s.depths_anchor, s.depths_gt) and s.depth_std_source is None
    assert s.depth_align_prm == DAL.check_params()
    g = D.Scene(D.parse_gin(bindings=base + ["Config.depth_align_anchor = 'gt'", "Config.depth_loss_type = 'gnll'", 'Config.depth_cons_views = 2']))
    assert g.depth_std_source == 'alignment'                                     # ahead of the consistency check's spread
    g = D.Scene(D.parse_gin(bindings=base + ["Config.depth_align_anchor = 'gt'", "Config.depth_loss_type = 'gnll'", 'Config.depth_gnll_std = 0.1']))
    assert g.depth_std_source == 'constant'                                      # after the constant
    for bad, text in ((["Config.depth_align_anchor = 'noisy'"], "Config.depth_align_anchor = 'noisy' is the prior itself"),
                      (["Config.depth_align_anchor = 'gt'", 'Config.depth_align_iters = 40'], 'iters = 40: expected an integer 0 .. 32'),
                      (["Config.depth_align_anchor = 'gt'", "Config.depth_align_space = 'log'"], "space = 'log'")):
        with pytest.raises(D.ConfigError, match=text):
            D.Scene(D.parse_gin(bindings=base + bad))
    with pytest.raises(ValueError, match='depths_lidar does not exist'):
        D.Scene(D.parse_gin(bindings=base + ["Config.depth_align_anchor = 'lidar'"]))
    assert DAL._lib is None


def test_nerfpp_flags_parse_and_refuse():
    pytest.importorskip('torch')
    from outdoor_nerf_depth_amd import ddp_train_nerf as T_
    base = ['--expname', 'x', '--synthetic']
    args = T_.config_parser().parse_args(base)
    assert args.depth_align_anchor == '' and DAL.args_params(args) == {k: v for k, v in R.DEFAULTS.items() if k != 'std_floor'}
    T_.validate_args(args)
    args = T_.config_parser().parse_args(base + ['--use_depth', '--depth_sup_type', 'mono_crop', '--depth_align_anchor', 'lidar', '--depth_align_space',
                                                 'disparity', '--depth_align_iters', '5', '--depth_align_c', '2', '--depth_align_min_points', '8',
                                                 '--depth_align_max_depth', '80', '--depth_align_keep_anchor'])
    assert DAL.args_params(args, 0.5) == dict(space='disparity', iters=5, c=2.0, min_points=8, max_depth=40.0, keep_anchor=True)
    T_.validate_args(args)
    cli = DAL.make_parser().parse_args(['--data_dir', 'd', '--depth_sup_type', 'mono', '--anchor_sup_type', 'lidar', '--space', 'disparity', '--iters', '4',
                                        '--std_floor', '0.5', '--keep_anchor', '--gin_bindings', 'Config.factor = 2'])
    assert DAL.args_params(cli, 2.0, '') == dict(space='disparity', iters=4, c=1.0, min_points=16, max_depth=float('inf'), keep_anchor=True, std_floor=1.0)
    assert cli.gin_bindings == ['Config.factor = 2'] and cli.anchor_sup_type == 'lidar'
    for bad, text in ((['--depth_align_anchor', 'lidar'], 'it needs --use_depth'),
                      (['--use_depth', '--depth_sup_type', 'lidar', '--depth_align_anchor', 'lidar'], 'is the prior itself'),
                      (['--use_depth', '--depth_align_anchor', 'lidar', '--depth_align_iters', '33'], 'iters = 33'),
                      (['--use_depth', '--depth_align_anchor', 'lidar', '--depth_align_c', '0'], 'c = 0.0')):
        with pytest.raises(SystemExit, match=text):
            T_.validate_args(T_.config_parser().parse_args(base + bad))


def test_samplers_of_differing_size_and_count_are_refused():
    class S(object):
        def __init__(self, H, W, sup=True):
            self.H, self.W, self.depth_sup, self.depth_std = H, W, np.ones(H * W, np.float32) if sup else None, None
    with pytest.raises(DAL.DepthAlignError, match='the frames differ in size'):
        DAL.align_samplers([S(4, 6), S(4, 8)], [S(4, 6), S(4, 6)], None)
    with pytest.raises(DAL.DepthAlignError, match='carry no depth prior to align'):
        DAL.align_samplers([S(4, 6, False)], [S(4, 6)], None)
    with pytest.raises(DAL.DepthAlignError, match='carry no anchor prior'):
        DAL.align_samplers([S(4, 6)], [S(4, 6, False)], None)
    with pytest.raises(DAL.DepthAlignError, match=r'2 frames of \(4, 6\) to align against 1 of \(4, 6\)'):
        DAL.align_samplers([S(4, 6), S(4, 6)], [S(4, 6)], None)

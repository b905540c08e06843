"""GPU: libdepthvis_hip.so against the numpy helper tests/depth_vis_reference.py.

Percentiles are held to the helper bit for bit where every partial sum of the weights is exact in float64 (weights 0 or in
[2^-8, 1] on float32's grid, N <= 2^20: 24 + 8 + 20 = 52 bits), and otherwise to the worst a different summation order can do to
the straddling bin: |dev - ref| <= (2 N u W / w_j) (x[j+1] - x[j]) + 4 u |ref|, u = 2^-53.  Min / max equal numpy's bits.  The
pictures equal the helper's bytes outside its `fragile` mask, which may hold at most 0.1 % of a frame.
"""
import numpy as np
import pytest
import torch

from tests import depth_vis_reference as R

pytestmark = pytest.mark.gpu

U53 = 2.0 ** -53
SHAPES = [(1, 1), (1, 2), (1, 63), (1, 64), (1, 65), (1, 4097), (96, 129)]
PS_SETS = [(0.5, 99.5), (0., 100.), (50.,)]
PICTURE_SHAPES = [(7, 9), (16, 16), (17, 33), (96, 129)]


def dv():
    if not torch.cuda.is_available():
        pytest.skip('needs a GPU')
    from outdoor_nerf_depth_amd import depth_vis
    return depth_vis


def T(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def exact_weights(rs, n):
    """float32 weights in [2^-8, 1]"""
    return rs.uniform(2.0 ** -8, 1.0, n).astype(np.float32)


def exact_frames(n, seed):
    """(value [4, n], weight [4, n]): plain, duplicated values, 10 % zero weights, NaN values at weight 0"""
    rs = np.random.RandomState(seed)
    v = rs.uniform(0.1, 30.0, (4, n)).astype(np.float32)
    w = np.stack([exact_weights(rs, n) for _ in range(4)])
    v[1] = rs.choice(v[1, :max(1, n // 7)], n)
    w[2, rs.rand(n) < 0.1] = 0
    nan = rs.rand(n) < 0.15
    v[3, nan], w[3, nan] = np.nan, 0
    return v, w


@pytest.mark.parametrize('shape', SHAPES)
def test_percentiles_bit_equal_where_sums_are_exact(shape):
    D = dv()
    n = shape[0] * shape[1]
    v, w = exact_frames(n, n)
    for ps in PS_SETS:
        got = D.weighted_percentiles(T(v), T(w), ps)
        ref = np.stack([R.percentiles(v[f], w[f], ps) for f in range(4)])
        assert got.dtype == np.float64 and got.shape == (4, len(ps))
        np.testing.assert_array_equal(got, ref, err_msg='N = %d ps = %s' % (n, ps))              # NaN where the helper has NaN
        ok = ~np.isnan(ref)
        np.testing.assert_array_equal(got[ok].view(np.uint64), ref[ok].view(np.uint64), err_msg='N = %d ps = %s' % (n, ps))


def order_gate(value, weight, ps):
    """(ref [P], gate [P]): the helper's percentiles and the worst another summation order can do to them"""
    ref, j, wj, xs, cw = R.weighted_percentile(value, weight, ps)
    gate = 4 * U53 * np.abs(ref)
    for k in range(len(ps)):
        if np.isfinite(wj[k]):
            gate[k] += 2 * xs.size * U53 * cw[-1] / wj[k] * (xs[j[k] + 1] - xs[j[k]])
    return ref, gate


@pytest.mark.parametrize('shape', SHAPES)
def test_percentiles_general_weights_within_the_order_bound(shape):
    D = dv()
    n = shape[0] * shape[1]
    rs = np.random.RandomState(100 + n)
    v = rs.uniform(0.1, 30.0, (3, n)).astype(np.float32)
    w = (1.0 - rs.rand(3, n)).astype(np.float32)              # uniform in (0, 1]
    worst = 0.0
    for ps in PS_SETS:
        got = D.weighted_percentiles(T(v), T(w), ps)
        for f in range(3):
            ref, gates = order_gate(v[f], w[f], ps)
            for k in range(len(ps)):
                gate = gates[k]
                err = abs(got[f, k] - ref[k])
                worst = max(worst, err / max(abs(ref[k]), 1e-300))
                print('N = %d p = %g: dev %.17g ref %.17g err %.3g gate %.3g' % (n, ps[k], got[f, k], ref[k], err, gate))
                assert err <= gate, (n, ps[k], got[f, k], ref[k], err, gate)
    print('N = %d: worst relative error %.3g' % (n, worst))


def test_same_bits_twice_and_batch_of_five_is_five_single_calls():
    D = dv()
    rs = np.random.RandomState(7)
    n = 96 * 129
    v = rs.uniform(0.1, 30.0, (5, n)).astype(np.float32)
    w = (1.0 - rs.rand(5, n)).astype(np.float32)
    tv, tw = T(v), T(w)
    a = D.weighted_percentiles(tv, tw, (0.5, 99.5))
    b = D.weighted_percentiles(tv, tw, (0.5, 99.5))
    np.testing.assert_array_equal(a.view(np.uint64), b.view(np.uint64))
    single = np.concatenate([D.weighted_percentiles(tv[f:f + 1], tw[f:f + 1], (0.5, 99.5)) for f in range(5)])
    np.testing.assert_array_equal(a.view(np.uint64), single.view(np.uint64))
    ma, mb = D.minmax(tv), np.concatenate([D.minmax(tv[f:f + 1]) for f in range(5)])
    np.testing.assert_array_equal(ma.view(np.uint32), mb.view(np.uint32))
    img = D.minmax_colorize_async(tv.reshape(5, 96, 129)).get()['image']
    one = np.concatenate([D.minmax_colorize_async(tv[f].reshape(1, 96, 129)).get()['image'] for f in range(5)])
    np.testing.assert_array_equal(img, one)


@pytest.mark.parametrize('shape', SHAPES)
def test_minmax_equals_numpy(shape):
    D = dv()
    n = shape[0] * shape[1]
    rs = np.random.RandomState(n)
    v = rs.normal(0, 20, (4, n)).astype(np.float32)
    v[1] = np.float32(3.25)                                   # a constant frame
    v[2, rs.randint(n)] = np.nan
    v[3] = np.nan
    got = D.minmax(T(v))
    ref = np.stack([R.minmax(v[f]) for f in range(4)])
    assert got.dtype == np.float32
    np.testing.assert_array_equal(got, ref)
    ok = ~np.isnan(ref)
    np.testing.assert_array_equal(got[ok].view(np.uint32), ref[ok].view(np.uint32))


def smooth(rs, H, W, lo, hi):
    """a smooth random field in [lo, hi]"""
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)
    f = sum(rs.normal() * np.sin(rs.uniform(0.05, 0.4) * x + rs.uniform(0.05, 0.4) * y + rs.uniform(0, 6)) for _ in range(4))
    f = (f - f.min()) / max(f.max() - f.min(), 1e-9)
    return (lo + (hi - lo) * f).astype(np.float32)


def picture_inputs(H, W, seed):
    """one frame's suite inputs: smooth fields, acc = 0 and acc = 1 regions, a NaN distance"""
    rs = np.random.RandomState(seed)
    acc = smooth(rs, H, W, 0.05, 0.95)
    acc[:max(1, H // 4)] = 0
    acc[-max(1, H // 4):, :max(1, W // 2)] = 1
    dmean, dmedian = smooth(rs, H, W, 0.5, 9.0), smooth(rs, H, W, 0.5, 9.0)
    p5, p95 = (dmedian * np.float32(0.8)).astype(np.float32), (dmedian * np.float32(1.3)).astype(np.float32)
    dmean[H // 2, W // 2] = np.nan
    rgb = np.stack([smooth(rs, H, W, -0.1, 1.1) for _ in range(3)], -1)
    org = np.stack([smooth(rs, H, W, -1, 1) for _ in range(3)], -1)
    dirs = np.stack([smooth(rs, H, W, -1, 1) for _ in range(3)], -1)
    return dict(rgb=rgb, acc=acc, dmean=dmean, dmedian=dmedian, p5=p5, p95=p95, origins=org, directions=dirs)


def check_picture(got, ref, fragile, what):
    assert got.shape == ref.shape and got.dtype == np.uint8, what
    assert fragile.mean() <= 1e-3, '%s: %d fragile pixels of %d' % (what, fragile.sum(), fragile.size)
    bad = (got != ref).any(-1) & ~fragile
    assert not bad.any(), '%s: %d pixels differ, first at %s: %s vs %s' % (what, bad.sum(), np.argwhere(bad)[0],
                                                                          got[bad][0], ref[bad][0])


@pytest.mark.parametrize('shape', PICTURE_SHAPES)
def test_suite_pictures_equal_the_helper(shape):
    H, W = shape
    frames = [picture_inputs(H, W, 10 * H + f) for f in range(2)]
    refs = [R.mip360_suite(**f) for f in frames]
    for f, r in zip(frames, refs):
        acc = R.effective_acc(f['acc'], f['dmean'])
        trip = R.triplet_value(f['dmedian'], f['p5'], f['p95'])
        for k, v, w in (('mean', f['dmean'], acc), ('median', f['dmedian'], acc), ('triplet', trip, np.repeat(acc[..., None], 3, -1))):
            r['gate_' + k] = order_gate(v, w, R.SUITE_PS)[1]
    for r in refs:                                            # on the CPU, before any launch: the inputs keep the helper under the cap
        for k in ('depth_mean', 'depth_median', 'depth_triplet', 'color_matte', 'coords_mod'):
            assert r[k][1].mean() <= 1e-3, k
    D = dv()
    st = lambda k: T(np.stack([f[k] for f in frames]))
    got = D.mip360_suite_async(st('rgb'), st('acc'), st('dmean'), st('dmedian'), st('p5'), st('p95'), st('origins'),
                               st('directions')).get()
    for f, r in enumerate(refs):
        np.testing.assert_array_equal(got['acc'][f], R.effective_acc(frames[f]['acc'], frames[f]['dmean']))
        for k in ('mean', 'median', 'triplet'):
            assert np.all(np.abs(got['lohi_' + k][f] - r['lohi_' + k]) <= r['gate_' + k]), (k, got['lohi_' + k][f], r['lohi_' + k])
        for k in D.SUITE_KEYS:
            check_picture(got[k][f], r[k][0], r[k][1], '%s %dx%d frame %d' % (k, H, W, f))


@pytest.mark.parametrize('shape', PICTURE_SHAPES)
def test_minmax_pictures_equal_the_helper(shape):
    H, W = shape
    rs = np.random.RandomState(H)
    x = np.stack([smooth(rs, H, W, 0.3, 40.0), np.full((H, W), 2.5, np.float32), smooth(rs, H, W, -3.0, 3.0)])
    refs = [R.colorize_minmax(x[f]) for f in range(3)]
    for r in refs:
        assert r[1].mean() <= 1e-3
    D = dv()
    got = D.minmax_colorize_async(T(x)).get()
    for f, (b, fr, (vmin, vmax)) in enumerate(refs):
        assert got['minmax'][f, 0] == np.float32(vmin)
        check_picture(got['image'][f], b, fr, 'minmax %dx%d frame %d' % (H, W, f))


@pytest.mark.parametrize('shape', PICTURE_SHAPES)
def test_cmap_with_equal_bounds_and_identity_curve(shape):
    """lo == hi after the curve: the weight sits on a block of the frame's smallest value, which is too large for +-eps to
    move, so the division is by 0 (that value 0 / 0 -> 0, everything else clips); and the identity curve on jet."""
    H, W = shape
    rs = np.random.RandomState(H + 1)
    v = smooth(rs, H, W, 2.0 ** 41, 2.0 ** 42)
    acc = np.zeros((H, W), np.float32)
    v[:2, :3], acc[:2, :3] = np.float32(2.0 ** 40), 1
    b0, fr0, lohi0 = R.visualize_cmap(v, acc, 'turbo', 'neg_log')
    assert lohi0[0] == lohi0[1] == 2.0 ** 40
    v1, acc1 = smooth(rs, H, W, 0.5, 9.0), smooth(rs, H, W, 0.0, 1.0)
    b1, fr1, _ = R.visualize_cmap(v1, acc1, 'jet', 'identity')
    assert fr0.mean() <= 1e-3 and fr1.mean() <= 1e-3
    D = dv()
    got0 = D.colorize_cmap_async(T(v), T(acc), cmap='turbo', curve='neg_log').get()
    assert tuple(got0['lohi'][0]) == lohi0
    check_picture(got0['image'][0], b0, fr0, 'lo == hi %dx%d' % (H, W))
    got1 = D.colorize_cmap_async(T(v1), T(acc1), cmap='jet', curve='identity').get()
    check_picture(got1['image'][0], b1, fr1, 'identity %dx%d' % (H, W))

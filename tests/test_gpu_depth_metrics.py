"""GPU: libdepthmetrics_hip.so against the numpy helper tests/depth_metrics_reference.py.

n_valid, the error map and a1 / a2 / a3 equal the helper's (the inputs hold no thresh within 1e-12 relative of a threshold: checked
on the CPU, on the inputs).  rmse, absrel, sqrel and absdiff are within (2 N + 8) 2^-53 relative: their terms are non-negative, so
any order of summation is within (N - 1) 2^-53 of the exact sum on either side, and 8 covers the final division and root and a
last-bit difference in a term.  rmse_log gets 1.5e-14 absolute on top: the device's float64 log is held to OpenCL's 3 ulp and
numpy's to 1, |log x| <= 6.91 on [1e-3, 80], so each L moves by at most 1.2e-14 and a root mean square by no more than its terms.
A frame's numbers are the same bits from call to call and in any batch."""
import numpy as np
import pytest
import torch

from tests import depth_metrics_reference as R

pytestmark = pytest.mark.gpu

SCALE = 0.0137
NAMES = R.METRIC_NAMES


def dm():
    if not torch.cuda.is_available():
        pytest.skip('needs a GPU')
    from outdoor_nerf_depth_amd import depth_metrics
    return depth_metrics


def T(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def sizes():
    from outdoor_nerf_depth_amd.depth_metrics import WG_PIXELS
    two = WG_PIXELS + 1                                       # the smallest frame two workgroups reduce
    return [(1, 1), (1, 2), (1, 63), (1, 64), (1, 65), (1, 255), (1, 256), (1, 257), (1, 1023), (1, 1025), (1, 4097), (96, 129),
            (1, two - 1), (1, two), (1, two + 1)]


def odd_sizes():
    two = sizes()[-2][1]
    return [1, 63, 65, 257, 1023, 1025, 4097, 96 * 129 - 1] + [n for n in (two - 1, two, two + 1) if n % 2]


def bits(host):
    return {k: np.ascontiguousarray(host[k]).view(np.uint64 if k != 'err_map' else np.uint32) for k in host}


def check(got, pred, gt, scale, what):
    ref, err_map, near = R.split_metrics(pred, gt, scale)
    assert near == 0, '%s: the inputs hold %d thresh values on a threshold' % (what, near)
    for k in NAMES:
        assert got[k].dtype == np.float64 and got[k].shape == (pred.shape[0],)
    R.assert_rows_close(got, ref, what)
    if 'err_map' in got:
        assert got['err_map'].dtype == np.float32
        np.testing.assert_array_equal(got['err_map'], err_map, err_msg=what)
    return ref


@pytest.mark.parametrize('shape', sizes())
def test_one_frame_against_the_helper(shape):
    D = dm()
    pred, gt = R.seeded_frames(shape, SCALE, seed=shape[0] * shape[1])
    got = D.depth_metrics(T(pred), T(gt), SCALE, err_map=True)
    check(got, pred, gt, SCALE, 'shape %s' % (shape,))
    plain = D.depth_metrics(T(pred[0]), T(gt[0]), SCALE)      # [H, W], no map: the same numbers
    assert 'err_map' not in plain
    for k in NAMES:
        np.testing.assert_array_equal(bits(plain)[k], bits(got)[k])


@pytest.mark.parametrize('n_frames', [2, 5])
@pytest.mark.parametrize('n', odd_sizes())
def test_batches_of_odd_frames(n_frames, n):
    """odd n: every other frame starts 4 bytes off a 16-byte boundary, so both load forms run in one call"""
    D = dm()
    assert n % 2 == 1
    pred, gt = R.seeded_frames((1, n), SCALE, seed=7 * n + n_frames, n_frames=n_frames)
    got = D.depth_metrics(T(pred), T(gt), SCALE, err_map=True)
    check(got, pred, gt, SCALE, 'F %d n %d' % (n_frames, n))
    again = D.depth_metrics(T(pred), T(gt), SCALE, err_map=True)
    for k in got:
        np.testing.assert_array_equal(bits(again)[k], bits(got)[k], err_msg='%s: call to call' % k)
    for f in range(n_frames):                                 # a frame's bits do not depend on the batch around it
        single = D.depth_metrics(T(pred[f:f + 1]), T(gt[f:f + 1]), SCALE, err_map=True)
        for k in got:
            np.testing.assert_array_equal(bits(single)[k][0], bits(got)[k][f], err_msg='%s: frame %d alone' % (k, f))


@pytest.mark.parametrize('shape', [(1, 65), (5, 411), (96, 129)])
def test_empty_and_nan_frames_leave_their_neighbours_alone(shape):
    D = dm()
    pred, gt = R.seeded_frames(shape, SCALE, seed=11 + shape[1], n_frames=5)
    clean = D.depth_metrics(T(pred), T(gt), SCALE, err_map=True)
    pred2, gt2 = pred.copy(), gt.copy()
    gt2[1] = 0                                                # an empty frame
    valid = R.prepare(pred2[3], gt2[3], SCALE)[2]
    assert valid.any()
    pred2[3][tuple(np.argwhere(valid)[-1])] = np.nan          # a NaN prediction on a valid pixel
    got = D.depth_metrics(T(pred2), T(gt2), SCALE, err_map=True)
    check(got, pred2, gt2, SCALE, 'shape %s' % (shape,))
    assert got['n_valid'][1] == 0 and all(np.isnan(got[k][1]) for k in NAMES[1:]) and not got['err_map'][1].any()
    assert got['n_valid'][3] == np.count_nonzero(valid)
    assert all(np.isnan(got[k][3]) for k in ('rmse', 'absrel', 'sqrel', 'absdiff', 'rmse_log'))
    assert all(np.isfinite(got[k][3]) and got[k][3] <= clean[k][3] for k in ('a1', 'a2', 'a3'))    # it counts in no threshold
    assert np.count_nonzero(np.isnan(got['err_map'][3])) == 1
    for f in (0, 2, 4):
        for k in got:
            np.testing.assert_array_equal(bits(got)[k][f], bits(clean)[k][f], err_msg='%s: frame %d' % (k, f))


def test_clipping_and_invalid_ground_truth():
    D = dm()
    s = np.float32(SCALE)
    gt = (np.array([[10.0, 10.0, 10.0, 10.0, 10.0, np.nan, np.inf, -np.inf, 10.0]], np.float32) * s)[None]
    pred = (np.array([[-np.inf, np.inf, -3.0, 500.0, 1e-5, 10.0, 10.0, 10.0, 12.0]], np.float32) * s)[None]
    got = D.depth_metrics(T(pred), T(gt), SCALE, err_map=True)
    check(got, pred, gt, SCALE, 'clipping')
    assert got['n_valid'][0] == 6                             # a NaN or infinite ground truth is invalid
    want = gt[0, 0, 0] / s
    lo, hi = np.abs(want - np.float32(1e-3)), np.abs(want - np.float32(80))
    np.testing.assert_array_equal(got['err_map'][0, 0, :5], np.array([lo, hi, lo, hi, lo], np.float32))
    np.testing.assert_array_equal(got['err_map'][0, 0, 5:8], np.zeros(3, np.float32))
    assert got['a1'][0] == 1.0 / 6


@pytest.mark.parametrize('scale', [1.0, 0.31])
def test_other_scales_and_the_bounds(scale):
    D = dm()
    s = np.float32(scale)
    pred, gt = R.seeded_frames((7, 59), scale, seed=int(100 * scale), n_frames=2)
    gt[0, 0, 0], gt[0, 0, 1] = np.float32(80) * s, np.float32(1e-3) * s           # exactly on the bounds: excluded
    got = D.depth_metrics(T(pred), T(gt), scale, err_map=True)
    ref = check(got, pred, gt, scale, 'scale %s' % scale)
    assert got['err_map'][0, 0, 0] == 0 and got['err_map'][0, 0, 1] == 0 and ref['n_valid'][0] > 0


def test_wrong_arguments_are_named():
    D = dm()
    a = torch.zeros(2, 4, 6, device='cuda')
    with pytest.raises(D.DepthMetricsError, match='gt: expected a CUDA/HIP'):
        D.depth_metrics_async(a, a.cpu(), 1.0)
    with pytest.raises(D.DepthMetricsError, match='pred: expected torch.float32'):
        D.depth_metrics_async(a.double(), a, 1.0)
    with pytest.raises(D.DepthMetricsError, match=r'pred \(2, 4, 6\) and gt \(2, 4, 5\): shapes differ'):
        D.depth_metrics_async(a, a[..., :5].contiguous(), 1.0)
    with pytest.raises(D.DepthMetricsError, match='gt: expected a contiguous'):
        D.depth_metrics_async(a, torch.zeros(2, 6, 4, device='cuda').transpose(1, 2), 1.0)
    with pytest.raises(D.DepthMetricsError, match='scale'):
        D.depth_metrics_async(a, a, 0.0)
    with pytest.raises(D.DepthMetricsError, match=r'pred: expected \[F, H, W\]'):
        D.depth_metrics_async(a[0, 0], a[0, 0], 1.0)


def test_async_tensors_stay_on_the_device():
    D = dm()
    pred, gt = R.seeded_frames((9, 31), SCALE, seed=5, n_frames=3)
    pend = D.depth_metrics_async(T(pred), T(gt), SCALE, err_map=True)
    assert pend.tensors['rows'].is_cuda and pend.tensors['rows'].shape == (3, 9) and pend.tensors['rows'].dtype == torch.float64
    assert pend.tensors['err_map'].shape == (3, 9, 31)
    host = pend.get()
    assert host is pend.get()
    np.testing.assert_array_equal(host['rmse'], pend.tensors['rows'][:, 1].cpu().numpy())

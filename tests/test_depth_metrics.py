"""Host side of the depth-error metrics: the numpy helper tests/depth_metrics_reference.py against the host
function the evaluators use (eval_outputs.depth_errors) and against frames whose answers are known in closed form, the argument checks of
libdepthmetrics_hip.so (which need no GPU), the five parsers' flag and eval_images' file selection for --depth_metrics."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from tests import depth_metrics_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCALES = [1.0, 0.0137, 0.31]
NAMES = R.METRIC_NAMES


def row(pred, gt, scale=1.0):
    return dict(zip(NAMES, R.frame_metrics(np.asarray(pred, np.float32), np.asarray(gt, np.float32), scale)['row']))


@pytest.mark.parametrize('scale', SCALES)
@pytest.mark.parametrize('shape', [(1, 65), (96, 129)])
def test_helper_is_the_two_host_functions(shape, scale):
    from outdoor_nerf_depth_amd import eval_outputs
    pred, gt = R.seeded_frames(shape, scale, seed=shape[1] + int(1000 * scale))
    pred, gt = pred[0], gt[0]
    ref = R.frame_metrics(pred, gt, scale)
    g = gt / scale
    valid = (g < 80) & (g > 1e-3)
    assert 0.6 < valid.mean() < 0.8                                               # about 30 % of the ground truth is invalid
    assert (pred < 0).any() and (pred / scale > 80).any() and valid.any()
    np.testing.assert_array_equal(ref['valid'], valid)
    rmse, absrel, absrel_map = eval_outputs.depth_errors(pred, gt, scale)          # both families' host function
    assert absrel_map.dtype == np.float32 and ref['err_map'].dtype == np.float32
    np.testing.assert_array_equal(ref['err_map'], absrel_map)
    m = dict(zip(NAMES, ref['row']))
    assert m['n_valid'] == np.count_nonzero(valid)
    for got, want in ((m['rmse'], rmse), (m['absrel'], absrel)):
        print('helper %r host %r relative %.3e' % (got, want, abs(got - want) / abs(want)))
        assert abs(got - want) <= 5e-6 * abs(want)                                # the host path is float32


def test_closed_forms():
    one = row([[3.0]], [[2.0]])                                                   # one valid pixel
    assert one['n_valid'] == 1 and one['rmse'] == 1.0 and one['absrel'] == 0.5 and one['sqrel'] == 0.5 and one['absdiff'] == 1.0
    assert one['rmse_log'] == abs(np.log(2.0) - np.log(3.0)) and (one['a1'], one['a2'], one['a3']) == (0.0, 1.0, 1.0)
    gt = np.array([[1.0, 2.0, 4.0, 8.0, 0.0, 100.0]], np.float32)
    same = row(gt, gt)                                                            # pred == gt
    assert same['n_valid'] == 4
    assert all(same[k] == 0.0 for k in ('rmse', 'absrel', 'sqrel', 'absdiff', 'rmse_log')) and same['a1'] == same['a3'] == 1.0
    twice = row(2 * gt, gt)                                                       # pred = 2 gt: 2 is not below 1.953125
    assert twice['absrel'] == 1.0 and (twice['a1'], twice['a2'], twice['a3']) == (0.0, 0.0, 0.0)
    assert twice['absdiff'] == 15.0 / 4 and twice['sqrel'] == 15.0 / 4 and twice['rmse'] == np.sqrt(85.0 / 4)
    np.testing.assert_allclose(twice['rmse_log'], np.log(2.0), rtol=1e-15)
    half = row(0.5 * gt, gt)                                                      # the ratio is symmetric
    assert half['absrel'] == 0.5 and (half['a1'], half['a2'], half['a3']) == (0.0, 0.0, 0.0)
    a = row([[1.2, 1.5, 1.9, 2.5]], [[1.0, 1.0, 1.0, 1.0]])
    assert (a['a1'], a['a2'], a['a3']) == (0.25, 0.5, 0.75)
    scaled = row(np.float32(0.5) * 2 * gt, np.float32(0.5) * gt, 0.5)             # the scale divides out (a power of two: exactly)
    assert all(scaled[k] == twice[k] for k in NAMES)


def test_empty_frame_is_nan():
    for gt in ([[0.0, -1.0, 80.0, 500.0]], [[np.nan]]):
        m = row(np.ones_like(gt), gt)
        assert m['n_valid'] == 0
        assert all(np.isnan(m[k]) for k in NAMES[1:])
        assert not R.frame_metrics(np.ones_like(gt, np.float32), np.asarray(gt, np.float32), 1.0)['err_map'].any()


@pytest.mark.parametrize('scale', SCALES)
def test_bounds_are_excluded(scale):
    s = np.float32(scale)
    lo, hi = np.float32(1e-3) * s, np.float32(80) * s
    assert lo / s == np.float32(1e-3) and hi / s == np.float32(80)                 # the two frames below sit exactly on the bounds
    gt = np.array([[lo, hi, np.nextafter(hi, np.float32(0)), np.float32(2) * s]], np.float32)
    f = R.frame_metrics(np.full((1, 4), s, np.float32), gt, scale)
    np.testing.assert_array_equal(f['valid'], [[False, False, True, True]])
    assert f['row'][0] == 2


def test_predictions_clip_and_nan_passes():
    gt = np.full((1, 5), 10.0, np.float32)
    pred = np.array([[-np.inf, -3.0, 0.0, np.inf, 500.0]], np.float32)
    g, vp, valid, err = R.prepare(pred, gt, 1.0)
    np.testing.assert_array_equal(vp, np.array([[1e-3, 1e-3, 1e-3, 80.0, 80.0]], np.float32))
    np.testing.assert_array_equal(vp, np.clip(pred, np.float32(1e-3), np.float32(80)))
    m = row(pred, gt)
    assert m['n_valid'] == 5 and m['a3'] == 0.0 and np.isfinite(m['rmse_log'])
    pred = np.array([[10.0, np.nan, 10.0, 10.0, 10.0]], np.float32)               # a NaN prediction on a valid pixel
    g, vp, valid, err = R.prepare(pred, gt, 1.0)
    assert np.isnan(vp[0, 1]) and np.isnan(np.clip(pred, np.float32(1e-3), np.float32(80))[0, 1]) and np.isnan(err[0, 1])
    m = row(pred, gt)
    assert m['n_valid'] == 5 and all(np.isnan(m[k]) for k in ('rmse', 'absrel', 'sqrel', 'absdiff', 'rmse_log'))
    assert m['a1'] == m['a2'] == m['a3'] == 0.8                                   # it counts in no threshold
    gt[0, 1] = 0                                                                  # on an invalid pixel it touches nothing
    m = row(pred, gt)
    assert m['n_valid'] == 4 and m['rmse'] == 0.0 and m['a1'] == 1.0


def test_near_threshold_count():
    assert R.frame_metrics(np.float32([[1.25]]), np.float32([[1.0]]), 1.0)['near'] == 1
    assert R.frame_metrics(np.float32([[1.3]]), np.float32([[1.0]]), 1.0)['near'] == 0


def test_sizes_and_scale_are_rejected_with_a_reason():
    from outdoor_nerf_depth_amd import depth_metrics as D
    assert D.METRIC_NAMES == NAMES
    assert D.workspace_bytes(1, 1) > 0 and D.workspace_bytes(30, 375 * 1242) % 256 == 0
    assert D.workspace_bytes(65535, 1) > 0 and D.workspace_bytes(1, 1 << 28) > 0
    with pytest.raises(D.DepthMetricsError, match='at least one pixel'):
        D.workspace_bytes(1, 0)
    with pytest.raises(D.DepthMetricsError, match=r'2\^28'):
        D.workspace_bytes(1, (1 << 28) + 1)
    for f in (0, 65536):
        with pytest.raises(D.DepthMetricsError, match='n_frames'):
            D.workspace_bytes(f, 16)
    call = lambda F, n, scale, ptr=None: D.lib().depthmetrics_frames(None, F, n, ptr, ptr, scale, ptr, ptr, None)
    for F, n, what in ((0, 4, 'n_frames'), (1, 0, 'at least one pixel'), (1, (1 << 28) + 1, r'2\^28')):
        assert call(F, n, 1.0) == 1 and re.search(what, D.last_error()), D.last_error()
    for scale in (0.0, -1.0, float('nan'), float('inf'), 1e-60, 1e60):           # the last two are 0 and inf in float32
        assert call(1, 4, scale) == 1 and 'scale' in D.last_error(), D.last_error()
    assert call(1, 4, 1.0) == 1 and 'non-null' in D.last_error()                  # sizes and scale pass, the pointers do not
    assert call(1, 4, 1.0, C.c_void_p(258)) == 1 and 'aligned' in D.last_error()


def test_binding_mirrors_the_header():
    from outdoor_nerf_depth_amd import depth_metrics as D
    text = open(os.path.join(ROOT, 'include', 'depthmetrics_hip.h')).read()
    define = lambda name: re.search(r'#define DEPTHMETRICS_%s\s+(\S+)' % name, text).group(1)
    assert int(define('ABI_VERSION')) == D.ABI_VERSION and int(define('WG_PIXELS')) == D.WG_PIXELS
    assert int(define('ROW')) == len(D.METRIC_NAMES) and int(define('MAX_FRAMES')) == D.MAX_FRAMES
    for k, name in enumerate(D.METRIC_NAMES):
        assert int(define(name.upper())) == k
    for sym in D.SYMBOLS:
        assert re.search(r'\b%s\(' % sym, text), sym


def test_binding_names_the_wrong_argument():
    torch = pytest.importorskip('torch')
    from outdoor_nerf_depth_amd import depth_metrics as D
    with pytest.raises(D.DepthMetricsError, match='pred: expected a CUDA/HIP'):
        D.depth_metrics_async(torch.zeros(2, 3), torch.zeros(2, 3), 1.0)
    with pytest.raises(D.DepthMetricsError, match='pred: expected a CUDA/HIP'):
        D.depth_metrics_async(np.zeros((2, 3), np.float32), np.zeros((2, 3), np.float32), 1.0)


def test_the_five_parsers_accept_the_flag():
    from outdoor_nerf_depth_amd import ddp_test_nerf, ddp_train_nerf, eval_images, mip360_eval, mip360_train
    for parser in (mip360_eval.make_parser, mip360_train.make_parser, eval_images.make_parser):
        assert parser().parse_args(['--depth_metrics']).depth_metrics is True
        assert parser().parse_args([]).depth_metrics is False
        assert 'a1 / a2 / a3' in parser().format_help() or 'a1, a2, a3' in parser().format_help()
    base = ['--expname', 'x']
    assert ddp_test_nerf.config_parser is ddp_train_nerf.config_parser            # the two NeRF++ CLIs share one parser
    assert ddp_train_nerf.config_parser().parse_args(base + ['--depth_metrics']).depth_metrics is True
    assert ddp_train_nerf.config_parser().parse_args(base).depth_metrics is False
    args = eval_images.make_parser().parse_args([])
    assert args.gt_depth_dir is None and args.pred_depth_dir is None and args.depth_frames is None


def _write16(path, a):
    from PIL import Image
    Image.fromarray(np.asarray(a, np.uint16)).save(str(path))


def _folders(tmp_path, n_gt=20, shape=(5, 7)):
    """depths_gt with n_gt frames (raw 0 and 1 among the values), a render folder with one depth_*.png per test frame"""
    rs = np.random.RandomState(0)
    gt_dir, pred_dir = tmp_path / 'depths_gt', tmp_path / 'preds'
    gt_dir.mkdir()
    pred_dir.mkdir()
    gts = []
    for i in range(n_gt):
        a = rs.randint(2, 80 * 256, shape).astype(np.uint16)
        a[0, :3] = (0, 1, 2)
        a[1, 0] = 81 * 256
        gts.append(a)
        _write16(gt_dir / ('%04d.png' % i), a)
    preds = []
    for k in range(n_gt // 10):
        a = rs.randint(0, 90 * 256, shape).astype(np.uint16)
        preds.append(a)
        _write16(pred_dir / ('depth_%03d.png' % k), a)
    (pred_dir / 'color_000.png').write_bytes(b'not an image: --depth_metrics reads no colour file')
    return gt_dir, pred_dir, gts, preds


def _helper_fn(calls):
    def fn(preds, gts):
        assert preds.dtype == np.float32 and gts.dtype == np.float32 and preds.shape == gts.shape and preds.ndim == 3
        calls.append((preds.copy(), gts.copy()))
        return R.split_metrics(preds, gts, 1.0)[0]
    return fn


def _read(path):
    return [float(v) for v in path.read_text().split('\n')]


def test_eval_images_selects_test_frames(tmp_path):
    from outdoor_nerf_depth_amd import eval_images as E
    gt_dir, pred_dir, gts, preds = _folders(tmp_path)
    before = set(os.listdir(str(pred_dir)))
    calls = []
    out = E.depth_metrics_folder(str(gt_dir), str(pred_dir), 'mipnerf360', metrics_fn=_helper_fn(calls))
    assert len(calls) == 1                                                        # frames of one size: one call
    p, g = calls[0]
    for k, i in enumerate((9, 19)):                                               # indices 9, 19 as select_files takes them
        want = gts[i].astype(np.float32) / 256
        want[gts[i] < 2] = -1                                                     # the loader's rule: raw < 2 is invalid
        np.testing.assert_array_equal(g[k], want)
        np.testing.assert_array_equal(p[k], preds[k].astype(np.float32) / 256)
    assert set(os.listdir(str(pred_dir))) == before | {'eval_depth_%s.txt' % n for n in NAMES}
    ref = R.split_metrics(p, g, 1.0)[0]
    for n in NAMES:
        vals = _read(pred_dir / ('eval_depth_%s.txt' % n))
        assert vals == out[n] and len(vals) == 3 and vals[:2] == [float(v) for v in ref[n]] and vals[2] == float(np.mean(ref[n]))
    # nerfpp: raw / 256 without the rule (0 and 1 / 256 m are invalid by the 1e-3 m bound or not at all)
    calls.clear()
    E.depth_metrics_folder(str(gt_dir), str(pred_dir), 'nerfpp', metrics_fn=_helper_fn(calls))
    np.testing.assert_array_equal(calls[0][1][0], gts[9].astype(np.float32) / 256)
    # all: every file, so the counts differ and the error names both sides
    with pytest.raises(E.EvalImagesError) as e:
        E.depth_metrics_folder(str(gt_dir), str(pred_dir), 'nerfpp', depth_frames='all', metrics_fn=_helper_fn(calls))
    assert '20 ground-truth depth frames' in str(e.value) and '2 predictions' in str(e.value)
    assert str(gt_dir) in str(e.value) and str(pred_dir) in str(e.value)
    with pytest.raises(E.EvalImagesError, match='mipnerf360_cc'):
        E.depth_metrics_folder(str(gt_dir), str(pred_dir), 'mipnerf360_cc', metrics_fn=_helper_fn(calls))


def test_eval_images_scores_a_prior_folder(tmp_path):
    from outdoor_nerf_depth_amd import eval_images as E
    gt_dir, pred_dir, gts, _ = _folders(tmp_path, n_gt=4)
    prior_dir = tmp_path / 'depths_mono_crop'
    prior_dir.mkdir()
    rs = np.random.RandomState(1)
    priors = []
    for i in range(4):
        a = rs.randint(2, 80 * 256, gts[0].shape).astype(np.uint16)
        a[2, :2] = (0, 1)                                                         # holes of the prior
        priors.append(a)
        _write16(prior_dir / ('%04d.png' % i), a)
    calls = []
    out = E.depth_metrics_folder(str(gt_dir), str(pred_dir), 'mipnerf360', pred_depth_dir=str(prior_dir), metrics_fn=_helper_fn(calls))
    p, g = calls[0]
    assert p.shape == (4,) + gts[0].shape                                         # implies `all`
    for i in range(4):
        want = gts[i].astype(np.float32) / 256
        want[gts[i] < 2] = -1
        want[priors[i] < 2] = -1                                                  # the prior's holes leave the valid set
        np.testing.assert_array_equal(g[i], want)
        np.testing.assert_array_equal(p[i], priors[i].astype(np.float32) / 256)
        valid = (gts[i] >= 2) & (gts[i] < 80 * 256) & (priors[i] >= 2)
        assert out['n_valid'][i] == np.count_nonzero(valid)
    assert {'eval_depth_%s.txt' % n for n in NAMES} <= set(os.listdir(str(pred_dir)))
    with pytest.raises(E.EvalImagesError, match='no frame'):                      # 4 files hold no test frame
        E.depth_metrics_folder(str(gt_dir), str(pred_dir), 'mipnerf360', depth_frames='test', pred_depth_dir=str(prior_dir),
                               metrics_fn=_helper_fn(calls))


def test_eval_images_mismatches_name_both_sides(tmp_path):
    from outdoor_nerf_depth_amd import eval_images as E
    gt_dir, pred_dir, gts, preds = _folders(tmp_path)
    _write16(pred_dir / 'depth_001.png', np.zeros((5, 8), np.uint16))             # another size than its ground truth
    with pytest.raises(E.EvalImagesError) as e:
        E.depth_metrics_folder(str(gt_dir), str(pred_dir), 'mipnerf360', metrics_fn=_helper_fn([]))
    assert '0019.png is 5 x 7' in str(e.value) and 'depth_001.png is 5 x 8' in str(e.value)
    _write16(pred_dir / 'depth_001.png', preds[1])
    _write16(pred_dir / 'depth_002.png', preds[1])                                # one prediction too many
    with pytest.raises(E.EvalImagesError) as e:
        E.depth_metrics_folder(str(gt_dir), str(pred_dir), 'mipnerf360', metrics_fn=_helper_fn([]))
    assert '2 ground-truth depth frames' in str(e.value) and '3 predictions' in str(e.value)
    with pytest.raises(E.EvalImagesError, match='--gt_depth_dir'):
        E.main(['--depth_metrics', '--pred_dir', str(pred_dir)])


def test_eval_images_groups_frames_by_size(tmp_path):
    from outdoor_nerf_depth_amd import eval_images as E
    gt_dir, pred_dir = tmp_path / 'depth', tmp_path / 'preds'
    gt_dir.mkdir()
    pred_dir.mkdir()
    rs = np.random.RandomState(2)
    for i, shape in enumerate([(4, 6), (3, 5), (4, 6)]):
        _write16(gt_dir / ('%06d.png' % i), rs.randint(256, 70 * 256, shape))
        _write16(pred_dir / ('depth_%06d.png' % i), rs.randint(256, 70 * 256, shape))
    calls = []
    out = E.depth_metrics_folder(str(gt_dir), str(pred_dir), 'nerfpp', depth_frames='all', metrics_fn=_helper_fn(calls))
    assert [c[0].shape for c in calls] == [(2, 4, 6), (1, 3, 5)]
    assert out['n_valid'] == [24.0, 15.0, 24.0, 21.0]

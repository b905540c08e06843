"""CPU: the numpy statement of SSIM / 8-bit PSNR that the GPU tests compare against (tests/ssim_reference.py) pinned from
independent sides -- the formula written directly, closed forms -- plus the eval_images CLI on a temporary folder of PNGs and the
library's size check, which needs no GPU.  scikit-image itself is not installed, so no golden file can come from it."""
import os

import numpy as np
import pytest

from tests import ssim_reference as R


def _pair(shape, seed, sigma=20.0):
    rs = np.random.RandomState(seed)
    a = rs.randint(0, 256, shape).astype(np.uint8)
    b = np.clip(a + rs.normal(0, sigma, shape), 0, 255).astype(np.uint8)
    return a, b


def _single_window(x, y):
    """SSIM of one 7 x 7 window written directly: means, sample variances, sample covariance"""
    x, y = x.astype(np.float64).ravel(), y.astype(np.float64).ravel()
    ux, uy = np.mean(x), np.mean(y)
    vx, vy = np.var(x, ddof=1), np.var(y, ddof=1)
    vxy = np.cov(x, y, ddof=1)[0, 1]
    return (2 * ux * uy + R.C1) * (2 * vxy + R.C2) / ((ux ** 2 + uy ** 2 + R.C1) * (vx + vy + R.C2))


def test_one_window_equals_the_direct_formula():
    a, b = _pair((7, 7, 3), 0)
    want = np.mean([_single_window(a[..., c], b[..., c]) for c in range(3)])
    assert abs(R.ssim(a, b) - want) <= 1e-12


def test_image_equals_the_mean_of_the_direct_formula_over_all_crops():
    a, b = _pair((16, 20, 3), 1)
    per_channel = []
    for c in range(3):
        s = [_single_window(a[i:i + 7, j:j + 7, c], b[i:i + 7, j:j + 7, c]) for i in range(10) for j in range(14)]
        assert len(s) == 140
        per_channel.append(np.mean(s))
    assert abs(R.ssim(a, b) - np.mean(per_channel)) <= 1e-12
    assert R.ssim_map(a[..., 0], b[..., 0]).shape == (10, 14)


def test_box_sums_are_exact_integers():
    a = np.full((9, 11), 255, np.uint8)
    s = R.box_sums(a.astype(np.int64) ** 2)
    assert s.dtype == np.int64 and s.shape == (3, 5) and (s == 49 * 255 * 255).all()


def test_closed_forms():
    a, b = _pair((23, 31, 3), 2)
    assert R.ssim(a, a) == 1.0
    assert R.ssim(a, b) == R.ssim(b, a)
    assert R.psnr8(a, b) == R.psnr8(b, a)
    for va, vb in ((0, 255), (10, 200), (128, 127), (255, 255)):
        ca, cb = np.full((12, 15, 3), va, np.uint8), np.full((12, 15, 3), vb, np.uint8)
        want = (2.0 * va * vb + R.C1) / (va ** 2 + vb ** 2 + R.C1)
        assert abs(R.ssim(ca, cb) - want) <= 1e-12, (va, vb)
    lo = np.random.RandomState(3).randint(0, 255, (10, 12, 3)).astype(np.uint8)
    assert abs(R.psnr8(lo, lo + 1) - 20 * np.log10(255.0)) <= 1e-12
    assert R.psnr8(a, a) == float('inf')
    s, p = R.image_metrics(np.stack([a, a]), np.stack([a, b]))
    assert s.shape == p.shape == (2,) and s[0] == 1.0 and p[0] == float('inf') and s[1] == R.ssim(a, b) and p[1] == R.psnr8(a, b)


def test_helper_rejects_small_images_and_wrong_types():
    with pytest.raises(ValueError):
        R.ssim(np.zeros((6, 20, 3), np.uint8), np.zeros((6, 20, 3), np.uint8))
    with pytest.raises(ValueError):
        R.ssim(np.zeros((8, 8, 3), np.uint8), np.zeros((8, 9, 3), np.uint8))
    with pytest.raises(TypeError):
        R.ssim(np.zeros((8, 8, 3), np.float32), np.zeros((8, 8, 3), np.float32))


def test_library_rejects_images_smaller_than_the_window_without_a_gpu():
    from outdoor_nerf_depth_amd import _lib as L
    from outdoor_nerf_depth_amd import image_metrics as IM
    lib = L.lib()
    for H, W in ((6, 100), (100, 6), (0, 0)):
        assert lib.nerfpp_image_metrics_workspace_bytes(1, H, W) == -1
        assert b'7 x 7' in lib.nerfpp_last_error()
        rc = lib.nerfpp_image_metrics_u8(None, 1, H, W, None, None, None, None)      # sizes are checked before any pointer or HIP call
        assert rc == 1 and b'7 x 7' in lib.nerfpp_last_error()                       # NERFPP_ERR_ARG
        with pytest.raises(L.NerfppError, match='7 x 7'):
            IM.workspace_bytes(1, H, W)
    assert lib.nerfpp_image_metrics_u8(None, 0, 7, 7, None, None, None, None) == 1 and b'n_frames' in lib.nerfpp_last_error()
    assert lib.nerfpp_image_metrics_u8(None, 1, 7, 7, None, None, None, None) == 1 and b'non-null' in lib.nerfpp_last_error()
    # one float64 per (frame, channel, tile) and one uint64 per (frame, tile); tiles of 16 x 32 window positions
    assert IM.workspace_bytes(1, 7, 7) == 32
    assert IM.workspace_bytes(30, 375, 1242) == 30 * 24 * 39 * 32
    assert lib.nerfpp_abi_version() == L.ABI_VERSION == 10


def test_to_bytes_nearest_inverts_the_loaders_division():
    from outdoor_nerf_depth_amd.image_metrics import to_bytes_nearest
    b = np.arange(256, dtype=np.uint8)
    assert (to_bytes_nearest(b.astype(np.float32) / 255.) == b).all()
    assert (to_bytes_nearest(np.array([-0.5, 1.5, 0.5])) == [0, 255, 128]).all()


# ------------------------------------------------------------------------------------------------ eval_images
def _write_folders(tmp_path, method, n_gt=30, hw=(12, 17), gt_ext='png', seed=0):
    from PIL import Image
    rs = np.random.RandomState(seed)
    gt_dir, pred_dir = tmp_path / 'images', tmp_path / 'preds'
    gt_dir.mkdir()
    pred_dir.mkdir()
    gts = []
    for i in range(n_gt):
        im = rs.randint(0, 256, hw + (3,)).astype(np.uint8)
        Image.fromarray(im).save(str(gt_dir / ('frame_%04d.%s' % (i, gt_ext))))
        gts.append(im)
    test_gts = [gts[i] for i in range(9, n_gt, 10)]
    preds = []
    for k, g in enumerate(test_gts):
        p = np.clip(g + rs.normal(0, 10 + 10 * k, g.shape), 0, 255).astype(np.uint8)
        Image.fromarray(p).save(str(pred_dir / (('color_%03d.png' if method == 'mipnerf360' else '%06d.png') % k)))
        preds.append(p)
    # files that the patterns must not pick up
    Image.fromarray(preds[0][..., 0]).save(str(pred_dir / 'depth_000.png'))
    Image.fromarray(preds[0]).save(str(pred_dir / 'fg_000000.png'))
    return gt_dir, pred_dir, test_gts, preds


def _helper_fn(calls):
    def fn(gts, preds):
        calls.append((gts, preds))
        return R.image_metrics(np.stack(gts), np.stack(preds))
    return fn


@pytest.mark.parametrize('method', ['mipnerf360', 'nerfpp'])
def test_eval_images_selects_files_and_writes_both_metric_files(tmp_path, method, capsys, monkeypatch):
    from outdoor_nerf_depth_amd import eval_images as E
    gt_dir, pred_dir, test_gts, preds = _write_folders(tmp_path, method)
    calls = []
    monkeypatch.setattr(E, 'device_image_metrics', _helper_fn(calls))          # the device call: no GPU on this host
    E.main(['--gt_dir', str(gt_dir), '--pred_dir', str(pred_dir), '--method', method, '--split', '4'])
    assert len(calls) == 1 and len(calls[0][0]) == 3                            # ground-truth indices 9, 19, 29
    for got, want in zip(calls[0][0], test_gts):
        assert (got == want).all()
    for got, want in zip(calls[0][1], preds):
        assert (got == want).all()
    for name, fn in (('psnr', R.psnr8), ('ssim', R.ssim)):
        text = (pred_dir / ('eval_%s.txt' % name)).read_text()
        assert not text.endswith('\n')
        vals = [float(v) for v in text.split('\n')]
        want = [fn(g, p) for g, p in zip(test_gts, preds)]
        assert vals[:-1] == want and vals[-1] == sum(want) / 3                  # per image, then the mean; repr round-trips
    assert not (pred_dir / 'eval_lpips.txt').exists()
    out = capsys.readouterr().out
    assert 'eval_lpips.txt is not written' in out and 'VGG' in out


def test_eval_images_prefers_jpg_ground_truth(tmp_path):
    from PIL import Image
    from outdoor_nerf_depth_amd import eval_images as E
    gt_dir, pred_dir, _, _ = _write_folders(tmp_path, 'nerfpp', n_gt=10, gt_ext='jpg')
    Image.fromarray(np.zeros((12, 17, 3), np.uint8)).save(str(gt_dir / 'zzz_unrelated.png'))      # ignored while *.jpg exist
    gts, preds = E.select_files(str(gt_dir), str(pred_dir), 'nerfpp', 1)
    assert [os.path.basename(g) for g in gts] == ['frame_0009.jpg'] and [os.path.basename(p) for p in preds] == ['000000.png']


def test_eval_images_mismatch_errors(tmp_path):
    from PIL import Image
    from outdoor_nerf_depth_amd import eval_images as E
    gt_dir, pred_dir, _, preds = _write_folders(tmp_path, 'mipnerf360')
    calls = []
    Image.fromarray(preds[0]).save(str(pred_dir / 'color_003.png'))            # 4 predictions, 3 test frames
    with pytest.raises(E.EvalImagesError, match='3 ground-truth test frames .* 4 predictions'):
        E.evaluate(str(gt_dir), str(pred_dir), 'mipnerf360', 4, metrics_fn=_helper_fn(calls))
    os.remove(str(pred_dir / 'color_003.png'))
    Image.fromarray(np.zeros((12, 18, 3), np.uint8)).save(str(pred_dir / 'color_001.png'))
    with pytest.raises(E.EvalImagesError, match='12 x 17 .* 12 x 18'):
        E.evaluate(str(gt_dir), str(pred_dir), 'mipnerf360', 4, metrics_fn=_helper_fn(calls))
    with pytest.raises(E.EvalImagesError, match='split'):
        E.evaluate(str(gt_dir), str(pred_dir), 'mipnerf360', 0, metrics_fn=_helper_fn(calls))
    assert not calls and not (pred_dir / 'eval_ssim.txt').exists()

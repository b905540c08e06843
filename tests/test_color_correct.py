"""No GPU: the numpy helper of the colour correction (tests/color_correct_reference.py) against upstream's own
property test and closed forms; libcolorcc_hip.so's symbols, sizes and argument errors; the CLI flags and eval_images' file
selection and writing with a stand-in for the device call."""
import os
import re

import numpy as np
import pytest
import torch

from tests import color_correct_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------------ the helper
def test_helper_recovers_ccm_quadratic_and_shift():
    """upstream's tests/image_test.py:32-58 restated with numpy's generator (jax's PRNG is not available): ten 128 x 128 uniform
    [0.1, 0.9] images through a random colour matrix + quadratic term + shift are recovered at atol = rtol = 1e-5.  The target
    goes through the helper's uint8 input only where the test allows it: the helper takes float targets here via _float_ref."""
    rs = np.random.RandomState(0)
    for _ in range(10):
        im0 = rs.uniform(0.1, 0.9, (128, 128, 3))
        ccm_scale, shift, sq_mult = rs.randn() / 10, rs.randn() / 10, rs.randn() / 10
        ccm = np.eye(3) + rs.randn(3, 3) * ccm_scale
        im1 = np.clip((im0.reshape(-1, 3) @ ccm).reshape(im0.shape) + sq_mult * im0 ** 2 + shift, 0, 1)
        np.testing.assert_allclose(_float_ref(im0, im1), im1, atol=1e-5, rtol=1e-5)


def _float_ref(img, ref):
    """the helper's loop on a float64 target (upstream's signature): color_correct itself takes the uint8 ground truth"""
    x0, ref = np.asarray(img, np.float64).reshape(-1, 3), np.asarray(ref, np.float64).reshape(-1, 3)
    mask0, x = R.unclipped(x0), x0
    for _ in range(R.NUM_ITERS):
        a = R.features(x)
        w = np.stack([np.linalg.lstsq(np.where(m[:, None], a, 0.), np.where(m, ref[:, c], 0.), rcond=-1)[0]
                      for c, m in ((c, mask0[:, c] & R.unclipped(x[:, c]) & R.unclipped(ref[:, c])) for c in range(3))], -1)
        x = np.clip(a @ w, 0., 1.)
    return x.reshape(np.shape(img))


def test_helper_loop_is_the_float_loop_on_bytes():
    """color_correct(img, ref_u8) is _float_ref(img, ref_u8 / 255): the property test above pins the function the GPU tests use"""
    img, ref = R.gained_pair(40, 56, 3, noise=0.02)
    np.testing.assert_array_equal(R.color_correct(img, ref)[0], _float_ref(img.astype(np.float64), ref / 255.))


def test_helper_closed_forms():
    img, ref = R.gained_pair(48, 64, 1)
    same = (ref / 255.).astype(np.float32)                      # unclipped: natural_frame stays in [0.05, 0.95]
    assert R.unclipped(ref / 255.).all()
    out, _, counts = R.color_correct(same, ref)
    assert np.abs(out - ref / 255.).max() < 1e-6                # float32(byte / 255) is not byte / 255: the fit undoes it
    out64 = R.color_correct(ref / 255., ref)[0]
    assert np.abs(out64 - ref / 255.).max() < 1e-12 and (counts == 48 * 64).all()
    # a per-channel affine gain is undone
    gain, off = np.array([0.7, 1.2, 0.9]), np.array([0.02, -0.01, 0.03])
    out = R.color_correct(ref / 255. * gain + off, ref)[0]
    assert np.abs(out - ref / 255.).max() < 1e-10


def test_helper_ignores_saturated_values():
    img, ref = R.gained_pair(48, 64, 2, noise=0.01, saturate=0.1)
    _, w, counts = R.color_correct(img, ref)
    assert (counts < 48 * 64).all()
    sat_ref = ref == 255
    assert sat_ref.sum() > 50
    other = ref.copy()
    other[sat_ref] = 0                                          # still clipped: bytes 0 and 255 are the clipped ones
    np.testing.assert_array_equal(R.color_correct(img, other)[1], w)
    c = int(np.argmax((img > 1 - R.EPS).sum((0, 1))))          # the channel of img with most saturated values
    sat_img = img[..., c] > 1 - R.EPS                          # no row of channel c's system
    assert sat_img.sum() > 50
    moved = img.copy()
    moved[..., c][sat_img] = 0.0                                # another clipped value; the other channels' features do change
    w_moved = R.color_correct(moved, ref)[1]
    np.testing.assert_array_equal(w_moved[0][:, c], w[0][:, c])
    assert (w_moved[0][:, (c + 1) % 3] != w[0][:, (c + 1) % 3]).any()
    out, w1, c1 = R.color_correct(np.ones_like(img), ref)
    assert (out == 0).all() and (w1 == 0).all() and (c1 == 0).all()          # all saturated: a black frame


# ------------------------------------------------------------------------------------------------ the library without a GPU
def test_library_exports_every_declared_symbol():
    from outdoor_nerf_depth_amd import color_correct as P
    text = open(os.path.join(ROOT, 'include', 'colorcc_hip.h')).read()
    assert '#define COLORCC_ABI_VERSION 1' in text
    text = re.sub(r'/\*.*?\*/', '', text, flags=re.S)
    declared = set(re.findall(r'\b(colorcc_[a-z0-9_]+)\s*\(', text))
    assert declared == set(P.SYMBOLS) and len(declared) == 5
    lib = P.lib()
    for name in declared:
        assert getattr(lib, name) is not None
    assert lib.colorcc_abi_version() == P.ABI_VERSION == 1


def test_library_sizes_and_argument_errors_without_a_gpu():
    from outdoor_nerf_depth_amd import color_correct as P
    lib = P.lib()
    for n in (0, -3, 65536):
        assert lib.colorcc_workspace_bytes(n, 16, 16) == -1 and b'n_frames' in lib.colorcc_last_error()
        assert lib.colorcc_correct(None, n, 16, 16, None, None, 1, None, None, None, None) == 1 and b'n_frames' in lib.colorcc_last_error()
        assert lib.colorcc_normal_equations(None, n, 16, 16, None, None, None, None) == 1
    for H, W in ((0, 5), (5, 0), (-1, 4)):
        assert lib.colorcc_workspace_bytes(1, H, W) == -1 and b'H * W >= 1' in lib.colorcc_last_error()
        assert lib.colorcc_correct(None, 1, H, W, None, None, 1, None, None, None, None) == 1
        with pytest.raises(P.ColorCorrectError, match='H . W >= 1'):
            P.workspace_bytes(1, H, W)
    assert lib.colorcc_workspace_bytes(1, 1 << 15, (1 << 13) + 1) == -1 and b'2^28' in lib.colorcc_last_error()
    assert lib.colorcc_correct(None, 1, 8, 8, None, None, 1, None, None, None, None) == 1 and b'non-null' in lib.colorcc_last_error()
    assert lib.colorcc_normal_equations(None, 1, 8, 8, None, None, None, None) == 1 and b'non-null' in lib.colorcc_last_error()
    # weights [F, 5, 3, 10] + partials [F, 3, nwg, 66] + squared-error partials [F, nwg] float64, nwg = min(ceil(HW / 256), 64)
    size = lambda F, H, W: (8 * F * (150 + (3 * 66 + 1) * min(-(-H * W // 256), 64)) + 255) // 256 * 256
    for F, H, W in ((1, 1, 1), (1, 7, 7), (5, 37, 53), (30, 375, 1242)):
        assert P.workspace_bytes(F, H, W) == size(F, H, W)
    assert P.workspace_bytes(3, 375, 1242) - P.workspace_bytes(2, 375, 1242) == P.workspace_bytes(2, 375, 1242) - P.workspace_bytes(1, 375, 1242)


def test_color_correct_has_no_cpu_path():
    from outdoor_nerf_depth_amd import color_correct as P
    img, ref = torch.zeros((8, 8, 3)), torch.zeros((8, 8, 3), dtype=torch.uint8)
    with pytest.raises(P.ColorCorrectError, match='no CPU path'):
        P.color_correct(img, ref)
    with pytest.raises(P.ColorCorrectError, match='no CPU path'):
        P.color_correct_async(img, ref)
    with pytest.raises(P.ColorCorrectError, match='no CPU path'):
        P.normal_equations(img, ref)


# ------------------------------------------------------------------------------------------------ the CLIs
def test_cli_parsers_carry_the_flags():
    from outdoor_nerf_depth_amd import eval_images as E
    from outdoor_nerf_depth_amd import mip360_eval as ME
    a = ME.make_parser().parse_args(['--color_correct'])
    assert a.color_correct and not a.image_metrics and a.lpips_weights is None
    assert not ME.make_parser().parse_args([]).color_correct
    a = E.make_parser().parse_args(['--method', 'mipnerf360_cc'])
    assert a.method == 'mipnerf360_cc' and not a.color_correct
    assert E.make_parser().parse_args(['--color_correct']).color_correct


def _folders(tmp_path):
    from PIL import Image
    from tests.test_image_metrics import _write_folders
    gt_dir, pred_dir, test_gts, preds = _write_folders(tmp_path, 'mipnerf360', hw=(12, 17))
    ccs = [np.ascontiguousarray(255 - p) for p in preds]
    for k, c in enumerate(ccs):
        Image.fromarray(c).save(str(pred_dir / ('color_cc_%03d.png' % k)))
    return gt_dir, pred_dir, test_gts, preds, ccs


def test_select_files_separates_corrected_renders(tmp_path):
    from outdoor_nerf_depth_amd import eval_images as E
    gt_dir, pred_dir, test_gts, preds, ccs = _folders(tmp_path)
    base = lambda names: [os.path.basename(n) for n in names]
    gts, sel = E.select_files(str(gt_dir), str(pred_dir), 'mipnerf360', 4)            # a folder that holds both kinds
    assert base(sel) == ['color_%03d.png' % k for k in range(3)] and len(gts) == 3
    _, sel = E.select_files(str(gt_dir), str(pred_dir), 'mipnerf360_cc', 4)
    assert base(sel) == ['color_cc_%03d.png' % k for k in range(3)]
    for k, n in enumerate(sel):
        np.testing.assert_array_equal(E._imread_rgb(n), ccs[k])
    assert base([E.cc_name('/x/color_007.png'), E.cc_name('/x/000007.png')]) == ['color_cc_007.png', 'color_cc_000007.png']


def test_eval_images_color_correct_plumbing(tmp_path, capsys, monkeypatch):
    from outdoor_nerf_depth_amd import eval_images as E
    from tests import ssim_reference as S
    from tests.test_image_metrics import _write_folders
    gt_dir, pred_dir, test_gts, preds = _write_folders(tmp_path, 'mipnerf360', hw=(12, 17))
    seen = []

    def fake_cc(gts, ps):                                                         # the device call: no GPU on this host
        seen.append((len(gts), len(ps)))
        return [R.to_u8(R.color_correct(np.float32(p) / np.float32(255), g)[0]) for g, p in zip(gts, ps)]

    monkeypatch.setattr(E, 'device_color_correct', fake_cc)
    monkeypatch.setattr(E, 'device_image_metrics', lambda g, p: S.image_metrics(np.stack(g), np.stack(p)))
    argv = ['--gt_dir', str(gt_dir), '--pred_dir', str(pred_dir), '--method', 'mipnerf360', '--split', '4']
    E.main(argv)
    plain = set(os.listdir(str(pred_dir)))
    assert not [f for f in plain if '_cc' in f] and not seen
    E.main(argv + ['--color_correct'])
    assert seen == [(3, 3)]
    assert set(os.listdir(str(pred_dir))) == plain | {'color_cc_%03d.png' % k for k in range(3)} | {'eval_cc_psnr.txt', 'eval_cc_ssim.txt'}
    want_cc = fake_cc(test_gts, preds)
    for k in range(3):
        np.testing.assert_array_equal(E._imread_rgb(str(pred_dir / ('color_cc_%03d.png' % k))), want_cc[k])
    want_s, want_p = S.image_metrics(np.stack(test_gts), np.stack(want_cc))
    for name, want in (('eval_cc_psnr.txt', want_p), ('eval_cc_ssim.txt', want_s)):
        text = (pred_dir / name).read_text()
        vals = [float(v) for v in text.split('\n')]
        assert not text.endswith('\n') and vals[:-1] == [float(v) for v in want] and vals[-1] == sum(vals[:-1]) / 3
    assert 'cc_psnr = ' in capsys.readouterr().out
    # a second run of the plain method in the folder that now holds both kinds still finds its three predictions
    E.main(argv)
    # ... and the corrected files are scored on their own
    E.main(argv[:5] + ['mipnerf360_cc'] + argv[6:])
    assert [float(v) for v in (pred_dir / 'eval_psnr.txt').read_text().split('\n')][:-1] == [float(v) for v in want_p]
    with pytest.raises(E.EvalImagesError, match='colour-corrected already'):
        E.main(argv[:5] + ['mipnerf360_cc'] + argv[6:] + ['--color_correct'])
    # with LPIPS: the twin file of the corrected bytes
    got = E.evaluate(str(gt_dir), str(pred_dir), 'mipnerf360', 4, lpips_fn=lambda g, p: [0.5, 0.25, 0.75], cc_fn=fake_cc)
    assert got['cc_lpips'] == [0.5, 0.25, 0.75, 0.5] and (pred_dir / 'eval_cc_lpips.txt').exists()


def test_write_color_corrected_files(tmp_path, monkeypatch):
    """mip360_train.write_color_corrected with a stand-in for the device call: the file set and upstream's format of
    metric_cc_psnr (eval.py:287-289: single spaces, no mean)"""
    from outdoor_nerf_depth_amd import color_correct as P
    from outdoor_nerf_depth_amd import mip360_train as T
    pairs = [R.gained_pair(12, 17, s, noise=0.02) for s in (0, 1)]
    img, ref = np.stack([p[0] for p in pairs]), np.stack([p[1] for p in pairs])
    cc = np.stack([R.color_correct(i, r)[0] for i, r in zip(img, ref)])
    psnr = np.array([R.psnr_cc(c, r) for c, r in zip(cc, ref)])

    class Pending(object):
        tensors = {'cc_u8': R.to_u8(cc)}

        def get(self):
            return cc, R.to_u8(cc), psnr, None

    monkeypatch.setattr(P, 'color_correct_async', lambda i, r, q: Pending())
    got = T.write_color_corrected(str(tmp_path), 7, torch.from_numpy(ref), torch.from_numpy(img), True)
    assert set(os.listdir(str(tmp_path))) == {'color_cc_000.png', 'color_cc_001.png', 'metric_cc_psnr_7.txt'}
    text = (tmp_path / 'metric_cc_psnr_7.txt').read_text()
    assert text == ' '.join(str(float(v)) for v in psnr) and list(got) == list(psnr)
    from PIL import Image
    np.testing.assert_array_equal(np.array(Image.open(str(tmp_path / 'color_cc_001.png'))), R.to_u8(cc[1]))

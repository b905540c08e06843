"""GPU: libcolorcc_hip.so against the numpy helper tests/color_correct_reference.py (np.linalg.lstsq on the
full matrix), which is the yardstick; mip360_eval --color_correct and eval_images end to end on the small test scene.

Gates.  rgb_cc: 10 x the worst |device - helper| measured on the MI355X over well_conditioned_cases()
(profiles/r11_color_correct_error.json, tools/color_correct_bench.py), never above 1e-8.  Normal equations: 10 x the measured
relative error (relative to the sum of absolute products: both are float64 sums of the same terms), never above 1e-12.
psnr_cc: 1e-9 dB; where the helper's own mean squared error is below 1e-24 (rounding noise of an exact fit, a PSNR above
240 dB that no float64 sum defines to 1e-9 dB) the device's must be below 1e-24 too.
"""
import json
import os

import numpy as np
import pytest
import torch

from tests import color_correct_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu

MEASURED = json.load(open(os.path.join(ROOT, 'profiles', 'r11_color_correct_error.json')))
GATE = min(10 * MEASURED['worst_rgb_cc_abs_err'], 1e-8)
GATE_NE = min(10 * MEASURED['worst_normal_equations_rel_err'], 1e-12)
_helper = {}


def dev():
    if not torch.cuda.is_available():
        pytest.skip('needs a GPU')
    return torch.device('cuda:0')


def _P():
    from outdoor_nerf_depth_amd import color_correct as P
    return P


def up(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev())


def cases():
    if 'cases' not in _helper:
        _helper['cases'] = [(label, img, ref, R.color_correct(img, ref)) for label, img, ref in R.well_conditioned_cases()]
    return _helper['cases']


def _psnr_agrees(got, rgb_cc, ref, quantize, label):
    want = R.psnr_cc(rgb_cc, ref, quantize)
    q = np.round(rgb_cc * 255) / 255 if quantize else rgb_cc
    mse = ((q - ref / 255.) ** 2).mean()
    print(label, 'quantize', quantize, 'psnr_cc', got, 'helper', want)
    if mse < 1e-24:
        assert got > 240, (label, got, want)
    else:
        assert abs(got - want) <= 1e-9, (label, got, want)


def test_normal_equations_match_float64_sums():
    P = _P()
    assert 0 < GATE_NE <= 1e-12
    for label, img, ref, _ in cases():
        got = P.normal_equations(up(img), up(ref))
        want, mag = R.normal_equations(img, ref)
        assert got.shape == (1, 3, 66)
        err = (np.abs(got[0] - want) / np.maximum(mag, 1e-300)).max()
        print(label, 'normal equations: relative error', err, 'gate', GATE_NE)
        assert err <= GATE_NE, (label, err)
        np.testing.assert_array_equal(got[0, :, 65], want[:, 65])


def test_correct_matches_the_helper():
    P = _P()
    assert 0 < GATE <= 1e-8
    for label, img, ref, (want, _, counts) in cases():
        got, got_u8, psnr, got_counts = P.color_correct(up(img), up(ref), True)
        assert got.shape == (1,) + img.shape and got.dtype == np.float64 and got_u8.dtype == np.uint8
        err = np.abs(got[0] - want).max()
        n_diff, n_bad, n_near = R.byte_rule(got_u8[0], want)
        print(label, 'rgb_cc: worst abs error', err, 'gate', GATE, 'bytes differing', n_diff, 'of them outside the rule', n_bad,
              'helper values within 1e-6 of a byte edge', n_near)
        assert err <= GATE, (label, err)
        np.testing.assert_array_equal(got_counts[0], counts)
        assert n_bad == 0, '%s: %d bytes differ, %d outside the rule (%d helper values near a byte edge)' % (label, n_diff, n_bad, n_near)
        np.testing.assert_array_equal(got_u8[0], R.to_u8(got[0]))                   # the bytes are the device's own values, truncated
        _psnr_agrees(float(psnr[0]), want, ref, True, label)
        _psnr_agrees(float(P.color_correct(up(img), up(ref), False)[2][0]), want, ref, False, label)


def test_same_bits_twice_and_batch_of_five_is_five_single_calls():
    P = _P()
    pairs = [R.gained_pair(37, 53, 30 + s, noise=0.02, saturate=0.03 * (s % 2)) for s in range(4)] + [R.degenerate_cases(37, 53)[0][1:]]
    img, ref = up(np.stack([p[0] for p in pairs])), up(np.stack([p[1] for p in pairs]))
    a, b = P.color_correct(img, ref), P.color_correct(img, ref)
    singles = [P.color_correct(img[i], ref[i]) for i in range(5)]
    for k in range(4):
        assert a[k].tobytes() == b[k].tobytes()
        assert a[k].tobytes() == np.concatenate([s[k] for s in singles]).tobytes()
    big = R.well_conditioned_cases()[1]
    x, y = P.color_correct(up(big[1]), up(big[2])), P.color_correct(up(big[1]), up(big[2]))
    assert all(x[k].tobytes() == y[k].tobytes() for k in range(4))
    n1, n2 = P.normal_equations(up(big[1]), up(big[2])), P.normal_equations(up(big[1]), up(big[2]))
    assert n1.tobytes() == n2.tobytes()


def test_degenerate_frames_are_finite_reproducible_and_raise_nothing():
    P = _P()
    for label, img, ref in R.degenerate_cases():
        a, b = P.color_correct(up(img), up(ref)), P.color_correct(up(img), up(ref))
        assert np.isfinite(a[0]).all() and a[0].min() >= 0 and a[0].max() <= 1, label
        assert all(a[k].tobytes() == b[k].tobytes() for k in range(4)), label
        print(label, 'psnr_cc', a[2], 'mask counts', a[3][0, -1])
        if label == 'all saturated':
            assert (a[0] == 0).all() and (a[1] == 0).all() and (a[3] == 0).all()


def test_correction_undoes_exposure_and_white_balance():
    """the point of the feature: pred = clip(gt * gain + offset), per-channel gains in [0.6, 1.4]"""
    P = _P()
    for noise in (0.0, 0.02):
        img, ref = R.gained_pair(375, 1242, 40, noise=noise)
        plain = R.psnr_cc(np.clip(img.astype(np.float64), 0, 1), ref, True)
        psnr = float(P.color_correct(up(img), up(ref))[2][0])
        print('noise', noise, 'uncorrected', plain, 'corrected', psnr)
        assert psnr > plain + (15 if noise == 0.0 else 0)  # with sigma 0.02 noise the corrected PSNR is bounded near 30 dB: reported


def test_no_launch_without_the_flag(tmp_path, monkeypatch):
    """mip360_eval without --color_correct makes no call into libcolorcc_hip.so (and with it exactly one); the files, bytes and
    metric values of the flag against the helper on the very float32 frames that were rendered."""
    dev()
    import glob
    from PIL import Image
    from outdoor_nerf_depth_amd import color_correct as P
    from outdoor_nerf_depth_amd import eval_images as E
    from outdoor_nerf_depth_amd import mip360_eval as ME
    from outdoor_nerf_depth_amd import mip360_train as T
    from tests.test_gpu_image_metrics import _read_metric, _run
    from tests.test_mip360_scene import write_scene
    data, ckpt = tmp_path / 'scene', tmp_path / 'run'
    write_scene(str(data), n_frames=12, H=32, W=40)
    bind = lambda extra=(): sum([['--gin_bindings', x] for x in [
        "Config.data_dir = '%s'" % data, "Config.checkpoint_dir = '%s'" % ckpt, 'Config.max_steps = 4', 'Config.checkpoint_every = 4',
        'Config.print_every = 4', 'Config.batch_size = 1024', 'Config.lr_delay_steps = 0', "Config.depth_sup_type = 'mono_crop'",
        'Config.render_chunk_size = 1024', 'Config.sample_every = 1', 'Config.compute_disp_metrics = True',
        "Config.depth_loss_type = 'mse'"] + list(extra)], [])
    _run('mip360_train', bind())
    calls, frames = [], []

    class Spy(object):                                                         # counts calls through the ctypes handle
        def __init__(self, handle):
            self._h = handle

        def __getattr__(self, name):
            fn = getattr(self._h, name)
            if name in ('colorcc_correct', 'colorcc_normal_equations'):
                def counted(*a):
                    calls.append(name)
                    return fn(*a)
                return counted
            return fn

    monkeypatch.setattr(P, '_lib', Spy(P.lib()))
    real = T.write_color_corrected

    def recording(out_dir, step, gt_u8, rgb_f32, *a, **k):
        frames.append((gt_u8.cpu().numpy(), rgb_f32.cpu().numpy()))
        return real(out_dir, step, gt_u8, rgb_f32, *a, **k)

    monkeypatch.setattr(T, 'write_color_corrected', recording)
    ME.main(bind(["Config.eval_suffix = 'plain'"]))
    plain = set(os.listdir(str(ckpt / 'test_eval_preds_plain')))
    assert calls == [] and frames == [] and not [f for f in plain if '_cc' in f]
    assert 'metric_psnr_4.txt' in plain and 'color_000.png' in plain
    ME.main(bind(["Config.eval_suffix = 'cc'"]) + ['--color_correct'])
    d = ckpt / 'test_eval_preds_cc'
    assert calls == ['colorcc_correct'] and len(frames) == 1
    assert set(os.listdir(str(d))) == plain | {'color_cc_000.png', 'metric_cc_psnr_4.txt'}
    ME.main(bind(["Config.eval_suffix = 'ccim'"]) + ['--color_correct', '--image_metrics'])
    d2 = ckpt / 'test_eval_preds_ccim'
    assert set(os.listdir(str(d2))) == plain | {'color_cc_000.png', 'metric_cc_psnr_4.txt', 'metric_ssim_4.txt', 'metric_psnr8_4.txt',
                                                'metric_cc_ssim_4.txt', 'metric_cc_psnr8_4.txt'}
    gt, rgb = frames[0]
    assert gt.shape == rgb.shape == (1, 32, 40, 3) and rgb.dtype == np.float32
    np.testing.assert_array_equal(gt[0], np.array(Image.open(sorted(glob.glob(str(data / 'images' / '*.png')))[9])))
    png = np.array(Image.open(str(d / 'color_cc_000.png')))
    text = (d / 'metric_cc_psnr_4.txt').read_text()
    vals = [float(v) for v in text.split(' ')]
    assert len(vals) == 1 and '\n' not in text                                 # one test frame; single spaces, no mean
    want, _, counts = R.color_correct(rgb[0], gt[0])
    got, got_u8, psnr, got_counts = P.color_correct(up(rgb[0]), up(gt[0]), True)
    # Is the frame of this early checkpoint in the well-conditioned class?  The unit-diagonal Gram matrix of each channel's first
    # fit decides it: full rank and a condition number within 10 x that of the gated list (near 1e4, so below 1e5) -- the error
    # of the normal-equation route grows with that number, and the gate was measured at 1e4.  Otherwise only the weak conditions of
    # the degenerate class hold, plus the consistency of files and device values.  Which branch ran: the 4-step
    # fixture renders a dark, nearly grey 32 x 40 frame with condition 2.1e6; there the device is 1.4e-8 from the helper (measured
    # on the MI355X), so the weak branch runs.
    sums, _ = R.normal_equations(rgb[0], gt[0])
    conds = []
    for c in range(3):
        G = np.zeros((10, 10))
        G[np.triu_indices(10)] = sums[c, :55]
        G = G + np.triu(G, 1).T
        s = np.where(np.diag(G) > 0, 1 / np.sqrt(np.where(np.diag(G) > 0, np.diag(G), 1)), 1)
        lam = np.linalg.eigvalsh(G * s[:, None] * s[None, :])
        conds.append(lam.max() / lam.min() if lam.min() > 0 else np.inf)
    well = max(conds) < 1e5
    print('rendered frame: condition of the scaled Gram matrices', conds, '-> well-conditioned gate' if well else '-> weak conditions',
          'device vs helper', np.abs(got[0] - want).max(), 'mask counts', counts[-1])
    np.testing.assert_array_equal(png, got_u8[0])                              # the file holds the device's bytes
    assert vals[0] == float(psnr[0])
    if well:
        assert np.abs(got[0] - want).max() <= GATE
        np.testing.assert_array_equal(got_counts[0], counts)
        n_diff, n_bad, n_near = R.byte_rule(png, want)
        assert n_bad == 0, '%d bytes differ, %d outside the rule (%d helper values near a byte edge)' % (n_diff, n_bad, n_near)
        _psnr_agrees(vals[0], want, gt[0], True, 'mip360_eval')
    else:
        assert np.isfinite(got).all() and got.min() >= 0 and got.max() <= 1
        np.testing.assert_array_equal(png, R.to_u8(got[0]))
        assert abs(vals[0] - R.psnr_cc(got[0], gt[0], True)) <= 1e-9
    # eval_images on that folder: the corrected files scored on their own reproduce metric_cc_psnr8
    E.main(['--gt_dir', str(data / 'images'), '--pred_dir', str(d2), '--method', 'mipnerf360_cc', '--split', '1'])
    assert _read_metric(d2 / 'eval_psnr.txt') == _read_metric(d2 / 'metric_cc_psnr8_4.txt')
    assert _read_metric(d2 / 'eval_ssim.txt') == _read_metric(d2 / 'metric_cc_ssim_4.txt')
    # ... and --color_correct on the plain renders (byte / 255 as img) writes the corrected twins and their scores
    E.main(['--gt_dir', str(data / 'images'), '--pred_dir', str(ckpt / 'test_eval_preds_plain'), '--method', 'mipnerf360', '--split', '1',
            '--color_correct'])
    after = set(os.listdir(str(ckpt / 'test_eval_preds_plain')))
    assert after == plain | {'eval_psnr.txt', 'eval_ssim.txt', 'eval_cc_psnr.txt', 'eval_cc_ssim.txt', 'color_cc_000.png'}

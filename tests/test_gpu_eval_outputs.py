"""GPU: a list of frames of mixed sizes through eval_outputs.FrameBatches into each real library -- the one call pattern that
differs from one call per frame.  The scorers make one library call per frame size, and every frame's result equals, bit for bit,
a call on that frame alone.  Frames are the smallest the libraries accept."""
import numpy as np
import pytest
import torch

from tests import depth_metrics_reference as DR

pytestmark = pytest.mark.gpu


def dev():
    if not torch.cuda.is_available():
        pytest.skip('needs a GPU')
    return torch.device('cuda:0')


def up(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev())


def _count(monkeypatch, module, name):
    calls, real = [], getattr(module, name)

    def counted(*a, **k):
        calls.append(tuple(a[0].shape))
        return real(*a, **k)
    monkeypatch.setattr(module, name, counted)
    return calls


def _byte_pairs(shapes, seed):
    rs = np.random.RandomState(seed)
    gts = [rs.randint(0, 256, s + (3,)).astype(np.uint8) for s in shapes]
    preds = [np.clip(g + rs.normal(0, 12, g.shape), 0, 255).astype(np.uint8) for g in gts]
    return gts, preds


def test_image_metrics_of_mixed_sizes(monkeypatch):
    dev()
    from outdoor_nerf_depth_amd import eval_outputs as EO, image_metrics as IM
    gts, preds = _byte_pairs([(7, 7), (8, 9), (7, 7), (8, 9), (7, 7)], 0)
    calls = _count(monkeypatch, IM, 'image_metrics_async')
    got = EO.image_scores(gts, preds)
    assert calls == [(3, 7, 7, 3), (2, 8, 9, 3)]                                # one call per size
    for i, (g, p) in enumerate(zip(gts, preds)):
        ssim, psnr8 = IM.image_metrics(up(g), up(p))
        assert got['ssim'][i] == float(ssim[0]) and got['psnr8'][i] == float(psnr8[0]), i


def test_lpips_of_mixed_sizes(monkeypatch):
    dev()
    from outdoor_nerf_depth_amd import eval_outputs as EO, lpips as LP
    from tests.test_gpu_lpips import weights
    gts, preds = _byte_pairs([(16, 16), (17, 31), (16, 16)], 1)
    w = weights()[1]
    calls = _count(monkeypatch, LP, 'lpips_u8')
    got = EO.lpips_scores(gts, preds, w)['lpips']
    assert calls == [(2, 16, 16, 3), (1, 17, 31, 3)]
    np.testing.assert_array_equal(LP.lpips_u8_lists(gts, preds, w), got)        # the list form is the same call
    for i, (g, p) in enumerate(zip(gts, preds)):
        assert got[i] == float(LP.lpips_u8(up(g), up(p), w)[0][0]), i


def test_colour_correction_of_mixed_sizes(monkeypatch):
    dev()
    from outdoor_nerf_depth_amd import color_correct as CC, eval_outputs as EO
    gts, preds = _byte_pairs([(5, 7), (8, 9), (5, 7)], 2)
    imgs = [p.astype(np.float32) / np.float32(255) for p in preds]
    calls = _count(monkeypatch, CC, 'color_correct_async')
    cc_u8, psnr_cc, scores = EO.color_corrected(gts, imgs, True)
    assert calls == [(2, 5, 7, 3), (1, 8, 9, 3)] and scores == {}
    lists_u8, lists_psnr = CC.color_correct_u8_lists(gts, preds)                # eval_images' form: byte / 255 is the img
    for i, (g, img) in enumerate(zip(gts, imgs)):
        _, one_u8, one_psnr, _ = CC.color_correct(up(img), up(g), True)
        np.testing.assert_array_equal(cc_u8[i], one_u8[0])
        np.testing.assert_array_equal(lists_u8[i], one_u8[0])
        assert psnr_cc[i] == one_psnr[0] and lists_psnr[i] == one_psnr[0], i


def test_depth_metrics_of_mixed_sizes_and_scales(monkeypatch):
    dev()
    from outdoor_nerf_depth_amd import depth_metrics as DM, eval_outputs as EO
    shapes, scales = [(5, 7), (8, 9), (5, 7), (5, 7)], [0.0137, 0.0137, 0.0137, 0.31]
    frames = [DR.seeded_frames(s, scale, seed=k) for k, (s, scale) in enumerate(zip(shapes, scales))]
    preds, gts = [f[0][0] for f in frames], [f[1][0] for f in frames]
    calls = _count(monkeypatch, DM, 'depth_metrics_async')
    got = EO.depth_scores(preds, gts, scales)
    assert calls == [(2, 5, 7), (1, 8, 9), (1, 5, 7)]                           # one call per size and depth scale
    for i in range(len(shapes)):
        one = DM.depth_metrics(up(preds[i]), up(gts[i]), scales[i])
        for name in DM.METRIC_NAMES:
            np.testing.assert_array_equal(got[name][i], one[name][0], err_msg='%s frame %d' % (name, i))
    assert got['n_valid'][0] > 0

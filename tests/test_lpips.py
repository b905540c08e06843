"""CPU: the LPIPS statement in tests/lpips_reference.py against a second, independent statement and closed forms; the range
of the gated pairs; liblpips_hip.so's size queries, argument checks and symbol table without a GPU; load_weights; and the
plumbing of eval_images --lpips_weights with the metric function injected.
"""
import os
import re

import numpy as np
import pytest
import torch

from tests import lpips_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------------ the reference itself
def _conv_pool_tap_loops(x, w, b, lin):
    """conv 3 x 3 (zero padding 1) + bias + ReLU, 2 x 2 max-pool (floor), tap distance of images 0 and 1: explicit loops.
    x [2, H, W, Cin] float64 -> (pooled [2, H // 2, W // 2, Cout], d)"""
    n, H, W, cin = x.shape
    cout = w.shape[0]
    y = np.zeros((n, H, W, cout))
    for i in range(n):
        for r in range(H):
            for c in range(W):
                for o in range(cout):
                    s = float(b[o])
                    for ky in range(3):
                        for kx in range(3):
                            rr, cc = r + ky - 1, c + kx - 1
                            if 0 <= rr < H and 0 <= cc < W:
                                s += float(np.dot(x[i, rr, cc, :], w[o, :, ky, kx]))
                    y[i, r, c, o] = max(s, 0.0)
    pooled = np.zeros((n, H // 2, W // 2, cout))
    for r in range(H // 2):
        for c in range(W // 2):
            pooled[:, r, c, :] = y[:, 2 * r:2 * r + 2, 2 * c:2 * c + 2, :].reshape(n, 4, cout).max(axis=1)
    d = 0.0
    for r in range(H):
        for c in range(W):
            f0, f1 = y[0, r, c], y[1, r, c]
            n0, n1 = f0 / (np.sqrt((f0 * f0).sum()) + 1e-10), f1 / (np.sqrt((f1 * f1).sum()) + 1e-10)
            d += float((lin * (n0 - n1) ** 2).sum())
    return pooled, d / (H * W)


def test_reference_layer_matches_explicit_loops():
    rs = np.random.RandomState(0)
    H, W, cin, cout = 5, 7, 3, 4                                        # odd sizes: the pool drops the last row and column
    x = rs.standard_normal((2, H, W, cin))
    w, b, lin = rs.standard_normal((cout, cin, 3, 3)), rs.standard_normal(cout), rs.rand(cout)
    pooled, d = _conv_pool_tap_loops(x, w, b, lin)
    xt = torch.from_numpy(x).permute(0, 3, 1, 2)
    y = torch.nn.functional.relu(torch.nn.functional.conv2d(xt, torch.from_numpy(w), torch.from_numpy(b), padding=1))
    got_pool = torch.nn.functional.max_pool2d(y, 2, 2).permute(0, 2, 3, 1).numpy()
    assert got_pool.shape == (2, 2, 3, cout) and np.abs(got_pool - pooled).max() <= 1e-13
    got_d = float(R.tap_distance(y[0:1], y[1:2], torch.from_numpy(lin))[0])
    assert abs(got_d - d) <= 1e-13
    nhwc = R.conv3x3_relu_nhwc(x, w, b)
    assert np.abs(nhwc - y.permute(0, 2, 3, 1).numpy()).max() == 0


def test_reference_network_shape_and_taps():
    w = R.random_weights(1)
    taps = R.features(R.scale_input(np.zeros((1, 33, 50, 3), np.uint8), torch.float64), w, torch.float64)
    assert [tuple(t.shape[1:]) for t in taps] == [(64, 33, 50), (128, 16, 25), (256, 8, 12), (512, 4, 6), (512, 2, 3)]
    x = R.scale_input(np.array([[[[0, 255, 51]]]], np.uint8), torch.float64)[0, :, 0, 0].numpy()
    want = [(-1 + .030) / .458, (1 + .088) / .448, (51 / 255 * 2 - 1 + .188) / .450]
    assert np.abs(x - want).max() <= 1e-15


def test_closed_forms():
    # orthogonal unit vectors: n0 - n1 = e_0 - e_1 at every pixel, so d = w[0] + w[1]
    f0, f1 = torch.zeros(1, 4, 3, 5, dtype=torch.float64), torch.zeros(1, 4, 3, 5, dtype=torch.float64)
    f0[:, 0], f1[:, 1] = 1.0, 1.0
    lin = torch.tensor([0.25, 0.5, 7.0, 9.0], dtype=torch.float64)
    assert abs(float(R.tap_distance(f0, f1, lin)[0]) - 0.75) <= 1e-9           # (1 / (1 + 1e-10))^2 * 0.75
    # scale invariance of the normalisation: 3 e_0 against 5 e_1 gives the same
    assert abs(float(R.tap_distance(3 * f0, 5 * f1, lin)[0]) - 0.75) <= 1e-9
    # the 1e-10 sits outside the square root: an all-zero pixel is 0 / 1e-10 = 0, not NaN; against a unit vector it gives w[0]
    z = torch.zeros_like(f0)
    assert float(R.tap_distance(z, z, lin)[0]) == 0.0
    assert abs(float(R.tap_distance(f0, z, lin)[0]) - 0.25) <= 1e-9
    # identical images: exactly 0 in all six values
    w = R.random_weights(2)
    g = R.content('noise', 16, 19, np.random.RandomState(1))
    t, per = R.lpips(g, g.copy(), w)
    assert t[0] == 0.0 and (per == 0.0).all()
    t32, _ = R.lpips(g, g.copy(), w, torch.float32)
    assert t32[0] == 0.0


def test_gated_pairs_lie_in_the_papers_range():
    """the condition on the GPU tests' inputs: with LIN_SCALE the float64 totals of the strongly differing pairs lie in
    [0.05, 1.5]; pred = gt is 0; every pair is finite and non-negative"""
    w = R.random_weights(R.WEIGHT_SEED, R.LIN_SCALE)
    ranged = 0
    for H, W in ((16, 16), (17, 31), (64, 96)):
        for label, g, p in R.gated_pairs(H, W):
            t, per = R.lpips(g, p, w)
            c, k = label.split('/')[:2]
            print(label, t[0])
            assert np.isfinite(per).all() and (per >= 0).all()
            if k == 'same':
                assert t[0] == 0.0
            else:
                assert t[0] > 0
            if (c, k) in R.RANGED:
                assert R.RANGE[0] <= t[0] <= R.RANGE[1], label
                ranged += 1
    assert ranged == 3 * 7


# ------------------------------------------------------------------------------------------------ the library without a GPU
def test_library_sizes_and_argument_errors_without_a_gpu():
    from outdoor_nerf_depth_amd import lpips as P
    lib = P.lib()
    assert lib.lpips_abi_version() == P.ABI_VERSION == 1
    for H, W in ((15, 100), (100, 15), (0, 0)):
        assert lib.lpips_workspace_bytes(1, H, W) == -1 and b'H >= 16' in lib.lpips_last_error()
        assert lib.lpips_u8(None, 1, H, W, None, None, None, None, None) == 1 and b'H >= 16' in lib.lpips_last_error()
        with pytest.raises(P.LpipsError, match='H >= 16'):
            P.workspace_bytes(1, H, W)
    for n in (0, -3):
        assert lib.lpips_workspace_bytes(n, 16, 16) == -1 and b'n_pairs' in lib.lpips_last_error()
        assert lib.lpips_u8(None, n, 16, 16, None, None, None, None, None) == 1 and b'n_pairs' in lib.lpips_last_error()
    assert lib.lpips_u8(None, 1, 16, 16, None, None, None, None, None) == 1 and b'non-null' in lib.lpips_last_error()
    assert lib.lpips_pack_weights(None, None, None) == 1 and b'non-null' in lib.lpips_last_error()
    assert lib.lpips_packed_conv_floats(3, 64) == 32 * 64 and lib.lpips_packed_conv_floats(64, 128) == 576 * 128
    assert lib.lpips_packed_conv_floats(0, 64) == -1 and lib.lpips_packed_conv_floats(3, 65) == -1
    assert lib.lpips_conv3x3_relu(None, 1, 8, 8, 3, 65, None, None, None, None) == 1
    assert lib.lpips_conv3x3_relu(None, 1, 8, 8, 3, 64, None, None, None, None) == 1 and b'non-null' in lib.lpips_last_error()
    assert lib.lpips_pack_conv(None, 3, 64, None, None) == 1 and b'non-null' in lib.lpips_last_error()
    n_flat = sum(co * ci * 9 + co for ci, co in R.CONV_SHAPES) + sum(R.TAP_CHANNELS)
    assert lib.lpips_flat_floats() == n_flat
    n_packed = sum((9 * ci + 15) // 16 * 16 * co + co for ci, co in R.CONV_SHAPES) + sum(R.TAP_CHANNELS)
    assert lib.lpips_packed_bytes() == 4 * n_packed
    # two 64-channel full-resolution float32 maps for both images of every pair of a group + one float64 per tap workgroup
    blocks = lambda H, W: sum(((H >> l) * (W >> l) + 63) // 64 for l in range(5))
    assert P.workspace_bytes(1, 16, 16) == 2 * 2 * 16 * 16 * 64 * 4 + 256            # 8 partials, rounded up to 256 bytes
    per_pair = 2 * 375 * 1242 * 64 * 4
    group = (2 << 30) // (2 * per_pair)
    assert group == 4                                                                # the 2 GiB bound: pairs go four at a time
    want = 2 * group * per_pair + 30 * blocks(375, 1242) * 8
    assert P.workspace_bytes(30, 375, 1242) == (want + 255) // 256 * 256


def test_library_exports_every_declared_symbol():
    from outdoor_nerf_depth_amd import lpips as P
    text = open(os.path.join(ROOT, 'include', 'lpips_hip.h')).read()
    text = re.sub(r'/\*.*?\*/', '', text, flags=re.S)
    declared = set(re.findall(r'\b(lpips_[a-z0-9_]+)\s*\(', text))
    assert declared == set(P.SYMBOLS) and len(declared) == 10
    lib = P.lib()
    for name in declared:
        assert getattr(lib, name) is not None
    assert '#define LPIPS_ABI_VERSION 1' in open(os.path.join(ROOT, 'include', 'lpips_hip.h')).read()


def test_lpips_u8_has_no_cpu_path():
    from outdoor_nerf_depth_amd import lpips as P
    w = P.Weights(R.random_weights(0))
    a = torch.zeros((16, 16, 3), dtype=torch.uint8)
    with pytest.raises(P.LpipsError, match='no CPU path'):
        P.lpips_u8(a, a, w)
    with pytest.raises(P.LpipsError, match='lpips.Weights'):
        P.lpips_u8(a, a, {})


# ------------------------------------------------------------------------------------------------ load_weights
def test_load_weights_files_prefixes_and_errors(tmp_path):
    from outdoor_nerf_depth_amd import lpips as P
    w = R.random_weights(3)
    vgg = {k: v for k, v in w.items() if k.startswith('features')}
    lin = {k: v for k, v in w.items() if k.startswith('lin')}
    # two files: a torch state dict with the classifier still in it, and an .npz with the `net.`-less lin keys
    sd = {'module.' + k: torch.from_numpy(v) for k, v in vgg.items()}
    sd['module.classifier.0.weight'] = torch.zeros(2, 2)
    torch.save(sd, str(tmp_path / 'vgg16.pth'))
    np.savez(str(tmp_path / 'lin.npz'), **lin)
    got = P.load_weights('%s,%s' % (tmp_path / 'vgg16.pth', tmp_path / 'lin.npz'))
    assert set(got.tensors) == set(w) and all((got.tensors[k] == w[k]).all() for k in w)
    assert [k for k, _ in P.weight_keys()] == list(w)                               # the flat order is the reference's order
    assert got.flat().size == P.lib().lpips_flat_floats()
    # one file with everything, `net.` in front of the VGG keys as the lpips package's own module names them
    np.savez(str(tmp_path / 'all.npz'), **dict(lin, **{'net.' + k: v for k, v in vgg.items()}))
    assert set(P.load_weights([str(tmp_path / 'all.npz')]).tensors) == set(w)
    with pytest.raises(P.LpipsError, match=r"lin0\.model\.1\.weight.*missing"):
        P.load_weights(str(tmp_path / 'vgg16.pth'))
    bad = dict(w)
    bad['features.5.weight'] = np.zeros((128, 64, 3, 2), np.float32)
    np.savez(str(tmp_path / 'bad.npz'), **bad)
    with pytest.raises(P.LpipsError, match=r"features\.5\.weight.*\(128, 64, 3, 2\).*\(128, 64, 3, 3\)"):
        P.load_weights(str(tmp_path / 'bad.npz'))
    with pytest.raises(P.LpipsError, match='no such file'):
        P.load_weights(str(tmp_path / 'nothing.pth'))
    with pytest.raises(P.LpipsError, match='one or two files'):
        P.load_weights('a,b,c')


# ------------------------------------------------------------------------------------------------ eval_images --lpips_weights
def test_eval_images_lpips_plumbing(tmp_path, capsys, monkeypatch):
    from outdoor_nerf_depth_amd import eval_images as E
    from outdoor_nerf_depth_amd import lpips as P
    from tests import ssim_reference as S
    from tests.test_image_metrics import _write_folders
    gt_dir, pred_dir, test_gts, preds = _write_folders(tmp_path, 'mipnerf360', hw=(16, 21))
    w = R.random_weights(4)
    np.savez(str(tmp_path / 'w.npz'), **w)
    seen = []

    def fake_lists(gts, ps, weights, device=None):                                 # the device call: no GPU on this host
        seen.append(weights)
        return R.lpips(np.stack(gts), np.stack(ps), weights.tensors)[0]

    monkeypatch.setattr(P, 'lpips_u8_lists', fake_lists)
    monkeypatch.setattr(E, 'device_image_metrics', lambda g, p: S.image_metrics(np.stack(g), np.stack(p)))
    argv = ['--gt_dir', str(gt_dir), '--pred_dir', str(pred_dir), '--method', 'mipnerf360', '--split', '4']
    E.main(argv + ['--lpips_weights', str(tmp_path / 'w.npz')])
    assert len(seen) == 1 and isinstance(seen[0], P.Weights)
    text = (pred_dir / 'eval_lpips.txt').read_text()
    assert not text.endswith('\n')
    vals = [float(v) for v in text.split('\n')]
    want = [float(v) for v in R.lpips(np.stack(test_gts), np.stack(preds), w)[0]]
    assert vals[:-1] == want and vals[-1] == sum(want) / 3                          # per image, then the mean (utils/eval.py:93-95)
    out = capsys.readouterr().out
    assert 'eval_lpips.txt is not written' not in out and 'lpips = ' in out
    assert (pred_dir / 'eval_psnr.txt').exists() and (pred_dir / 'eval_ssim.txt').exists()
    # without the flag nothing changes
    os.remove(str(pred_dir / 'eval_lpips.txt'))
    E.main(argv)
    assert 'eval_lpips.txt is not written' in capsys.readouterr().out and not (pred_dir / 'eval_lpips.txt').exists()
    # the in-process form
    got = E.evaluate(str(gt_dir), str(pred_dir), 'mipnerf360', 4, metrics_fn=lambda g, p: S.image_metrics(np.stack(g), np.stack(p)),
                     lpips_fn=lambda g, p: [0.5, 0.25, 0.75])
    assert got['lpips'] == [0.5, 0.25, 0.75, 0.5]


def test_cli_parsers_carry_the_flag():
    from outdoor_nerf_depth_amd import ddp_train_nerf as T
    a = T.config_parser().parse_args(['--lpips_weights', 'a.pth,b.pth'])
    assert a.lpips_weights == 'a.pth,b.pth' and T.wants_image_pairs(a) and not a.image_metrics
    a = T.config_parser().parse_args([])
    assert a.lpips_weights is None and not T.wants_image_pairs(a) and T.load_lpips_weights(a) is None
    from outdoor_nerf_depth_amd import mip360_train as MT
    assert MT.load_lpips_weights(None) is None and 'metric_lpips_{step}.txt' in MT.LPIPS_WEIGHTS_HELP % 'metric_lpips_{step}.txt'

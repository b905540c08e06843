"""Host side of the depth pictures: the numpy helper tests/depth_vis_reference.py against matplotlib and numpy,
the colour tables in the kernel header against tests/golden/colormaps.npz, the size checks of libdepthvis_hip.so (which need no
GPU) and the three parsers' flag."""
import os
import re

import numpy as np
import pytest

from tests import depth_vis_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, 'outdoor_nerf_depth_amd', 'csrc', 'depthvis_kernels.h')


@pytest.mark.parametrize('name', ['turbo', 'jet'])
def test_table_lookup_is_matplotlibs(name):
    matplotlib = pytest.importorskip('matplotlib')
    rs = np.random.RandomState(0)
    x = np.concatenate([rs.uniform(-0.2, 1.2, 20000), [0., 1., np.nan], np.arange(257) / 256.]).astype(np.float32)
    ref = matplotlib.colormaps[name](x)[:, :3]
    got, _ = R.cmap_lookup(x, name)
    np.testing.assert_array_equal(got, ref)


@pytest.mark.parametrize('name', ['turbo', 'jet'])
def test_header_tables_are_the_golden_file(name):
    text = open(HEADER).read()
    m = re.search(r'#define DEPTHVIS_TABLE_%s \\\n((?:.*\\\n)*.*\n)' % name.upper(), text)
    assert m, name
    vals = np.array([float(v) for v in m.group(1).replace('\\', ' ').replace(',', ' ').split()])
    assert vals.shape == (768,)
    np.testing.assert_array_equal(vals.reshape(256, 3), R.TABLES[name])


def direct(value, weight, ps):
    """vis.weighted_percentile with numpy: argsort, cumsum, interp"""
    x, w = np.asarray(value, np.float32).reshape(-1), np.asarray(weight, np.float32).reshape(-1)
    order = np.argsort(x, kind='stable')
    x, w = x[order].astype(np.float64), w[order].astype(np.float64)
    cw = np.cumsum(w)
    return np.interp(np.array(ps, np.float64) * (cw[-1] / 100), cw, x)


@pytest.mark.parametrize('n', [1, 2, 63, 64, 65, 4097, 96 * 129])
def test_helper_percentiles_are_argsort_cumsum_interp(n):
    rs = np.random.RandomState(n)
    v = rs.uniform(0.1, 30., n).astype(np.float32)
    w = (1.0 - rs.rand(n)).astype(np.float32)
    dup = rs.choice(v[:max(1, n // 7)], n)
    wz = w.copy()
    wz[rs.rand(n) < 0.1] = 0
    vn, wn = v.copy(), w.copy()
    nan = rs.rand(n) < 0.15
    vn[nan], wn[nan] = np.nan, 0
    for value, weight in ((v, w), (dup, w), (v, wz), (vn, wn)):
        for ps in ((0.5, 99.5), (0., 100.), (50.,), (5., 25., 75., 95.)):
            np.testing.assert_array_equal(R.percentiles(value, weight, ps), direct(value, weight, ps))


def test_uniform_weights_are_positions_in_the_sorted_frame():
    """cw = 1 .. n: the percentile p sits at sorted position p n / 100 - 1, np.percentile's linear rule on a shifted axis"""
    rs = np.random.RandomState(3)
    n = 1000
    v = rs.normal(0, 5, n).astype(np.float32)
    xs = np.sort(v).astype(np.float64)
    ps = (10., 37.5, 50., 99.9)
    pos = np.array(ps) * n / 100 - 1
    want = np.interp(pos, np.arange(n), xs)
    np.testing.assert_allclose(R.percentiles(v, np.ones(n, np.float32), ps), want, rtol=1e-13)
    shifted = np.percentile(xs, 100 * pos / (n - 1))
    np.testing.assert_allclose(R.percentiles(v, np.ones(n, np.float32), ps), shifted, rtol=1e-12)


def test_a_single_weight_returns_its_value():
    """on the frame's smallest value, that is: q < cw[0] for every p < 100.  Anywhere else np.interp runs from the element in
    front of it (running sum 0) up to it, and the answer lies between the two, at the element's own value only in the limit."""
    rs = np.random.RandomState(4)
    v = rs.normal(0, 5, 500).astype(np.float32)
    w = np.zeros(500, np.float32)
    w[np.argmin(v)] = 0.37
    np.testing.assert_array_equal(R.percentiles(v, w, (0., 0.5, 50., 99.5)), np.full(4, np.float64(v.min())))
    np.testing.assert_array_equal(R.percentiles(v[:1], w[np.argmin(v)][None], (0., 50., 100.)), np.full(3, np.float64(v[0])))
    w = np.zeros(500, np.float32)
    w[123] = 0.37
    below = np.float64(v[v < v[123]].max())
    got = R.percentiles(v, w, (0.5, 50., 99.5, 100 * (1 - 2.0 ** -40)))
    assert np.all((got > below) & (got <= np.float64(v[123]))) and np.all(np.diff(got) > 0)
    np.testing.assert_allclose(got[:3], below + np.array([0.005, 0.5, 0.995]) * (np.float64(v[123]) - below), rtol=1e-12)
    np.testing.assert_allclose(got[3], np.float64(v[123]), rtol=1e-11)


def test_workspace_bytes_rejects_sizes_with_a_reason():
    from outdoor_nerf_depth_amd import depth_vis as D
    assert D.workspace_bytes(1, 1) > 0 and D.workspace_bytes(5, 1 << 22) % 256 == 0
    assert D.workspace_bytes(5, 96 * 129) == 5 * D.workspace_bytes(1, 96 * 129) or D.workspace_bytes(5, 96 * 129) > 0
    with pytest.raises(D.DepthVisError, match='at least one value'):
        D.workspace_bytes(1, 0)
    with pytest.raises(D.DepthVisError, match=r'2\^22'):
        D.workspace_bytes(1, (1 << 22) + 1)
    with pytest.raises(D.DepthVisError, match='n_frames'):
        D.workspace_bytes(0, 16)


def test_the_three_parsers_accept_the_flag():
    from outdoor_nerf_depth_amd import ddp_train_nerf, eval_images, mip360_eval
    assert mip360_eval.make_parser().parse_args(['--depth_vis']).depth_vis is True
    assert mip360_eval.make_parser().parse_args([]).depth_vis is False
    assert eval_images.make_parser().parse_args(['--depth_vis']).depth_vis is True
    assert eval_images.make_parser().parse_args([]).depth_vis is False
    base = ['--expname', 'x']
    assert ddp_train_nerf.config_parser().parse_args(base + ['--depth_vis']).depth_vis is True
    assert ddp_train_nerf.config_parser().parse_args(base).depth_vis is False


def test_matte_and_bytes():
    acc = np.zeros((17, 33), np.float32)
    b, fr = R.matte_rgb(np.zeros((17, 33, 3), np.float32), acc)
    assert not fr.any()
    assert b[0, 0, 0] == 204 and b[0, 8, 0] == 255 and b[8, 0, 0] == 255 and b[8, 8, 0] == 204 and b[16, 32, 0] == 204
    b, _ = R.matte_rgb(np.full((17, 33, 3), np.nan, np.float32), np.ones((17, 33), np.float32))
    assert not b.any()

"""The float64 gradient reference of tests/grad_reference64.py (CPU): chunking over rays changes nothing but float64 summation
order, and the result agrees with the pinned numpy oracle's closed-form float32 backward (O.nerf_backward) within the float32
noise tests/test_oracle_golden.py accepts between that backward and torch autograd."""
import numpy as np
import pytest

torch = pytest.importorskip('torch')

from oracle import nerfpp_oracle as O                                   # noqa: E402
from tests import grad_reference64 as R                                  # noqa: E402


def _case(n, S, mode, seed):
    from outdoor_nerf_depth_amd.synthetic import SyntheticKitti
    b = SyntheticKitti(depth_sup_type='mono_crop').random_batch(n, np.random.RandomState(seed))
    b['depth_sup'][::3] = 0.0
    rs = np.random.RandomState(seed + 1)
    far = O.intersect_sphere(b['ray_o'], b['ray_d'])
    fg, bg = O.coarse_depths(b['min_depth'], far, S)
    fg = O.perturb_samples(fg, rs.rand(n, S).astype(np.float32))
    bg = O.perturb_samples(bg, rs.rand(n, S).astype(np.float32))
    level = O.init_params_like_reference(1)[0]
    cache = {}
    ret = O.nerf_forward(level, b['ray_o'], b['ray_d'], far, fg, bg, cache=cache)
    _, _, _, g_rgb, g_depth, g_w = O.loss_and_grads(ret, fg, far, b['rgb'], b['depth_sup'], mode != 'rgbonly',
                                                    'mse' if mode == 'rgbonly' else mode, 0.1, 0.01)
    return level, b, far, fg, bg, cache, g_rgb, g_depth, g_w


@pytest.mark.parametrize('n,S,mode', [(9, 16, 'mse'), (6, 33, 'kl'), (5, 64, 'rgbonly')])
def test_chunked_float64_reference_equals_unchunked_and_matches_the_oracle(n, S, mode):
    level, b, far, fg, bg, cache, g_rgb, g_depth, g_w = _case(n, S, mode, 3 * n + S)
    args = (level, b['ray_o'], b['ray_d'], far, fg, bg, g_rgb, g_depth, g_w)
    whole = R.level_grads64(*args, chunk_rays=n)
    chunked = R.level_grads64(*args, chunk_rays=2)
    assert list(whole) == O.param_order()
    for k in O.param_order():
        assert whole[k].dtype == torch.float64 and tuple(whole[k].shape) == level[k].shape
        a, c = whole[k].numpy(), chunked[k].numpy()
        assert np.linalg.norm(a - c) <= 1e-12 * np.linalg.norm(a) + 1e-300, (k, np.linalg.norm(a - c) / np.linalg.norm(a))
        assert np.linalg.norm(a) > 0, k
    g_o = O.nerf_backward(cache, g_rgb, g_depth, g_w)
    for k, (rel, mx) in R.errors(g_o, whole).items():
        assert mx <= 0.2, (k, mx)
        assert rel <= 5e-2, (k, rel)
    # a gradient one ray short is visible to the same measure (the comparison is not vacuous)
    short = R.level_grads64(level, b['ray_o'][1:], b['ray_d'][1:], far[1:], fg[1:], bg[1:], g_rgb[1:], g_depth[1:],
                            None if g_w is None else g_w[1:])
    assert max(rel for rel, _ in R.errors(short, whole).values()) > 1e-3


def test_flat_to_dict_is_the_level_layout():
    from outdoor_nerf_depth_amd import _lib as L
    vec = np.arange(L.LEVEL_PARAMS, dtype=np.float64)
    d = R.flat_to_dict(vec)
    assert list(d) == O.param_order()
    level = O.init_params_like_reference(1)[0]
    assert all(d[k].shape == level[k].shape for k in d)
    assert np.array_equal(np.concatenate([v.reshape(-1) for v in d.values()]), vec)

"""GPU tests of the two weight-gradient branches of the MipNeRF-360 MLP backward (mip360.mlp_backward_fm) at the bench's rows:

* the deferred multi-layer launch (USE_DEFER_DW, NerfMLP; USE_MULTI_DW, fused PropMLP) and the per-layer launches agree within
  float32 summation noise, and each equals the float64 sum of the gradients of row subsets run on their own (every row's
  forward and dZ depend on that row only, so only the float32 order of the split-K sums differs);
* which branch runs depends on the shapes alone: a trainer whose torch.cuda.mem_get_info reports almost no free memory takes
  bit-identical steps (the branch used to follow the free memory, i.e. other processes, and with it the bits).

Subsets are whole 256-row tiles: a row count the fm kernels do not take runs the row-major kernels, which round the operands
at other places (tests/test_gpu_mip360_fm.py: 2-5 % apart on the NerfMLP), so no exact-sum identity holds across the two paths."""
import numpy as np
import pytest

torch = pytest.importorskip('torch')
pytestmark = pytest.mark.gpu

from oracle import mip360_oracle as O                                    # noqa: E402
from tests.test_gpu_mip360 import T, N, dev, _rays                       # noqa: E402

# float32 split-K summation noise, measured on MI355X (per tensor, relative to the largest tensor norm of the MLP's gradient):
# PropMLP 4.4e-7 between the branches, <= 4.3e-7 against the float64 subset sum
BRANCH_GATE = 1e-5
SUBSET_GATE = 1e-5


@pytest.fixture(scope='module')
def M():
    dev()
    from outdoor_nerf_depth_amd import mip360
    return mip360


def _case(which, n, S, seed=0):
    rs = np.random.RandomState(seed)
    cfg = O.PROP_CFG if which == 'prop' else O.NERF_CFG
    params = O.init_mlp_params(cfg, rs)
    params = [(w, (rs.randn(*b.shape) * 0.05).astype(np.float32)) for w, b in params]
    rays = _rays(rs, n)
    s = np.sort(rs.rand(n, S + 1), -1).astype(np.float32)
    _, s_to_t = O.construct_ray_warps('reciprocal', rays['near'], np.full((n, 1), 30., np.float32))
    tdist = s_to_t(s).astype(np.float32)
    g_d = rs.randn(n, S).astype(np.float32)
    g_c = rs.randn(n, S, 3).astype(np.float32) if which == 'nerf' else None
    return params, rays, tdist, g_d, g_c


def _grads(M, which, case, sl):
    """flat float32 gradient of one MLP forward + backward (fm path) over the rays `sl`"""
    params, rays, tdist, g_d, g_c = case
    mcfg = M.PROP_CFG if which == 'prop' else M.NERF_CFG
    W = mcfg['net_width']
    n, S = g_d[sl].shape
    rows = n * S
    assert rows % 256 == 0
    tm = M.TrainableMLP(params, mcfg, dev())
    buf = M.fm_buffer(rows, W + 512, dev())
    M.cast_encode_fm(T(tdist[sl]), T(rays['origins'][sl]), T(rays['directions'][sl]), T(rays['radii'][sl]),
                     T(O.pos_basis_t()), buf, W, W + 512)
    density, rgb, saved = M.mlp_forward_train_fm(tm, buf, rows, T(rays['viewdirs'][sl]), n, S)
    assert saved['fm']
    M.mlp_backward(tm, saved, rows, T(g_d[sl]).reshape(-1), None if g_c is None else T(g_c[sl]).reshape(-1, 3), [None, None])
    out = tm.grads.clone()
    spans = [(int(tm.offsets[2 * t]), int(tm.offsets[2 * t + 1]), int(tm.offsets[2 * t + 2])) for t in range(len(params))]
    del tm, buf, saved, density, rgb
    torch.cuda.empty_cache()
    return out, spans


def _worst(a, b, spans):
    """largest per-tensor |a - b|_2 over the largest tensor norm of b (kernels and biases separately)"""
    a, b = a.double(), b.double()
    scale = max(float(torch.linalg.norm(b[s:e])) for s0, s1, s2 in spans for s, e in ((s0, s1), (s1, s2)))
    return max(float(torch.linalg.norm(a[s:e] - b[s:e])) for s0, s1, s2 in spans for s, e in ((s0, s1), (s1, s2))) / scale


# NerfMLP: the bench's 4096 rays x 32 samples (131 072 rows, 1024 wide: the deferred launch keeps 1.9 GB of dZ alive);
# PropMLP: 4096 x 64 (262 144 rows, the fused 4 x 256 path with its multi-layer weight-gradient launch)
@pytest.mark.parametrize('which,n,S,flag', [('nerf', 4096, 32, 'USE_DEFER_DW'), ('prop', 4096, 64, 'USE_MULTI_DW')])
def test_weight_gradient_branches_agree_and_equal_subset_sums(M, monkeypatch, which, n, S, flag):
    case = _case(which, n, S)
    if which == 'nerf':
        mcfg = M.NERF_CFG
        assert M.defer_dw_fits(dev(), n * S, mcfg['net_width'], mcfg['net_depth']), 'the bench shape takes the deferred launch'
    else:
        assert M.fused_prop_ok(M.PROP_CFG, n * S)
    res = {}
    for on in (True, False):
        monkeypatch.setattr(M, flag, on)
        res[on], spans = _grads(M, which, case, slice(0, n))
    assert bool(torch.isfinite(res[True]).all()) and float(res[True].abs().max()) > 0
    d_branch = _worst(res[False], res[True], spans)
    monkeypatch.setattr(M, flag, True)
    # subsets: 8 x 32 rays (one 256-row tile at S = 32), then uneven multiples of 256 rows
    cuts = [0, 8, 40, 1000, 2504, n] if S == 32 else [0, 4, 36, 1000, 2500, n]
    total = torch.zeros_like(res[True], dtype=torch.float64)
    for a, b in zip(cuts[:-1], cuts[1:]):
        total += _grads(M, which, case, slice(a, b))[0].double()
    d_sub = {on: _worst(res[on], total, spans) for on in (True, False)}
    print('\n%s %d x %d: branches %.3e, vs float64 subset sum: deferred %.3e, per-layer %.3e' % (
        which, n, S, d_branch, d_sub[True], d_sub[False]))
    assert d_branch <= BRANCH_GATE, d_branch
    assert d_sub[True] <= SUBSET_GATE and d_sub[False] <= SUBSET_GATE, d_sub
    # negative control: the same comparison with one 256-row tile left out of the subsets fails the gate
    short = total - _grads(M, which, case, slice(0, 256 // S))[0].double()
    assert _worst(res[True], short, spans) > SUBSET_GATE


def test_trainer_steps_do_not_depend_on_free_memory(M, monkeypatch):
    """Mip360Trainer steps with torch.cuda.mem_get_info reporting 1 MiB free are bit-identical to unpatched ones: the deferred
    weight-gradient launch is chosen from the shapes (mip360.defer_dw_fits), so a resumed run repeats the original."""
    rs = np.random.RandomState(4)
    n = 256                                            # 8192 NerfMLP rows: fm path, deferred launch
    rays = {k: T(v) for k, v in _rays(rs, n).items()}
    gt = T(rs.rand(n, 3).astype(np.float32))
    sup = T((0.5 + rs.rand(n)).astype(np.float32))
    jit = [[T(np.random.RandomState(10 * s + l).rand(n).astype(np.float32)) for l in range(3)] for s in range(3)]
    total = torch.cuda.get_device_properties(dev()).total_memory
    finals = []
    for starved in (False, True):
        if starved:
            monkeypatch.setattr(torch.cuda, 'mem_get_info', lambda device=None: (1 << 20, total))
        prs = np.random.RandomState(7)
        tr = M.Mip360Trainer(O.init_mlp_params(O.PROP_CFG, prs), O.init_mlp_params(O.NERF_CFG, prs), dev(), max_steps=1000)
        for s in range(3):
            tr.train_step(rays, gt, sup, jitter01=jit[s])
        tr.flush()
        finals.append([N(t) for t in (tr.nerf.flat, tr.prop.flat, tr.nerf.mu, tr.nerf.nu)])
    assert M.USE_DEFER_DW
    for a, b in zip(*finals):
        np.testing.assert_array_equal(a, b)

"""CPU (no GPU): the scale-and-shift-invariant depth loss -- the numpy reference (tests/depth_ssi_reference.py) against
torch float64 autograd through the least-squares solve, the properties the loss is named for, the groups that are not fitted, the
configuration surface of both training paths, and libdepthssi_hip.so's symbols, workspace query and argument checks (all made before
any device call)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from tests import depth_ssi_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def draw(seed, n, G, supervised=0.7):
    """float32 rendered depth, prior (about 30 % unsupervised) and group ids: every group's prior is its own affine map of the
    depth plus noise, so the fits differ from group to group"""
    rs = np.random.RandomState(seed)
    g = rs.randint(0, G, n).astype(np.int32)
    d = rs.uniform(1.0, 6.0, n).astype(np.float32)
    a, b = rs.uniform(0.5, 2.0, G), rs.uniform(-1.0, 1.0, G)
    p = (a[g] * d + b[g] + 0.2 * rs.randn(n)).astype(np.float32)
    p = np.where(p > 0, p, np.float32(0.5))
    p[rs.rand(n) >= supervised] = 0
    return d, p.astype(np.float32), g


# ------------------------------------------------------------------------------------------------ gradient
@pytest.mark.parametrize('norm', R.NORMS)
@pytest.mark.parametrize('n,G', [(7, 1), (257, 3), (4096, 37)])
def test_reference_gradient_matches_autograd_through_lstsq(n, G, norm):
    """The closed form 2 w r / D against torch float64 autograd through torch.linalg.lstsq: w and q minimise the sum, so their
    derivatives drop out"""
    torch = pytest.importorskip('torch')
    d, p, g = draw(n * 10 + G, n, G)
    min_rays = 3
    ref = R.ssi(d, p, g, G, min_rays, norm)
    assert ref['fit'][:, 3].any() and ref['value'] > 0
    td = torch.from_numpy(d.astype(np.float64)).requires_grad_()
    tp = torch.from_numpy(p.astype(np.float64))
    total = torch.zeros((), dtype=torch.float64)
    for k in range(G):
        if not ref['fit'][k, 3]:
            continue
        idx = torch.from_numpy(np.flatnonzero((p > 0) & (g == k)))
        A = torch.stack([td[idx], torch.ones(len(idx), dtype=torch.float64)], 1)
        wq = torch.linalg.lstsq(A, tp[idx, None]).solution
        np.testing.assert_allclose(wq.detach().numpy()[:, 0], ref['fit'][k, :2], rtol=1e-9, atol=1e-11)
        total = total + ((A @ wq)[:, 0] - tp[idx]).pow(2).sum()
    value = total / ref['D']
    value.backward()
    got, want = ref['grad'], td.grad.numpy()
    err = np.abs(got - want).max()
    print('n = %d, G = %d, norm %s: max |closed form - autograd| = %.3e (max |grad| %.3e)' % (n, G, norm, err, np.abs(want).max()))
    np.testing.assert_allclose(ref['value'], float(value.detach()), rtol=1e-12)
    assert err <= 1e-10
    assert (got[~ref['touched']] == 0).all() and (want[~ref['touched']] == 0).all()


def test_normalisers():
    d, p, g = draw(1, 300, 4)
    a, s = R.ssi(d, p, g, 4, 8, 'all'), R.ssi(d, p, g, 4, 8, 'supervised')
    n_sup = float((p > 0).sum())
    assert a['D'] == 300 and s['D'] == n_sup and a['stats'][0] == n_sup
    np.testing.assert_allclose(a['value'] * 300, s['value'] * n_sup, rtol=1e-13)
    none = R.ssi(d, np.zeros_like(p), g, 4, 8, 'supervised')                # no supervised ray: 0 with no gradient, not NaN
    assert none['value'] == 0 and none['D'] == 1 and not none['grad'].any() and not none['touched'].any()


# ------------------------------------------------------------------------------------------------ properties
@pytest.mark.parametrize('norm', R.NORMS)
def test_invariant_to_scale_and_shift_of_the_render(norm):
    d, p, g = draw(2, 500, 5)
    d64 = d.astype(np.float64)
    base = R.ssi(d64, p, g, 5, 8, norm)
    for a, b in ((3.0, 0.0), (0.25, 7.0), (-1.5, 2.0), (1.0, -0.75)):
        v = R.ssi(a * d64 + b, p, g, 5, 8, norm)
        np.testing.assert_allclose(v['value'], base['value'], rtol=1e-9)
        np.testing.assert_allclose(v['fit'][:, 0] * a, base['fit'][:, 0], rtol=1e-9)
        np.testing.assert_allclose(v['grad'] * a, base['grad'], rtol=1e-7, atol=1e-12)


@pytest.mark.parametrize('norm', R.NORMS)
def test_scale_and_shift_of_the_prior_scale_the_loss_by_a_squared(norm):
    d, p, g = draw(3, 500, 5)
    p64 = p.astype(np.float64)
    base = R.ssi(d, p64, g, 5, 8, norm)
    for a, b in ((2.0, 0.0), (0.5, 3.0), (1.0, 1.25)):                      # (positive maps: the supervised set is p > 0)
        q = np.where(p64 > 0, a * p64 + b, 0.0)
        np.testing.assert_allclose(R.ssi(d, q, g, 5, 8, norm)['value'], a * a * base['value'], rtol=1e-9)


@pytest.mark.parametrize('norm', R.NORMS)
def test_never_exceeds_mse_on_the_same_inputs(norm):
    for seed in range(5):
        d, p, g = draw(10 + seed, 400, 6)
        v = R.ssi(d, p, g, 6, 8, norm)
        m = p > 0
        mse_sum = ((d.astype(np.float64) - p.astype(np.float64))[m] ** 2).sum()
        assert 0 < v['D'] * v['value'] <= mse_sum


# ------------------------------------------------------------------------------------------------ groups that are not fitted
def test_unfitted_groups_contribute_nothing():
    """group 1 has fewer than min_rays supervised rays, group 2 a render that is exactly constant, group 3 no supervised ray; a
    collapsed render earns nothing"""
    d, p, g = draw(4, 600, 5)
    few = np.flatnonzero((g == 1) & (p > 0))
    p[few[5:]] = 0
    d[g == 2] = np.float32(3.7)
    p[g == 3] = 0
    v = R.ssi(d, p, g, 5, 8, 'all')
    np.testing.assert_array_equal(v['fit'][:, 3], [1, 0, 0, 0, 1])
    assert v['fit'][1, 2] == 5 and v['fit'][2, 2] > 8 and v['fit'][3, 2] == 0
    assert not v['touched'][np.isin(g, (1, 2, 3))].any() and not v['grad'][np.isin(g, (1, 2, 3))].any()
    keep = np.isin(g, (0, 4))
    alone = R.ssi(d[keep], p[keep], g[keep], 5, 8, 'all')
    np.testing.assert_allclose(v['value'] * 600, alone['value'] * keep.sum(), rtol=1e-13)
    assert v['stats'][1] == v['fit'][[0, 4], 2].sum() and v['stats'][0] == (p > 0).sum()
    flat = R.ssi(np.full(600, 2.5, np.float32), p, g, 5, 8, 'all')           # a collapsed render
    assert flat['value'] == 0 and not flat['fit'][:, 3].any() and not flat['grad'].any()
    assert R.ssi(d, p, g, 5, 1000, 'all')['value'] == 0                      # min_rays above every group


def test_ids_outside_the_groups_are_unsupervised():
    d, p, g = draw(5, 300, 3)
    g2 = g.copy()
    out = np.arange(300) % 7 == 0
    g2[out] = np.where(np.arange(300)[out] % 2 == 0, -1, 3)
    p_off = p.copy()
    p_off[out] = 0
    a, b = R.ssi(d, p, g2, 3, 8, 'supervised'), R.ssi(d, p_off, g, 3, 8, 'supervised')
    assert (p[out] > 0).any() and a['stats'][0] == b['stats'][0] == ((p > 0) & ~out).sum()
    assert a['value'] == b['value'] and (a['grad'] == b['grad']).all() and not a['touched'][out].any()


# ------------------------------------------------------------------------------------------------ configuration
def test_gin_accepts_the_type_and_the_key():
    from outdoor_nerf_depth_amd import mip360_data as D
    cfg = D.parse_gin(bindings=[])
    assert cfg['depth_ssi_min_rays'] == 8 and D.CONFIG_DEFAULTS['depth_ssi_min_rays'] == 8
    cfg = D.parse_gin(bindings=["Config.depth_loss_type = 'ssi'", 'Config.depth_ssi_min_rays = 12'])
    assert cfg['depth_loss_type'] == 'ssi' and cfg['depth_ssi_min_rays'] == 12
    from outdoor_nerf_depth_amd import mip360 as M
    assert M.SSI == 'ssi' and 'ssi' in M.DEPTH_LOSS_TYPES and set(M.DEPTH_TYPES) < set(M.DEPTH_LOSS_TYPES)
    assert 'ssi' not in M.DEPTH_TYPES                     # no code of libmip360_hip.so: the loss lives in its own library


def test_nerfpp_cli_flags():
    from outdoor_nerf_depth_amd import ddp_train_nerf as T
    a = T.config_parser().parse_args(['--expname', 'x', '--use_depth', '--depth_loss_type', 'ssi', '--depth_ssi_min_rays', '5'])
    assert a.depth_loss_type == 'ssi' and a.depth_ssi_min_rays == 5
    T.validate_args(a)
    assert T.config_parser().parse_args(['--expname', 'x']).depth_ssi_min_rays == 8


def test_nerfpp_trainer_rejects_the_two_combinations():
    """both raise when the trainer is built, before anything touches a device, and name both options"""
    from outdoor_nerf_depth_amd.trainer import NerfppTrainer
    with pytest.raises(ValueError, match=r"'ssi' and fuse_loss"):
        NerfppTrainer('cpu', depth_loss_type='ssi', fuse_loss=True)
    with pytest.raises(ValueError, match=r"'ssi' and optim_autoexpo"):
        NerfppTrainer('cpu', depth_loss_type='ssi', optim_autoexpo=True, img_names=['a'])
    with pytest.raises(ValueError, match='depth_ssi_min_rays'):
        NerfppTrainer('cpu', depth_loss_type='ssi', depth_ssi_min_rays=0)
    with pytest.raises(ValueError, match="ssi is this implementation's"):
        NerfppTrainer('cpu', depth_loss_type='huber')


def test_argument_errors_name_the_tensor():
    torch = pytest.importorskip('torch')
    from outdoor_nerf_depth_amd import depth_ssi as S
    x = torch.zeros(8)
    with pytest.raises(S.DepthSsiError, match=r'pred_levels\[0\]: expected a CUDA/HIP'):
        S.ssi_loss([x], x)
    with pytest.raises(S.DepthSsiError, match='pred_levels: 0 levels'):
        S.ssi_loss([], x)
    with pytest.raises(S.DepthSsiError, match='pred_levels: 9 levels'):
        S.ssi_loss([x] * 9, x)


def test_nothing_imports_the_binding_until_ssi_is_used():
    """a fresh interpreter that imports both trainers, both training CLIs and the benchmark has not imported depth_ssi: the library
    is mapped by the first ssi step only"""
    import subprocess
    import sys
    code = ('import sys; import bench; import outdoor_nerf_depth_amd.trainer, outdoor_nerf_depth_amd.mip360, '
            'outdoor_nerf_depth_amd.mip360_train, outdoor_nerf_depth_amd.ddp_train_nerf; '
            "assert 'outdoor_nerf_depth_amd.depth_ssi' not in sys.modules; print('clean')")
    out = subprocess.run([sys.executable, '-c', code], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and 'clean' in out.stdout, out.stdout[-1000:] + out.stderr[-2000:]


# ------------------------------------------------------------------------------------------------ header, bindings, validation
def test_header_and_bindings_agree():
    from outdoor_nerf_depth_amd import depth_ssi as S
    text = open(os.path.join(ROOT, 'include', 'depthssi_hip.h')).read()
    declared = set(re.findall(r'\b(depthssi_\w+)\(', text))
    assert declared == set(S.SYMBOLS) and len(declared) == 4
    for name, value in (('ABI_VERSION', S.ABI_VERSION), ('MAX_GROUPS', S.MAX_GROUPS), ('MAX_LEVELS', S.MAX_LEVELS),
                        ('NORM_ALL', S.NORMS['all']), ('NORM_SUPERVISED', S.NORMS['supervised'])):
        assert re.search(r'#define DEPTHSSI_%s %d\b' % (name, value), text), name
    assert re.search(r'#define DEPTHSSI_MAX_RAYS \(1 << 20\)', text) and S.MAX_RAYS == 1 << 20
    assert S.lib().depthssi_abi_version() == S.ABI_VERSION == 1


def test_workspace_query_answers_without_a_device():
    from outdoor_nerf_depth_amd import depth_ssi as S
    assert S.workspace_bytes(1, 1) == 256
    for L, G in ((3, 37), (8, 65535), (2, 280)):
        b = S.workspace_bytes(L, G)
        assert b % 256 == 0 and 0 <= b - 8 * (L * G + L) < 256
    for L, G, what in ((0, 1, 'n_levels = 0'), (9, 1, 'n_levels = 9'), (1, 0, 'n_groups = 0'), (1, 65536, 'n_groups = 65536')):
        with pytest.raises(S.DepthSsiError, match=what):
            S.workspace_bytes(L, G)


def test_entry_point_validates_arguments_without_a_device():
    from outdoor_nerf_depth_amd import depth_ssi as S
    lib = S.lib()
    d = 256                                                    # a non-null, aligned value no failing call dereferences
    names = ['stream', 'n', 'n_levels', 'd', 'p', 'g', 'g_stride', 'n_groups', 'min_rays', 'norm', 'scale', 'grads', 'workspace',
             'values', 'fit', 'stats', 'fold_total', 'fold_last', 'fold_others', 'fold_n_sup']
    ptrs = lambda *v: (C.c_void_p * 3)(*v)
    ok = [None, 4096, 3, ptrs(d, d, d), d, d, 3, 37, 8, 0, (C.c_float * 3)(1, 1, 1), ptrs(d, 2 * d, 3 * d), d, d, d, d, None, None,
          None, None]

    def call(**kw):
        a = list(ok)
        for k, v in kw.items():
            a[names.index(k)] = v
        return lib.depthssi_levels(*a)
    err = lambda: lib.depthssi_last_error()
    for n in (0, -1, (1 << 20) + 1):
        assert call(n=n) == 1 and b'expected 1 .. 2^20 rays' in err(), n
    for G in (0, 65536):
        assert call(n_groups=G) == 1 and b'n_groups = %d, expected 1 .. 65535' % G in err(), G
    for L in (0, 9):
        assert call(n_levels=L) == 1 and b'n_levels = %d, expected 1 .. 8' % L in err(), L
    assert call(min_rays=0) == 1 and b'min_rays = 0' in err()
    assert call(norm=2) == 1 and b'norm = 2' in err()
    for ptr in ('d', 'p', 'scale', 'workspace', 'values', 'fit', 'stats'):
        assert call(**{ptr: None}) == 1 and b'non-null' in err(), ptr
    assert call(d=ptrs(d, None, d)) == 1 and b'd[1] is null' in err()
    assert call(d=ptrs(d, d, d + 2)) == 1 and b'd[2] is null or not aligned' in err()
    assert call(g=None) == 1 and b'n_groups = 37 without group ids' in err()
    assert call(g_stride=0) == 1 and b'g_stride = 0' in err()
    assert call(workspace=d + 8) == 1 and b'workspace aligned to 256' in err()
    assert call(scale=(C.c_float * 3)(1, float('nan'), 1)) == 1 and b'scale[1]' in err()
    assert call(grads=ptrs(d, 2 * d, d)) == 1 and b'grads[0] and grads[2] are the same buffer' in err()
    assert call(fold_last=d + 1) == 1 and b'the folds aligned to 4' in err()

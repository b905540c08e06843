"""CPU (no GPU): the distortion and opacity regularisers of the NeRF++ path -- the numpy reference
(tests/ray_reg_reference.py) against the oracle's pairwise distortion loss and against central differences, the case generator, the
configuration surface of the trainer and its CLI, and librayreg_hip.so's symbols, workspace query and argument checks (all made
before any device call)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from tests import ray_reg_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------------ reference
@pytest.mark.parametrize('S', [1, 2, 5, 64, 192])
def test_prefix_form_matches_the_pairwise_oracle(S):
    """On the normalised edges, the prefix form against oracle.mip360_oracle.lossfun_distortion and lossfun_distortion_grad_w
    (pairwise, float64): 1e-12 relative to the sum of the absolute values of the terms (the weights are not negative, so that is
    the value itself; for a gradient entry it is grad_abs)."""
    from oracle import mip360_oracle as O
    c = R.draw(10 + S, 7, S)
    ref = R.ray_reg(c['w'], c['z'], c['lo'], c['hi'], 1.0, 0.0)
    e, valid = R.edges(c['z'], c['lo'], c['hi'])
    w = c['w'].astype(np.float64)
    n = len(valid)
    assert valid.sum() == n - 1 and (S < 2 or (np.diff(c['z'][R.TIED]) == 0).any())
    want = np.where(valid, O.lossfun_distortion(e, w), 0.0)
    want_g = valid[:, None] * O.lossfun_distortion_grad_w(e, w) / n
    err_v = np.abs(ref['dist'] - want).max() / max(np.abs(want).max(), 1e-300)
    err_g = (np.abs(ref['grad'] - want_g) / np.maximum(ref['grad_abs'], 1e-300)).max()
    err_p = np.abs(R.pairwise(e, w) * valid - want).max()
    print('S = %d: value %.3e relative, gradient %.3e of its terms, own pairwise form %.3e' % (S, err_v, err_g, err_p))
    assert err_v <= 1e-12 and err_g <= 1e-12 and err_p <= 1e-12
    assert ref['values'][0] == ref['dist'].sum() / n and ref['values'][1] == 0 and not ref['opac'].any()
    assert not ref['grad'][~valid].any() and ref['stats'][0] == n - 1


@pytest.mark.parametrize('S', [1, 5, 64])
def test_gradients_match_central_differences(S):
    """Both terms are checked by themselves.  The distortion is a quadratic form in w, so a central difference has no truncation
    error; the opacity's is h^2 f''' / 6 = h^2 / (6 o^2), doubled for f''' within the step.  Rounding of the two values:
    8 * 2^-53 * max(|value|, 1) / h.  Rays with o < 1e-3 (the all-zero weights among them) are left out of the opacity check: the
    step h = 1e-6 has to stay small against o."""
    c = R.draw(20 + S, 5, S)
    w = c['w'].astype(np.float64)
    n, h, worst = 5, 1e-6, 0.0
    for ld, lo_, key in ((1.0, 0.0, 'dist'), (0.0, 1.0, 'opac')):
        f = lambda ww: R.ray_reg(ww, c['z'], c['lo'], c['hi'], ld, lo_)
        ref = f(w)
        for r in range(n):
            if key == 'opac' and w[r].sum() < 1e-3:
                continue
            for s in sorted({0, S // 2, S - 1}):
                e = np.zeros_like(w)
                e[r, s] = h
                fd = (f(w + e)[key][r] - f(w - e)[key][r]) / (2 * h)
                o = w[r].sum() + R.OPAC_EPS
                tol = 8 * 2.0 ** -53 * max(abs(ref[key][r]), 1.0) / h + (h * h / (3 * o * o) if key == 'opac' else 0.0)
                worst = max(worst, abs(fd - n * ref['grad'][r, s]) / tol)
    print('S = %d: worst difference to central differences at %.3f of its bound' % (S, worst))
    assert worst <= 1.0


def test_generator_plants_the_four_rays():
    for S in (1, 2, 63, 1024):
        c = R.draw(S, 3, S)
        ref = R.ray_reg(c['w'], c['z'], c['lo'], c['hi'], 1.0, 1.0)
        assert (np.diff(c['z'], axis=-1) >= 0).all() and (c['w'] >= 0).all()
        assert S < 2 or (np.diff(c['z'][R.TIED]) == 0).any()
        assert not c['w'][R.ZERO].any() and ref['opac'][R.ZERO] == -1e-10 * np.log(1e-10) and np.isfinite(ref['grad']).all()
        assert c['hi'][R.INVALID] <= c['lo'][R.INVALID] and not ref['valid'][R.INVALID] and ref['dist'][R.INVALID] == 0
        assert abs(c['w'][R.UNIT].astype(np.float64).sum() - 1.0) <= 1e-6
        off = R.ray_reg(c['w'], c['z'], c['lo'], c['hi'], 1.0, 0.0)
        assert off['touched'].tolist() == [True, True, False] and ref['touched'].all()


# ------------------------------------------------------------------------------------------------ configuration
def test_cli_flags_and_rejections():
    from outdoor_nerf_depth_amd import ddp_train_nerf as T
    a = T.config_parser().parse_args(['--expname', 'x'])
    assert a.lambda_distortion == 0.0 and a.lambda_opacity == 0.0
    T.validate_args(a)
    a = T.config_parser().parse_args(['--expname', 'x', '--lambda_distortion', '0.01', '--lambda_opacity', '0.002'])
    assert a.lambda_distortion == 0.01 and a.lambda_opacity == 0.002
    T.validate_args(a)
    for flag in ('--lambda_distortion', '--lambda_opacity'):
        for bad in ('-0.1', 'nan', 'inf'):
            with pytest.raises(SystemExit, match=flag):
                T.validate_args(T.config_parser().parse_args(['--expname', 'x', flag + '=' + bad]))


def test_trainer_rejects_fuse_loss_with_a_lambda():
    from outdoor_nerf_depth_amd.trainer import NerfppTrainer
    for kw in (dict(lambda_distortion=0.01), dict(lambda_opacity=0.01)):
        with pytest.raises(ValueError, match='fuse_loss and lambda_distortion / lambda_opacity cannot be combined'):
            NerfppTrainer('cpu', use_depth=False, fuse_loss=True, **kw)
    for kw in (dict(lambda_distortion=-1.0), dict(lambda_opacity=float('nan'))):
        with pytest.raises(ValueError, match='expected a finite value that is not negative'):
            NerfppTrainer('cpu', use_depth=False, **kw)


def test_nothing_imports_the_binding_while_both_lambdas_are_zero():
    import subprocess
    import sys
    code = ('import sys; import bench; import outdoor_nerf_depth_amd.trainer, outdoor_nerf_depth_amd.ddp_train_nerf as T; '
            "T.validate_args(T.config_parser().parse_args(['--expname', 'x'])); "
            "assert not [m for m in sys.modules if 'ray_reg' in m]; print('clean')")
    out = subprocess.run([sys.executable, '-c', code], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and 'clean' in out.stdout, out.stdout[-1000:] + out.stderr[-2000:]


def test_argument_errors_name_the_tensor():
    torch = pytest.importorskip('torch')
    from outdoor_nerf_depth_amd import ray_reg as G
    w, v = torch.zeros(8, 4), torch.zeros(8)
    with pytest.raises(G.RayRegError, match=r'weights: expected a CUDA/HIP'):
        G.ray_reg(w, w, v, v, 1.0, 1.0)
    with pytest.raises(G.RayRegError, match=r'weights: expected a float32 device tensor \[n, S\]'):
        G.ray_reg(v, w, v, v, 1.0, 1.0)
    with pytest.raises(G.RayRegError, match='weights: 0 rays'):
        G.ray_reg(torch.zeros(0, 4), w, v, v, 1.0, 1.0)
    with pytest.raises(G.RayRegError, match='weights: 1025 samples per ray'):
        G.ray_reg(torch.zeros(2, 1025), w, v, v, 1.0, 1.0)
    with pytest.raises(G.RayRegError, match='weights: 0 samples per ray'):
        G.ray_reg(torch.zeros(2, 0), w, v, v, 1.0, 1.0)


# ------------------------------------------------------------------------------------------------ header, bindings, validation
def test_header_and_bindings_agree():
    from outdoor_nerf_depth_amd import ray_reg as G
    text = open(os.path.join(ROOT, 'include', 'rayreg_hip.h')).read()
    declared = set(re.findall(r'\b(rayreg_\w+)\(', text))
    assert declared == set(G.SYMBOLS) and len(declared) == 4
    for name, value in (('ABI_VERSION', G.ABI_VERSION), ('MAX_SAMPLES', G.MAX_SAMPLES)):
        assert re.search(r'#define RAYREG_%s %d\b' % (name, value), text), name
    assert re.search(r'#define RAYREG_MAX_RAYS \(1 << 20\)', text) and G.MAX_RAYS == 1 << 20
    assert G.lib().rayreg_abi_version() == G.ABI_VERSION == 1


def test_workspace_query_answers_without_a_device():
    from outdoor_nerf_depth_amd import ray_reg as G
    assert G.workspace_bytes(1) == 256
    for n in (257, 4096, 1 << 20):
        b = G.workspace_bytes(n)
        assert b % 256 == 0 and 0 <= b - 20 * n < 256
    for n, what in ((0, 'n = 0'), (-3, 'n = -3'), ((1 << 20) + 1, 'n = 1048577')):
        with pytest.raises(G.RayRegError, match=what):
            G.workspace_bytes(n)


def test_entry_point_validates_arguments_without_a_device():
    from outdoor_nerf_depth_amd import ray_reg as G
    lib = G.lib()
    d = 1 << 20                                                # a non-null, aligned value no failing call dereferences
    names = ['stream', 'n', 'S', 'w', 'z', 'lo', 'hi', 'lambda_dist', 'lambda_opac', 'g_w', 'workspace', 'values', 'stats', 'fold_total']
    ok = [None, 4096, 64, d, 3 * d, 5 * d, 5 * d + 4096 * 4, 0.01, 0.001, 7 * d, 9 * d, 11 * d, 11 * d + 8, None]

    def call(**kw):
        a = list(ok)
        for k, v in kw.items():
            a[names.index(k)] = v
        return lib.rayreg_level(*a)
    err = lambda: lib.rayreg_last_error()
    for n in (0, -1, (1 << 20) + 1):
        assert call(n=n) == 1 and b'expected 1 .. 2^20 rays' in err(), n
    for S in (0, 1025):
        assert call(S=S) == 1 and b'S = %d, expected 1 .. 1024' % S in err(), S
    for name in ('lambda_dist', 'lambda_opac'):
        for bad in (-1.0, float('nan'), float('inf')):
            assert call(**{name: bad}) == 1 and name.encode() in err() and b'not negative' in err(), (name, bad)
    assert call(lambda_dist=0.0, lambda_opac=0.0) == 1 and b'both 0' in err()
    for ptr in ('w', 'z', 'lo', 'hi', 'workspace', 'values', 'stats'):
        assert call(**{ptr: None}) == 1 and b'non-null' in err(), ptr
    for ptr in ('w', 'z', 'lo', 'hi', 'g_w'):
        assert call(**{ptr: ok[names.index(ptr)] + 2}) == 1 and b'aligned to 4' in err(), ptr
    assert call(workspace=9 * d + 8) == 1 and b'workspace aligned to 256' in err()
    assert call(fold_total=d + 1) == 1 and b'fold_total aligned to 4' in err()
    assert call(g_w=d) == 1 and b'g_w apart from w and z' in err()
    assert call(g_w=3 * d + 64) == 1 and b'g_w apart from w and z' in err()

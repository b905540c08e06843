"""CPU (no GPU): the depth-guided fine sampling of the NeRF++ path -- the properties of the numpy reference
(tests/depth_guide_reference.py), the inverse-CDF table, the count of samples per sigma band for any uniforms, the case generator,
the configuration surface of the binding, the trainer and both CLIs, and libdepthguide_hip.so's symbols and argument checks (all
made before any device call)."""
import os
import re
import subprocess
import sys
from statistics import NormalDist

import numpy as np
import pytest

from tests import depth_guide_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(1, 1, 1), (2, 3, 2), (64, 64 + 63, 65), (64, 64 + 64, 64), (65, 128, 63), (64, 384, 128)]


def run(c, G, **kw):
    return R.depth_guide(c['zp'], c['wp'], c['zin'], c['lo'], c['hi'], G, prior=c['p'], prior_std=c['s'], v=c['v'], **kw)


# ------------------------------------------------------------------------------------------------ reference
@pytest.mark.parametrize('S_prev,S_in,G', SHAPES)
@pytest.mark.parametrize('n', [1, 3, 257])
def test_reference_properties(n, S_prev, S_in, G):
    """z_merged ascending (NaNs last), its multiset zin plus float32(g), every g inside [lo, hi] where hi > lo, the planted rays in
    the modes they were planted for"""
    calls = R.draw(7 * n + G, n, S_prev, S_in, G)
    seen = []
    for c in calls:
        ref = run(c, G)
        z = ref['z_merged']
        assert z.shape == (n, S_in + G) and z.dtype == np.float32 and ref['guide'].dtype == np.float32
        fin = np.isfinite(z)
        assert (np.diff(np.where(fin, z, np.inf), axis=-1) >= 0).all()
        both = np.concatenate([c['zin'], ref['guide']], axis=-1)
        assert (np.sort(both.view(np.uint32), axis=-1) == np.sort(z.view(np.uint32), axis=-1)).all()
        ok = c['hi'] > c['lo']
        assert (ref['guide'][ok] >= c['lo'][ok, None]).all() and (ref['guide'][ok] <= c['hi'][ok, None]).all()
        for r, kind in enumerate(c['kinds']):
            if kind:
                assert ref['mode'][r] == R.EXPECTED_MODE[kind], kind
                seen.append(kind)
            if kind in ('std_tiny', 'prior_on_sample'):
                assert (ref['guide'][r] == c['p'][r]).all()
            if kind == 'std_huge':
                assert np.isin(ref['guide'][r], (c['lo'][r], c['hi'][r])).all()
            if kind == 'one_weight':
                assert ref['sd'][r] == 0 and (ref['guide'][r] == c['zp'][r, S_prev // 2]).all()
            if kind == 'inverted':
                assert (ref['guide'][r] == c['hi'][r]).all() and c['hi'][r] <= c['lo'][r]
            if kind == 'nan_in':
                assert np.isnan(z[r, -1]) and np.isfinite(z[r, :-1]).all()
            if kind == 'unsorted_in' and S_in >= 2:
                assert (np.diff(c['zin'][r]) <= 0).all() and (np.diff(c['zin'][r]) < 0).any()
    assert seen == (list(R.KINDS) if n >= 3 else [])
    assert len(calls) == (1 if n != 3 else 4)


def test_min_std_floors_both_gaussians():
    c = R.draw(5, 257, 64, 64, 16)[0]
    ref, floor = run(c, 16), run(c, 16, min_std=0.3)
    assert (floor['sd'][floor['mode'] < 2] >= 0.3).all() and (ref['sd'][ref['mode'] < 2] < 0.3).any()
    tiny = np.array([k in ('std_zero',) for k in c['kinds']])
    assert (ref['mode'][tiny] == 1).all() and (floor['mode'][tiny] == 0).all()          # a floor makes a prior of deviation 0 usable
    nan = c['kinds'] == 'std_nan'
    assert (floor['mode'][nan] == 1).all()                                              # ... and never a NaN one


def test_lane_tree_sum_is_a_sum():
    rs = np.random.RandomState(0)
    for S in (1, 63, 64, 65, 200):
        x = rs.rand(5, S)
        assert np.abs(R.lane_tree_sum(x) - x.sum(-1)).max() <= 1e-13


# ------------------------------------------------------------------------------------------------ the table
def test_table_is_monotone_and_close_to_the_exact_inverse():
    """strictly increasing, ends exactly +-3, the binding's equal to the reference's; linear interpolation within 0.02 sigma of the
    exact truncated inverse CDF on a grid of 20 001 quantiles"""
    from outdoor_nerf_depth_amd import depth_guide as DG
    T = DG.table()
    assert T.dtype == np.float64 and T.shape == (DG.TABLE_K + 1,) == (1025,)
    assert T[0] == -3.0 and T[-1] == 3.0 and (np.diff(T) > 0).all()
    assert (T == R.table()).all() and abs(T[512]) < 1e-15
    q = np.linspace(0.0, 1.0, 20001)
    exact = R.exact_inverse(q)
    got = R.interpolate(T, np.minimum(q, np.nextafter(1.0, 0.0)))
    err = np.abs(got - exact)
    err256 = np.abs(R.interpolate(R.table(256), np.minimum(q, np.nextafter(1.0, 0.0))) - exact).max()
    print('table: worst |interpolated - exact| = %.5f sigma at q = %.5f (K = 1024); %.5f at K = 256' % (err.max(), q[err.argmax()], err256))
    assert err.max() <= 0.02


# ------------------------------------------------------------------------------------------------ the count per sigma band
@pytest.mark.parametrize('G', [1, 2, 8, 16, 63, 64, 65, 128])
def test_one_sigma_count_holds_for_any_uniforms(G):
    """A mode-0 ray with p +- 3 sd inside [lo, hi]: the number of g within one sd of p lies in [c G - 2, c G + 2],
    c = (Phi(1) - Phi(-1)) / (Phi(3) - Phi(-3)), for 2000 draws of the uniforms, the all-0 and the all-(1 - 2^-24) draws among them"""
    nd = NormalDist()
    c = (nd.cdf(1) - nd.cdf(-1)) / (nd.cdf(3) - nd.cdf(-3))
    assert abs(c - 0.68454) < 5e-6
    n = 2000
    rs = np.random.RandomState(G)
    v = (rs.randint(0, 1 << 24, (n, G)) / float(1 << 24)).astype(np.float32)
    v[0], v[1] = 0.0, 1.0 - 2.0 ** -24
    p, sd = np.float32(1.0), np.float32(0.1)
    one = np.ones(n, np.float32)
    ref = R.depth_guide(np.ones((n, 4), np.float32), np.ones((n, 4), np.float32), np.ones((n, 1), np.float32), 0.1 * one, 2.0 * one, G,
                        prior=p * one, prior_std=sd * one, v=v)
    assert (ref['mode'] == 0).all()
    count = (np.abs(ref['g'] - float(p)) <= float(sd)).sum(-1)
    worst = np.abs(count - c * G).max()
    print('G = %d: counts %d .. %d around c G = %.3f, worst deviation %.3f' % (G, count.min(), count.max(), c * G, worst))
    assert worst <= 2.0


# ------------------------------------------------------------------------------------------------ configuration
def test_binding_checks_raise_value_errors():
    from outdoor_nerf_depth_amd import depth_guide as DG
    assert DG.check_samples(0, 128) == 0 and DG.check_samples(127, 128) == 127 and DG.check_samples(0, 0) == 0
    for G, S1 in ((128, 128), (129, 128), (-1, 128), (1, 1), (1, 0), (2.5, 128)):
        with pytest.raises(ValueError, match='depth_guide_samples'):
            DG.check_samples(G, S1)
    assert DG.check_std(None, have_map=True) is None and DG.check_std(0.0, have_map=True) == 0.0 and DG.check_std(0.02, have_map=False) == 0.02
    for std in (None, 0.0, -0.1, float('nan'), float('inf')):
        with pytest.raises(ValueError, match='depth_guide_std'):
            DG.check_std(std, have_map=False)
    assert DG.check_min_std(0) == 0.0
    for bad in (-1.0, float('nan'), float('inf')):
        with pytest.raises(ValueError, match='depth_guide_min_std'):
            DG.check_min_std(bad)


def test_trainer_rejects_what_the_binding_rejects():
    from outdoor_nerf_depth_amd.trainer import NerfppTrainer
    for G in (128, 200, -1):
        with pytest.raises(ValueError, match='depth_guide_samples = %d' % G):
            NerfppTrainer('cpu', use_depth=False, cascade_samples=(64, 128), depth_guide_samples=G)
    with pytest.raises(ValueError, match='depth_guide_samples = 8'):
        NerfppTrainer('cpu', use_depth=False, cascade_samples=(64,), depth_guide_samples=8)
    for std in (0.0, -0.5, float('nan')):                       # a constant is what a prior without a map falls back to: positive
        with pytest.raises(ValueError, match='depth_guide_std'):
            NerfppTrainer('cpu', use_depth=False, depth_guide_samples=8, depth_guide_std=std)
    with pytest.raises(ValueError, match='depth_guide_min_std'):
        NerfppTrainer('cpu', use_depth=False, depth_guide_samples=8, depth_guide_min_std=-1.0)


def test_cli_flags_and_rejections():
    from outdoor_nerf_depth_amd import ddp_train_nerf as T
    a = T.config_parser().parse_args(['--expname', 'x'])
    assert a.depth_guide_samples == 0 and a.depth_guide_std == 0.0 and a.depth_guide_min_std == 0.0
    T.validate_args(a)
    a = T.config_parser().parse_args(['--expname', 'x', '--cascade_samples', '64,128', '--depth_guide_samples', '64', '--depth_guide_std', '0.05',
                                      '--depth_guide_min_std', '0.01'])
    assert (a.depth_guide_samples, a.depth_guide_std, a.depth_guide_min_std) == (64, 0.05, 0.01)
    T.validate_args(a)
    for extra in (['--depth_guide_samples', '64'], ['--depth_guide_samples=-1'], ['--cascade_samples', '64,128', '--depth_guide_samples', '128'],
                  ['--depth_guide_samples', '8', '--depth_guide_std=-1'], ['--depth_guide_samples', '8', '--depth_guide_min_std', 'nan']):
        with pytest.raises(SystemExit, match='--depth_guide_samples'):                  # (the default cascade is 64,64)
            T.validate_args(T.config_parser().parse_args(['--expname', 'x'] + extra))


def test_nothing_imports_the_binding_while_the_flag_is_absent():
    code = ('import sys; import bench; import outdoor_nerf_depth_amd.trainer as TR, outdoor_nerf_depth_amd.ddp_train_nerf as T, '
            'outdoor_nerf_depth_amd.ddp_test_nerf; '
            "T.validate_args(T.config_parser().parse_args(['--expname', 'x'])); "
            "assert not [m for m in sys.modules if 'depth_guide' in m]; "
            "T.validate_args(T.config_parser().parse_args(['--expname', 'x', '--depth_guide_samples', '8'])); "
            "assert 'outdoor_nerf_depth_amd.depth_guide' in sys.modules; print('clean')")
    out = subprocess.run([sys.executable, '-c', code], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and 'clean' in out.stdout, out.stdout[-1000:] + out.stderr[-2000:]


def test_argument_errors_name_the_tensor():
    torch = pytest.importorskip('torch')
    from outdoor_nerf_depth_amd import depth_guide as DG
    z, v = torch.zeros(8, 4), torch.zeros(8)
    with pytest.raises(DG.DepthGuideError, match=r'z_prev: expected a CUDA/HIP'):
        DG.depth_guide(z, z, z, v, v, 2)
    with pytest.raises(DG.DepthGuideError, match=r'z_prev: expected a float32 device tensor \[n, S_prev\]'):
        DG.depth_guide(v, z, z, v, v, 2)
    with pytest.raises(DG.DepthGuideError, match='z_prev: 0 rays'):
        DG.depth_guide(torch.zeros(0, 4), z, z, v, v, 2)
    with pytest.raises(DG.DepthGuideError, match='z_prev: 1025 samples per ray'):
        DG.depth_guide(torch.zeros(8, 1025), z, z, v, v, 2)
    with pytest.raises(DG.DepthGuideError, match='z_in: 4 samples per ray and 509 guided ones'):
        DG.depth_guide(z, z, z, v, v, 509)
    with pytest.raises(DG.DepthGuideError, match='z_in: 4 samples per ray and 0 guided ones'):
        DG.depth_guide(z, z, z, v, v, 0)


# ------------------------------------------------------------------------------------------------ header, bindings, validation
def test_header_and_bindings_agree():
    from outdoor_nerf_depth_amd import depth_guide as DG
    text = open(os.path.join(ROOT, 'include', 'depthguide_hip.h')).read()
    declared = set(re.findall(r'\b(depthguide_\w+)\(', text))
    assert declared == set(DG.SYMBOLS) and len(declared) == 3
    for name, value in (('ABI_VERSION', DG.ABI_VERSION), ('MAX_PREV', DG.MAX_PREV), ('MAX_MERGED', DG.MAX_MERGED), ('TABLE_K', DG.TABLE_K),
                        ('RNG_STREAM', DG.RNG_STREAM)):
        assert re.search(r'#define DEPTHGUIDE_%s %d\b' % (name, value), text), name
    assert re.search(r'#define DEPTHGUIDE_MAX_RAYS \(1 << 20\)', text) and DG.MAX_RAYS == 1 << 20
    assert DG.lib().depthguide_abi_version() == DG.ABI_VERSION == 1
    # the stream id is on record beside the generator's include and in the main library's header (nerfpp_common.h itself is keyed
    # to the committed counter profile and stays byte for byte)
    own = open(os.path.join(ROOT, 'outdoor_nerf_depth_amd', 'csrc', 'depthguide_kernels.h')).read()
    assert 'stream 5 = the stratified quantiles' in own and '#include "nerfpp_common.h"' in own
    assert '5 the depth-guided fine samples' in open(os.path.join(ROOT, 'include', 'nerfpp_hip.h')).read()


def test_entry_point_validates_arguments_without_a_device():
    from outdoor_nerf_depth_amd import depth_guide as DG
    lib = DG.lib()
    d = 1 << 20                                                # a non-null, aligned value no failing call dereferences
    names = ['stream', 'n', 'S_prev', 'S_in', 'G', 'zp', 'wp', 'zin', 'lo', 'hi', 'prior', 'prior_std', 'std_const', 'min_std', 'table', 'v',
             'use_rng', 'seed', 'step', 'z_merged', 'mode', 'guide']
    ok = [None, 1024, 64, 128, 64, d, 3 * d, 5 * d, 7 * d, 9 * d, 11 * d, 13 * d, 0.0, 0.0, 15 * d, None, 1, 777, 1, 17 * d, 19 * d, None]

    def call(**kw):
        a = list(ok)
        for k, v in kw.items():
            a[names.index(k)] = v
        return lib.depthguide_merge(*a)
    err = lambda: lib.depthguide_last_error()
    for n in (0, -1, (1 << 20) + 1):
        assert call(n=n) == 1 and b'expected 1 .. 2^20 rays' in err(), n
    for S in (0, 1025):
        assert call(S_prev=S) == 1 and b'S_prev = %d, expected 1 .. 1024' % S in err(), S
    for S_in, G in ((0, 4), (4, 0), (449, 64), (128, 385), (2 ** 31 - 1, 2 ** 31 - 1)):
        assert call(S_in=S_in, G=G) == 1 and b'S_in + G <= 512' in err(), (S_in, G)
    for bad in (-1.0, float('nan'), float('inf')):
        assert call(min_std=bad) == 1 and b'min_std' in err() and b'not negative' in err(), bad
    for ptr in ('zp', 'wp', 'zin', 'lo', 'hi', 'table', 'z_merged', 'mode'):
        assert call(**{ptr: None}) == 1 and b'non-null' in err(), ptr
    for ptr in ('zp', 'wp', 'zin', 'lo', 'hi', 'prior', 'prior_std', 'z_merged', 'mode'):
        assert call(**{ptr: ok[names.index(ptr)] + 2}) == 1 and b'aligned to 4' in err(), ptr
    assert call(table=15 * d + 4) == 1 and b'table aligned to 8' in err()
    assert call(v=21 * d) == 1 and b'either use_rng or v' in err()
    assert call(z_merged=5 * d + 64) == 1 and b'z_merged apart from zin' in err()

"""CPU (no GPU): the Gaussian negative-log-likelihood depth loss -- the numpy reference (tests/depth_gnll_reference.py)
against upstream's own function (tests/golden/depth_gnll.npz) and against central differences, the case generator, both loaders
of the prior's standard deviation with their fallback and error rules, the configuration surface of both training paths, and
libdepthgnll_hip.so's symbols, workspace query and argument checks (all made before any device call)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from tests import depth_gnll_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------------ reference
@pytest.mark.parametrize('name,n', [('n7', 7), ('n257', 257)])
def test_reference_matches_upstream(name, n):
    """value rtol 1e-12, gradients atol 1e-12 against depth_gaussian_log_likelihood and torch autograd in float64"""
    g = np.load(os.path.join(ROOT, 'tests', 'golden', 'depth_gnll.npz'))
    w, x, d, p, sigma = (g['%s_%s' % (name, k)] for k in ('w', 'x', 'd', 'p', 'sigma'))
    assert w.shape == x.shape == (n, 64) and w.dtype == np.float32
    ref = R.gnll(w, x, d, p, sigma)
    sup, gated, clamped = ref['stats']
    ungated, invalid = (ref['sup'] & ~ref['gated']).sum(), (~ref['sup']).sum()
    err_d, err_w = np.abs(ref['g_d'] - g[name + '_g_d']).max(), np.abs(ref['g_w'] - g[name + '_g_w']).max()
    print('%s: value %.17g (golden %.17g); %d supervised, %d gated, %d clamped, %d ungated, %d invalid; max |g_d - golden| %.3e of %.3e, '
          'max |g_w - golden| %.3e of %.3e' % (name, ref['value'], float(g[name + '_value']), sup, gated, clamped, ungated, invalid, err_d,
                                               np.abs(g[name + '_g_d']).max(), err_w, np.abs(g[name + '_g_w']).max()))
    assert clamped >= 2 and ungated >= 1 and invalid >= 1
    np.testing.assert_allclose(ref['value'], float(g[name + '_value']), rtol=1e-12)
    np.testing.assert_allclose(ref['g_d'], g[name + '_g_d'], rtol=0, atol=1e-12)
    np.testing.assert_allclose(ref['g_w'], g[name + '_g_w'], rtol=0, atol=1e-12)
    assert not g[name + '_g_d'][~ref['gated']].any() and not g[name + '_g_w'][~ref['gated']].any()


@pytest.mark.parametrize('edges', [False, True])
def test_reference_gradient_matches_central_differences(edges):
    """On the gated rays above the clamp (below it the gradient passes through the clamp and is not the value's derivative), with
    the gate held: n * d value / d D and n * d value / d w against central differences of the ray's own l_r in float64.  The generator
    keeps every ray 1e-4 off the gate and the clamp; the step h = 1e-8 moves V by at most h * max (x - D)^2 = 3e-7, under that margin
    of any V >= 1e-3.  Bound per entry: truncation (h max (x - D)^2 / V)^2 <= 1e-7 relative (doubled), plus the rounding of the two
    values, 8 * 2^-53 * max(|l_r|, 1) / h."""
    c = R.draw(5, 96, [24], edges=edges, with_limit=True)
    w, x, d = c['w'][0].astype(np.float64), c['x'][0].astype(np.float64), c['d'][0].astype(np.float64)
    args = (c['p'], c['sigma'], c['limit'], edges)
    ref = R.gnll(w, x, d, *args)
    n = len(d)
    rays = np.flatnonzero(ref['gated'] & ~ref['clamped'])
    assert len(rays) >= 10
    h, worst = 1e-8, 0.0
    for r in rays:
        tol = lambda g: 2e-7 * abs(n * g) + 8 * 2.0 ** -53 * max(abs(ref['loss'][r]), 1.0) / h
        e = np.zeros_like(d)
        e[r] = h
        up, dn = R.gnll(w, x, d + e, *args), R.gnll(w, x, d - e, *args)
        assert up['gated'][r] and dn['gated'][r] and not up['clamped'][r] and not dn['clamped'][r]
        fd = (up['loss'][r] - dn['loss'][r]) / (2 * h)
        worst = max(worst, abs(fd - n * ref['g_d'][r]) / tol(ref['g_d'][r]))
        for s in (0, 11, 23):
            e2 = np.zeros_like(w)
            e2[r, s] = h
            fd = (R.gnll(w + e2, x, d, *args)['loss'][r] - R.gnll(w - e2, x, d, *args)['loss'][r]) / (2 * h)
            worst = max(worst, abs(fd - n * ref['g_w'][r, s]) / tol(ref['g_w'][r, s]))
    print('edges = %s: %d rays, worst difference to central differences at %.3f of its bound' % (edges, len(rays), worst))
    assert worst <= 1.0
    assert not ref['g_d'][~ref['gated']].any() and not ref['g_w'][~ref['gated']].any()


def test_limit_and_both_position_forms():
    c = R.draw(6, 80, [16], edges=True, with_limit=True)
    ref = R.gnll(c['w'][0], c['x'][0], c['d'][0], c['p'], c['sigma'], c['limit'], True)
    mid = (np.float32(0.5) * (c['x'][0][:, :-1] + c['x'][0][:, 1:])).astype(np.float32)
    same = R.gnll(c['w'][0], mid, c['d'][0], c['p'], c['sigma'], c['limit'], False)
    assert ref['value'] == same['value'] and (ref['g_w'] == same['g_w']).all()
    free = R.gnll(c['w'][0], c['x'][0], c['d'][0], c['p'], c['sigma'], None, True)
    cut = (c['p'] > 0) & (c['sigma'] > 0) & (c['p'] >= c['limit'])
    assert cut.any() and free['stats'][0] == ref['stats'][0] + cut.sum() and not ref['sup'][cut].any()
    none = R.gnll(c['w'][0], c['x'][0], c['d'][0], np.zeros(80, np.float32), c['sigma'], None, True)
    assert none['value'] == 0 and not none['g_d'].any() and not none['stats'].any()


@pytest.mark.parametrize('n,samples,edges,with_limit', [(64, [64], False, False), (257, [64, 64, 32], True, False), (1024, [192], False, True)])
def test_generator_plants_every_class_and_clears_the_gate(n, samples, edges, with_limit):
    c = R.draw(n, n, samples, edges, with_limit)
    census = R.census(c)
    print('(%d, %s, %d): %s, %d nudges' % (n, samples, edges, census, c['nudged']))
    for k in R.CLASSES:
        assert census[k] >= 1 or (k == 'limit' and not with_limit), k
    p, s = c['p'].astype(np.float64), c['sigma'].astype(np.float64)
    for l in range(len(samples)):
        ref = R.gnll(c['w'][l], c['x'][l], c['d'][l], c['p'], c['sigma'], c['limit'], edges)
        d, on = c['d'][l].astype(np.float64), s > 0
        assert (np.abs(np.abs(d - p) - s)[on] >= R.MARGIN * s[on]).all()
        assert (np.abs(s * s - ref['V'])[on] >= R.MARGIN * ref['V'][on]).all()
        assert (np.abs(ref['V'] - R.VAR_MIN) >= R.MARGIN * R.VAR_MIN).all()


# ------------------------------------------------------------------------------------------------ the standard deviation on disk
def _write_nerfpp_scene(tmp_path, with_std):
    from PIL import Image
    root = tmp_path / 'data' / 'scene'
    rs = np.random.RandomState(0)
    K = np.eye(4, dtype=np.float32)
    K[0, 0] = K[1, 1] = 5.0
    K[0, 2], K[1, 2] = 3.0, 2.0
    subs = ('rgb', 'pose', 'intrinsics', 'depth', 'depth_mono_crop') + (('depth_mono_crop_std',) if with_std else ())
    raw = []
    for sub in subs:
        os.makedirs(root / 'train' / sub)
    for i in range(3):
        Image.fromarray(rs.randint(0, 255, (4, 6, 3), dtype=np.uint8)).save(root / 'train' / 'rgb' / ('%03d.png' % i))
        dep = rs.randint(0, 80 * 256, (4, 6)).astype(np.uint16)
        std = rs.randint(0, 3 * 256, (4, 6)).astype(np.uint16)
        std[0, i] = 0
        raw.append(std)
        for sub in ('depth', 'depth_mono_crop'):
            Image.fromarray(dep).save(root / 'train' / sub / ('%03d.png' % i))
        if with_std:
            Image.fromarray(std).save(root / 'train' / 'depth_mono_crop_std' / ('%03d.png' % i))
        np.savetxt(root / 'train' / 'pose' / ('%03d.txt' % i), np.eye(4).reshape(1, 16))
        np.savetxt(root / 'train' / 'intrinsics' / ('%03d.txt' % i), K.reshape(1, 16))
    (root / 'scale').write_text('0.005\n')
    return str(tmp_path / 'data'), raw


def test_nerfpp_loader_reads_the_std_folder(tmp_path):
    from outdoor_nerf_depth_amd import data_loader_split as DL
    base, raw = _write_nerfpp_scene(tmp_path, with_std=True)
    plain = DL.load_data_split(base, 'scene', 'train', depth_sup_type='mono_crop')
    assert all(s.depth_std is None for s in plain) and 'depth_std' not in plain[0].get_all()    # nobody asked: nothing is read
    for const in (0.0, 0.7):                                                       # the folder wins over the constant
        samplers = DL.load_data_split(base, 'scene', 'train', depth_sup_type='mono_crop', depth_std=const)
        for s, r in zip(samplers, raw):
            np.testing.assert_array_equal(s.depth_std, np.float32(0.005) * (r.astype(np.float32) / 256.0).reshape(-1))
            assert s.depth_std.dtype == np.float32 and (s.depth_std == 0).any()
    np.random.seed(0)
    b = samplers[1].random_sample(5)
    assert b['depth_std'].shape == (5,) and set(b) >= {'depth_sup', 'depth_std'}
    skipped = DL.load_data_split(base, 'scene', 'train', skip=2, depth_sup_type='mono_crop', depth_std=0.0)
    np.testing.assert_array_equal(skipped[1].depth_std, samplers[2].depth_std)


def test_nerfpp_loader_fallback_and_error(tmp_path):
    from outdoor_nerf_depth_amd import data_loader_split as DL
    base, _ = _write_nerfpp_scene(tmp_path, with_std=False)
    samplers = DL.load_data_split(base, 'scene', 'train', depth_sup_type='mono_crop', depth_std=0.5)
    for s in samplers:
        np.testing.assert_array_equal(s.depth_std, np.full(24, 0.5 * 0.005, np.float32))
    with pytest.raises(ValueError, match=r'no maps in .*train/depth_mono_crop_std and --depth_gnll_std = 0'):
        DL.load_data_split(base, 'scene', 'train', depth_sup_type='mono_crop', depth_std=0.0)
    with pytest.raises(ValueError, match=r'train/depth_std '):                    # depth_sup_type gt: depth_std/ next to depth/
        DL.load_data_split(base, 'scene', 'train', depth_sup_type='gt', depth_std=0.0)


def test_synthetic_scene_has_a_std():
    from outdoor_nerf_depth_amd import data_loader_split as DL
    for kind in ('gt', 'mono_crop'):
        s = DL.synthetic_ray_samplers('train', 1, kind, n_frames=3, H=6, W=8, depth_std=0.0)[0]
        assert s.depth_std.dtype == np.float32 and ((s.depth_std > 0) == (s.depth_sup > 0)).all() and (s.depth_sup > 0).any()
        on = s.depth_sup > 0
        assert (s.depth_std[on] <= 0.1001 * s.depth_sup[on]).all() and (s.depth_std[on] >= 0.0099 * s.depth_sup[on]).all()
    s = DL.synthetic_ray_samplers('train', 1, 'gt', n_frames=3, H=6, W=8, depth_std=2.0)[0]
    np.testing.assert_array_equal(s.depth_std, np.full(48, 2.0 * s.depth_scale, np.float32))
    assert DL.synthetic_ray_samplers('train', 1, 'gt', n_frames=3, H=6, W=8)[0].depth_std is None


def _mip360_cfg(data, extra=()):
    from outdoor_nerf_depth_amd import mip360_data as D
    return D.parse_gin(bindings=["Config.data_dir = '%s'" % data, "Config.depth_sup_type = 'mono_crop'", 'Config.sample_every = 1',
                                 "Config.depth_loss_type = 'gnll'"] + list(extra))


def test_mip360_scene_reads_the_std_folder(tmp_path):
    from PIL import Image
    from outdoor_nerf_depth_amd import mip360_data as D
    from tests.test_mip360_scene import write_scene
    data = tmp_path / 'scene'
    write_scene(str(data), n_frames=12, H=8, W=10)
    with pytest.raises(ValueError, match=r'depths_mono_crop_std does not exist and Config.depth_gnll_std = 0'):
        D.Scene(_mip360_cfg(data))
    const = D.Scene(_mip360_cfg(data, ['Config.depth_gnll_std = 0.25']))
    assert const.depths_std is None and const.depth_std_const == float(np.float32(const.scale * 0.25))
    os.makedirs(data / 'depths_mono_crop_std')
    rs, raw = np.random.RandomState(1), {}
    for name in sorted(os.listdir(data / 'depths_mono_crop')):
        raw[name] = rs.randint(0, 2 * 256, (8, 10)).astype(np.uint16)
        raw[name][0, 0] = 0
        Image.fromarray(raw[name]).save(data / 'depths_mono_crop_std' / name)
    # the crop range and the keep ratio cut the prior, not its standard deviation; the folder wins over the constant
    scene = D.Scene(_mip360_cfg(data, ['Config.depth_gnll_std = 0.25', 'Config.depth_crop_range = 6.0']))
    assert scene.depth_std_const is None and scene.depths_std.shape == scene.depths_sup.shape and scene.depths_std.dtype == np.float32
    for i, name in enumerate(scene.names):
        np.testing.assert_array_equal(scene.depths_std[i], (scene.scale * D.convert_depth(raw[name].astype(np.float32))).astype(np.float32))
    assert (scene.depths_std[:, 0, 0] < 0).all() and (scene.depths_sup < 0).sum() > (D.Scene(_mip360_cfg(data)).depths_sup < 0).sum()
    other = D.Scene(D.parse_gin(bindings=["Config.data_dir = '%s'" % data, "Config.depth_sup_type = 'mono_crop'"]))
    assert other.depths_std is None and other.depth_std_const is None                # another depth type: nothing is read


# ------------------------------------------------------------------------------------------------ configuration
def test_gin_accepts_the_type_and_the_key():
    from outdoor_nerf_depth_amd import mip360_data as D
    from outdoor_nerf_depth_amd import mip360 as M
    assert D.parse_gin(bindings=[])['depth_gnll_std'] == 0.0 == D.CONFIG_DEFAULTS['depth_gnll_std']
    cfg = D.parse_gin(bindings=["Config.depth_loss_type = 'gnll'", 'Config.depth_gnll_std = 0.5'])
    assert cfg['depth_loss_type'] == 'gnll' and cfg['depth_gnll_std'] == 0.5
    assert M.GNLL == 'gnll' and 'gnll' in M.DEPTH_LOSS_TYPES and 'gnll' not in M.DEPTH_TYPES
    assert 'nll' not in M.DEPTH_LOSS_TYPES and 'los' not in M.DEPTH_LOSS_TYPES


def test_nerfpp_cli_flags_and_rejections():
    from outdoor_nerf_depth_amd import ddp_train_nerf as T
    a = T.config_parser().parse_args(['--expname', 'x', '--use_depth', '--depth_loss_type', 'gnll', '--depth_gnll_std', '0.4'])
    assert a.depth_loss_type == 'gnll' and a.depth_gnll_std == 0.4
    T.validate_args(a)
    assert T.config_parser().parse_args(['--expname', 'x']).depth_gnll_std == 0.0
    for dead in ('nll', 'los'):                                                     # stay rejected exactly as before
        with pytest.raises(SystemExit, match='dead code in the reference'):
            T.validate_args(T.config_parser().parse_args(['--expname', 'x', '--use_depth', '--depth_loss_type', dead]))


def test_nerfpp_trainer_rejects_the_two_combinations():
    from outdoor_nerf_depth_amd.trainer import NerfppTrainer
    with pytest.raises(ValueError, match=r"'gnll' and fuse_loss"):
        NerfppTrainer('cpu', depth_loss_type='gnll', fuse_loss=True)
    with pytest.raises(ValueError, match=r"'gnll' and optim_autoexpo"):
        NerfppTrainer('cpu', depth_loss_type='gnll', optim_autoexpo=True, img_names=['a'])
    for dead in ('nll', 'los'):
        with pytest.raises(ValueError, match='dead code there'):
            NerfppTrainer('cpu', depth_loss_type=dead)


def test_argument_errors_name_the_tensor():
    torch = pytest.importorskip('torch')
    from outdoor_nerf_depth_amd import depth_gnll as G
    w, v = torch.zeros(8, 4), torch.zeros(8)
    with pytest.raises(G.DepthGnllError, match=r'weights\[0\]: expected a CUDA/HIP'):
        G.gnll_loss([w], [w], [v], v, v)
    with pytest.raises(G.DepthGnllError, match='weights: 0 levels'):
        G.gnll_loss([], [], [], v, v)
    with pytest.raises(G.DepthGnllError, match='weights: 9 levels'):
        G.gnll_loss([w] * 9, [w] * 9, [v] * 9, v, v)
    with pytest.raises(G.DepthGnllError, match='x: 2 entries for 1 levels'):
        G.gnll_loss([w], [w, w], [v], v, v)


def test_nothing_imports_the_binding_until_gnll_is_used():
    import subprocess
    import sys
    code = ('import sys; import bench; import outdoor_nerf_depth_amd.trainer, outdoor_nerf_depth_amd.mip360, '
            'outdoor_nerf_depth_amd.mip360_train, outdoor_nerf_depth_amd.ddp_train_nerf; '
            "assert 'outdoor_nerf_depth_amd.depth_gnll' not in sys.modules; print('clean')")
    out = subprocess.run([sys.executable, '-c', code], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and 'clean' in out.stdout, out.stdout[-1000:] + out.stderr[-2000:]


# ------------------------------------------------------------------------------------------------ header, bindings, validation
def test_header_and_bindings_agree():
    from outdoor_nerf_depth_amd import depth_gnll as G
    text = open(os.path.join(ROOT, 'include', 'depthgnll_hip.h')).read()
    declared = set(re.findall(r'\b(depthgnll_\w+)\(', text))
    assert declared == set(G.SYMBOLS) and len(declared) == 4
    for name, value in (('ABI_VERSION', G.ABI_VERSION), ('MAX_LEVELS', G.MAX_LEVELS), ('MAX_SAMPLES', G.MAX_SAMPLES), ('STATS_ROW', G.STATS_ROW)):
        assert re.search(r'#define DEPTHGNLL_%s %d\b' % (name, value), text), name
    assert re.search(r'#define DEPTHGNLL_MAX_RAYS \(1 << 20\)', text) and G.MAX_RAYS == 1 << 20
    assert G.lib().depthgnll_abi_version() == G.ABI_VERSION == 1


def test_workspace_query_answers_without_a_device():
    from outdoor_nerf_depth_amd import depth_gnll as G
    assert G.workspace_bytes(1, 1) == 256
    for L, n in ((3, 4096), (8, 1 << 20), (2, 257)):
        b = G.workspace_bytes(L, n)
        assert b % 256 == 0 and 0 <= b - 12 * L * n < 256
    for L, n, what in ((0, 1, 'n_levels = 0'), (9, 1, 'n_levels = 9'), (1, 0, 'n = 0'), (1, (1 << 20) + 1, 'n = 1048577')):
        with pytest.raises(G.DepthGnllError, match=what):
            G.workspace_bytes(L, n)


def test_entry_point_validates_arguments_without_a_device():
    from outdoor_nerf_depth_amd import depth_gnll as G
    lib = G.lib()
    d = 256                                                    # a non-null, aligned value no failing call dereferences
    names = ['stream', 'n', 'n_levels', 'n_samples', 'x_is_edges', 'w', 'x', 'd', 'p', 'sigma', 'limit', 'scale', 'g_w', 'g_d',
             'workspace', 'values', 'stats', 'fold_total', 'fold_last', 'fold_others', 'fold_n_sup']
    ptrs = lambda *v: (C.c_void_p * 3)(*v)
    ints = lambda *v: (C.c_int * 3)(*v)
    ok = [None, 4096, 3, ints(64, 64, 32), 1, ptrs(d, d, d), ptrs(d, d, d), ptrs(d, d, d), d, d, None, (C.c_float * 3)(1, 1, 1),
          ptrs(d, 2 * d, 3 * d), ptrs(d, 2 * d, 3 * d), d, d, d, None, None, None, None]

    def call(**kw):
        a = list(ok)
        for k, v in kw.items():
            a[names.index(k)] = v
        return lib.depthgnll_levels(*a)
    err = lambda: lib.depthgnll_last_error()
    for n in (0, -1, (1 << 20) + 1):
        assert call(n=n) == 1 and b'expected 1 .. 2^20 rays' in err(), n
    for L in (0, 9):
        assert call(n_levels=L) == 1 and b'n_levels = %d, expected 1 .. 8' % L in err(), L
    assert call(x_is_edges=2) == 1 and b'x_is_edges = 2' in err()
    for S in (0, 1025):
        assert call(n_samples=ints(64, S, 32)) == 1 and b'n_samples[1] = %d, expected 1 .. 1024' % S in err(), S
    for ptr in ('n_samples', 'w', 'x', 'd', 'p', 'sigma', 'workspace', 'values', 'stats'):
        assert call(**{ptr: None}) == 1 and b'non-null' in err(), ptr
    for arr in ('w', 'x', 'd'):
        assert call(**{arr: ptrs(d, None, d)}) == 1 and b'%s[1] is null' % arr.encode() in err(), arr
        assert call(**{arr: ptrs(d, d, d + 2)}) == 1 and b'%s[2] is null or not aligned' % arr.encode() in err(), arr
    assert call(limit=d + 2) == 1 and b'p, sigma and limit aligned to 4' in err()
    assert call(workspace=d + 8) == 1 and b'workspace aligned to 256' in err()
    assert call(scale=(C.c_float * 3)(1, float('nan'), 1)) == 1 and b'scale[1]' in err()
    assert call(g_w=ptrs(d, 2 * d, d)) == 1 and b'g_w[0] and g_w[2] are the same buffer' in err()
    assert call(g_d=ptrs(d, d, 3 * d)) == 1 and b'g_d[0] and g_d[1] are the same buffer' in err()
    assert call(g_w=ptrs(d, d + 1, None)) == 1 and b'g_w[1] is not aligned' in err()
    assert call(fold_last=d + 1) == 1 and b'the folds aligned to 4' in err()

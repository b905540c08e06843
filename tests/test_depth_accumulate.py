"""No GPU: densifying sparse depth priors from neighbouring frames -- the reference on the analytic scene of
tests/test_depth_consistency.py, the host side of outdoor_nerf_depth_amd/depth_accumulate.py (argument checks, PNG encoding, the
report), the library's argument checks and both flag surfaces.

The conditions asserted on the reference's output are conditions on the definition (it densifies, the visibility filter matters),
stated by the issue that introduced it and measured on the CPU there: coverage x 3.8 .. 4.3, AbsRel of the added pixels against
the true depth 0.003 .. 0.005 with the filter and 0.013 .. 0.030 without.
"""
import os

import numpy as np
import pytest

from outdoor_nerf_depth_amd import depth_accumulate as DA
from outdoor_nerf_depth_amd import mip360_data as D
from tests import depth_accumulate_reference as R
from tests.test_depth_consistency import SHAPES, analytic_scene, sparse, with_invalids

_refs = {}


def prior_of(kind, shape):
    """'exact': the dense box scene; 'sparse': 5 % of it; 'invalids': the sparse one with a tenth each of 0, negatives and NaN"""
    depth = analytic_scene(shape, box=True)['depth']
    return {'exact': lambda: depth, 'sparse': lambda: sparse(depth, 0.05), 'invalids': lambda: with_invalids(sparse(depth, 0.3))}[kind]()


def reference(kind, shape, **params):
    """The reference's outputs for prior_of(kind, shape), computed once and shared (read-only)"""
    key = (kind, shape, tuple(sorted(params.items())))
    if key not in _refs:
        s = analytic_scene(shape, box=True)
        _refs[key] = R.accumulate(prior_of(kind, shape), s['cams'], s['nbr'], **params)
        for a in _refs[key].values():
            a.setflags(write=False)
    return _refs[key]


def absrel(out, true, mask):
    return float(np.mean(np.abs(out[mask].astype(np.float64) - true[mask]) / true[mask]))


# -------------------------------------------------------------------------------------------- 1. the reference on the scene
def test_reference_vectorised_and_scalar_forms_agree():
    shape = SHAPES[0]
    s = analytic_scene(shape, box=True)
    for prior, params in ((prior_of('invalids', shape), {}), (prior_of('sparse', shape), dict(occl_radius=8, occl_tol=0.0)),
                          (prior_of('sparse', shape), dict(occl_radius=0))):
        a, b = R.accumulate(prior, s['cams'], s['nbr'], **params), R.accumulate_scalar(prior, s['cams'], s['nbr'], **params)
        assert a['rows'][:, 1].sum() > 0
        for k in a:
            np.testing.assert_array_equal(a[k].view(np.uint8), b[k].view(np.uint8), err_msg=k)


@pytest.mark.parametrize('shape', SHAPES)
def test_reference_densifies_and_the_visibility_filter_matters(shape):
    true = analytic_scene(shape, box=True)['depth']
    prior = prior_of('sparse', shape)
    got, bare = reference('sparse', shape), reference('sparse', shape, occl_radius=0)
    before, after = (prior > 0).mean(), (got['depth_out'] > 0).mean()
    added, added_bare = got['origin'] == 2, bare['origin'] == 2
    e, e_bare = absrel(got['depth_out'], true, added), absrel(bare['depth_out'], true, added_bare)
    print('%s: coverage %.1f %% -> %.1f %% (x %.2f), rows %s; AbsRel of the added pixels %.4f, without the filter %.4f (x %.2f)'
          % (shape, 100 * before, 100 * after, after / before, got['rows'].sum(0).tolist(), e, e_bare, e_bare / e))
    assert after >= 3 * before
    assert got['rows'][:, 3].sum() > 0
    assert e < 0.01
    assert e_bare >= 2 * e
    # the outputs hang together
    own = prior > 0
    np.testing.assert_array_equal(got['origin'] == 1, own)
    np.testing.assert_array_equal(got['depth_out'][~added].view(np.int32), prior[~added].view(np.int32))
    assert (got['depth_out'][added] > 0).all() and ((got['src'] >= 0) == (got['origin'] >= 2)).all()
    F = shape[0]
    n = lambda m: m.reshape(F, -1).sum(1)
    np.testing.assert_array_equal(got['rows'], np.stack([n(own), n(got['origin'] >= 2), n(added), n(got['origin'] == 3)], 1))
    assert bare['rows'][:, 3].sum() == 0                                       # a window of the pixel alone hides nothing
    # a source pixel's slot and index: the winning key names a valid pixel of that neighbour
    s = analytic_scene(shape, box=True)
    f, y, x = np.nonzero(added)
    slot, pix = got['src'][added] >> 28, got['src'][added] & ((1 << 28) - 1)
    assert (prior[s['nbr'][f, slot], pix // shape[2], pix % shape[2]] > 0).all()


def test_ties_go_to_the_lower_slot_then_the_lower_source_pixel():
    K = np.array([[30.0, 0, 8.0], [0, 30.0, 6.0], [0, 0, 1.0]])
    c2w = np.tile(np.eye(4)[:3], (3, 1, 1))
    c2w[1:, 0, 3] = 0.2                                                        # frames 1 and 2: one pose, one depth
    cams = DA.pack_cams(K, c2w)
    depth = np.zeros((3, 12, 16), np.float32)
    depth[1:] = 5.0
    for nbr, slot in (([[1, 2], [-1, -1], [-1, -1]], 0), ([[2, 1], [-1, -1], [-1, -1]], 0), ([[-1, 2, 1], [-1] * 3, [-1] * 3], 1)):
        got = R.accumulate(depth, cams, np.array(nbr))
        added = got['origin'][0] == 2
        assert added.sum() > 100 and (got['src'][0][added] >> 28 == slot).all() and (got['origin'][1:] == 1).all()
    # two source pixels of ONE frame that land on one target pixel with the same z: the lower pixel index wins
    K2 = K.copy()
    K2[0, 0] = K2[1, 1] = 15.0                                                 # the target sees the same points at half the focal length
    cams = np.concatenate([DA.pack_cams(K2, c2w[:1]), DA.pack_cams(K, c2w[:1])], 0)
    got = R.accumulate(depth[:2], cams, np.array([[1], [-1]]))
    added = got['origin'][0] == 2
    pix = got['src'][0][added] & ((1 << 28) - 1)
    assert added.sum() > 20 and (pix % 2 == 0).all() and ((pix // 16) % 2 == 0).all()     # of each 2 x 2 block, the top left one


def test_invalid_inputs_pass_through_bit_for_bit():
    shape = SHAPES[1]
    prior = prior_of('invalids', shape).copy()
    prior.view(np.uint32)[0, 0, :3] = (0x7FC00123, 0xFFC00001, 0x80000000)       # NaN payloads and -0
    s = analytic_scene(shape, box=True)
    got = R.accumulate(prior, s['cams'], s['nbr'])
    kept = got['origin'] != 2
    np.testing.assert_array_equal(got['depth_out'][kept].view(np.int32), prior[kept].view(np.int32))
    assert np.isnan(prior[kept]).any() and (prior[kept] < 0).any() and (got['origin'] == 3).any() and (~kept).any()
    assert (got['rows'][:, 0].sum(), got['rows'][:, 1].sum()) == ((prior > 0).sum(), (got['origin'] >= 2).sum())
    none = R.accumulate(prior, s['cams'], np.full((shape[0], 2), -1))
    np.testing.assert_array_equal(none['depth_out'].view(np.int32), prior.view(np.int32))
    assert (none['src'] == -1).all() and none['rows'][:, 1:].sum() == 0


# ------------------------------------------------------------------------------------------ 2. argument errors, no device
def test_host_checks_name_the_argument():
    s = analytic_scene(SHAPES[0])
    assert DA.check_params() == dict(R.DEFAULTS) == dict(occl_radius=2, occl_tol=0.05)
    assert DA.check_params(8, 0)['occl_radius'] == 8
    for kw, text in ((dict(occl_radius=9), 'occl_radius = 9: expected an integer 0 .. 8'), (dict(occl_radius=-1), 'occl_radius = -1'),
                     (dict(occl_radius=1.5), 'occl_radius = 1.5'), (dict(occl_tol=-0.1), 'occl_tol = -0.1'),
                     (dict(occl_tol=float('nan')), 'occl_tol = nan'), (dict(occl_tol=float('inf')), 'occl_tol = inf')):
        with pytest.raises(DA.DepthAccError, match=text):
            DA.check_params(**kw)
    K = s['K'].copy()
    K[0, 1] = 0.25
    with pytest.raises(DA.DepthConsError, match='frame 0 has skew 0.25'):
        DA.pack_cams(K, s['c2w'])
    assert DA.pack_cams is __import__('outdoor_nerf_depth_amd.depth_consistency', fromlist=['x']).pack_cams       # reused, not copied


def test_tensor_checks_name_the_tensor_before_the_device_is_asked():
    torch = pytest.importorskip('torch')
    s = analytic_scene(SHAPES[0])
    for bad in (torch.zeros(6, 24, 32), np.zeros((6, 24, 32), np.float32)):
        with pytest.raises(DA.DepthAccError, match='depth: expected a CUDA/HIP float32 tensor'):
            DA.accumulate_async(bad, s['cams'], s['nbr'])
    prior = torch.zeros(6, 24, 32)
    for bad, text in ((prior.double(), r'depth: expected torch.float32, got torch.float64'), (prior[0], r'depth: expected \[F, H, W\]'),
                      (prior[:, :, ::2], 'depth: expected a contiguous tensor')):
        with pytest.raises(DA.DepthAccError, match=text):
            DA.accumulate_async(bad, s['cams'], s['nbr'])
    for out, text in ((prior, 'depth_out overlaps depth'), (prior[1:], r'depth_out \(5, 24, 32\)'), (prior.int(), 'depth_out: expected torch.float32'),
                      (torch.zeros(6, 24, 64)[:, :, ::2], 'depth_out: expected a contiguous tensor')):
        with pytest.raises(DA.DepthAccError, match=text):
            DA.accumulate_async(prior, s['cams'], s['nbr'], depth_out=out)
    with pytest.raises(DA.DepthAccError, match=r'views = 17: expected 0 \(off\) .. 16'):
        DA.accumulate_priors(prior, s['cams'], 17)


def test_scene_with_distortion_is_refused_by_name(tmp_path):
    from tests.test_mip360_scene import write_scene
    write_scene(str(tmp_path), n_frames=10, H=8, W=10, model='SIMPLE_RADIAL')
    scene = D.Scene(D.parse_gin(bindings=["Config.data_dir = '%s'" % tmp_path, "Config.depth_sup_type = 'mono_crop'", 'Config.depth_acc_views = 2']))
    with pytest.raises(D.ConfigError, match='pinhole-only .* the scene\'s camera is SIMPLE_RADIAL'):
        DA.cams_from_scene(scene)


# --------------------------------------------------------------------------------------------------- 3. the library, no GPU
def test_workspace_bytes_limits():
    assert DA.workspace_bytes(1, 1, 1) == 512                                    # one key and one tile's partials, each rounded up to 256
    assert DA.workspace_bytes(295, 375, 1242) == (295 * 375 * 1242 * 8 + 255) // 256 * 256 + (295 * 39 * 47 * 16 + 255) // 256 * 256
    assert DA.workspace_bytes(65535, 8, 32) > 0 and DA.workspace_bytes(1, 1 << 14, 1 << 14) > 0
    for args, text in (((0, 4, 4), 'n_frames = 0, expected 1 .. 65535'), ((65536, 4, 4), 'n_frames = 65536'),
                       ((1, 0, 4), 'a frame has at least one pixel'), ((1, 4, -1), 'a frame has at least one pixel'),
                       ((1, (1 << 14) + 1, 1 << 14), 'exceeds 2\\^28 pixels per frame')):
        with pytest.raises(DA.DepthAccError, match=text):
            DA.workspace_bytes(*args)


def test_binding_declares_the_headers_symbols_and_constants():
    import re
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, 'include', 'depthacc_hip.h')).read()
    declared = set(re.findall(r'^(?:const char\*|int64_t|int) (depthacc_\w+)\(', header, re.M))
    assert declared == set(DA.SYMBOLS) and len(declared) == 4
    const = dict((k, v) for k, v in re.findall(r'#define DEPTHACC_(\w+) \(?(\d+)', header))
    assert (int(const['ABI_VERSION']), int(const['MAX_FRAMES']), int(const['MAX_VIEWS']), int(const['CAM']), int(const['ROW']),
            int(const['MAX_RADIUS'])) == (DA.ABI_VERSION, DA.MAX_FRAMES, DA.MAX_VIEWS, DA.CAM, len(DA.ROW_NAMES), DA.MAX_RADIUS)
    assert [int(const['ORIGIN_' + k]) for k in ('NONE', 'OWN', 'ADDED', 'HIDDEN')] == [DA.ORIGIN_NONE, DA.ORIGIN_OWN, DA.ORIGIN_ADDED, DA.ORIGIN_HIDDEN] \
        == [R.ORIGIN_NONE, R.ORIGIN_OWN, R.ORIGIN_ADDED, R.ORIGIN_HIDDEN]
    assert [int(const['N_' + k.upper()[2:]]) for k in DA.ROW_NAMES] == [0, 1, 2, 3]
    assert len(DA.SYMBOLS['depthacc_accumulate'][1]) == header.split('int depthacc_accumulate(')[1].split(');')[0].count(',') + 1


def test_library_argument_checks_need_no_gpu():
    import ctypes as C
    lib = DA.lib()
    assert lib.depthacc_abi_version() == DA.ABI_VERSION
    buf = (C.c_double * 4096)()                                                  # host memory: every call below fails before any launch
    base = (C.addressof(buf) + 255) // 256 * 256
    p, q, ws = C.c_void_p(base), C.c_void_p(base + 4096), C.c_void_p(base + 8192)

    def call(F=1, H=2, W=2, V=1, depth=p, cams=p, nbr=p, radius=2, tol=0.05, ws=ws, out=q, origin=None, src=None, rows=None):
        return lib.depthacc_accumulate(None, F, H, W, V, depth, cams, nbr, radius, tol, ws, out, origin, src, rows)
    for kw, text in ((dict(F=0), 'n_frames = 0'), (dict(V=17), 'n_views = 17, expected 0 .. 16'), (dict(V=-1), 'n_views = -1'),
                     (dict(radius=9), 'occl_radius = 9, expected 0 .. 8'), (dict(radius=-1), 'occl_radius = -1'),
                     (dict(tol=-1.0), 'occl_tol = -1'), (dict(tol=float('nan')), 'occl_tol = nan'), (dict(tol=float('inf')), 'occl_tol = inf'),
                     (dict(depth=None), 'non-null depth, cams, depth_out, workspace'), (dict(ws=None), 'non-null depth, cams, depth_out, workspace'),
                     (dict(nbr=None), 'non-null nbr when n_views > 0'), (dict(out=p), 'depth_out overlaps depth'),
                     (dict(origin=C.c_void_p(base + 15)), 'origin overlaps depth'), (dict(src=C.c_void_p(base + 12)), 'src overlaps depth'),
                     (dict(rows=C.c_void_p(base + 8)), 'rows overlaps depth'), (dict(ws=p), 'workspace overlaps depth'),
                     (dict(ws=C.c_void_p(base + 8192 + 8)), 'workspace aligned to 256 bytes'),
                     (dict(out=C.c_void_p(base + 4097)), 'aligned to 4 bytes')):
        assert call(**kw) == 1, kw
        assert text in DA.last_error(), (kw, DA.last_error())


# ----------------------------------------------------------------------------------------------------- 4. PNG encoding
def test_png_encoding_round_trip(tmp_path):
    from PIL import Image
    raw = np.array([[0, 1, 2, 1536], [65535, 0, 7, 0]], np.uint16)
    added = np.array([[1, 0, 0, 0], [0, 1, 1, 1]], bool)
    metres = np.array([[6.0, 9.0, 9.0, 9.0], [9.0, 0.001, 10.009765625, 300.0]])
    enc = DA.encode_prior(raw, metres, added)
    assert enc.dtype == np.uint16
    np.testing.assert_array_equal(enc, [[1536, 1, 2, 1536], [65535, 2, 2562, 65535]])            # own raw values kept; half to even; clamp
    DA._write_png16(str(tmp_path / 'p.png'), enc)
    np.testing.assert_array_equal(np.asarray(Image.open(str(tmp_path / 'p.png'))), enc)
    # what the loaders make of it: an added pixel is valid; the others are what they were
    assert ((D.convert_depth(enc) > 0) == (added | (raw >= 2))).all()
    back = D.convert_depth(enc.astype(np.float32))
    assert abs(back[0, 0] - 6.0) <= 0.5 / 256 and abs(back[1, 2] - 10.009765625) <= 0.5 / 256


def test_report_totals(tmp_path):
    rows = np.array([[2, 3, 2, 1], [1, 1, 1, 0]])
    origin = np.array([[[1, 1, 2, 2, 3, 0]], [[1, 2, 0, 0, 0, 0]]], np.uint8)
    out = np.array([[[1.0, 2.0, 2.2, 4.0, 0.0, 0.0]], [[4.0, 3.0, 0.0, 0.0, 0.0, 0.0]]], np.float32)
    every = out.copy()
    every[0, 0, 4] = 7.5
    gt = np.array([[[1.0, 2.0, 2.0, 4.0, 5.0, 1.0]], [[4.0, 2.0, 1.0, 1.0, 1.0, 0.0]]], np.float32)
    DA.write_report(str(tmp_path / 'r.txt'), ['a.png', 'b.png'], rows, origin, out, gt, every)
    lines = (tmp_path / 'r.txt').read_text().splitlines()
    assert lines[0].split() == ['#', 'frame', 'n_own', 'n_candidates', 'n_added', 'n_hidden', 'coverage_before', 'coverage_after',
                                'absrel_added', 'absrel_hidden']
    a, tot = lines[1].split(), lines[-1].split()
    assert a[:5] == ['a.png', '2', '3', '2', '1'] and tot[:5] == ['total', '3', '4', '3', '1']
    assert (float(a[5]), float(a[6])) == (round(2 / 6, 6), round(4 / 6, 6)) and (float(tot[5]), float(tot[6])) == (0.25, 0.5)
    assert abs(float(a[7]) - 0.05) < 1e-6 and abs(float(a[8]) - 0.5) < 1e-6 and abs(float(tot[7]) - 0.2) < 1e-6     # (0.1 + 0 + 0.5) / 3
    assert lines[2].split()[8] == 'nan'
    DA.write_report(str(tmp_path / 'n.txt'), ['a.png', 'b.png'], rows, origin)
    assert (tmp_path / 'n.txt').read_text().splitlines()[-1] == 'total 3 4 3 1 0.250000 0.500000'
    assert DA.totals_line(rows, 4) == ('depth accumulation (4 views): 2 frames, 3 own prior pixels, 4 reached by a neighbour, 3 added, '
                                       '1 hidden (x 2.00)')


# ------------------------------------------------------------------------------------------------- 5. both flag surfaces
def test_mip360_config_keys_parse(tmp_path):
    cfg = D.parse_gin(bindings=[])
    assert (cfg['depth_acc_views'], cfg['depth_acc_occl_radius'], cfg['depth_acc_occl_tol']) == (0, 2, 0.05)
    assert DA.scene_params(cfg) == dict(R.DEFAULTS)
    cfg = D.parse_gin(bindings=['Config.depth_acc_views = 4', 'Config.depth_acc_occl_radius = 3', 'Config.depth_acc_occl_tol = 0.1'])
    assert cfg['depth_acc_views'] == 4 and DA.scene_params(cfg) == dict(occl_radius=3, occl_tol=0.1)
    from tests.test_depth_consistency import write_colmap_scene
    write_colmap_scene(str(tmp_path), F=10, H=8, W=10)
    base = ["Config.data_dir = '%s'" % tmp_path, "Config.depth_sup_type = 'noisy'"]
    s = D.Scene(D.parse_gin(bindings=base + ['Config.depth_acc_views = 16']))
    assert s.depth_acc_views == 16 and s.depth_cons_views == 0
    assert D.Scene(D.parse_gin(bindings=base)).depth_acc_views == 0
    with pytest.raises(D.ConfigError, match=r'Config.depth_acc_views = 17: expected 0 \(off\) .. 16'):
        D.Scene(D.parse_gin(bindings=base + ['Config.depth_acc_views = 17']))


def test_nerfpp_flags_parse():
    pytest.importorskip('torch')
    from outdoor_nerf_depth_amd import ddp_train_nerf as T_
    base = ['--expname', 'x', '--synthetic']
    args = T_.config_parser().parse_args(base)
    assert args.depth_acc_views == 0 and DA.args_params(args) == dict(R.DEFAULTS)
    args = T_.config_parser().parse_args(base + ['--depth_acc_views', '4', '--depth_acc_occl_radius', '3', '--depth_acc_occl_tol', '0.1'])
    assert args.depth_acc_views == 4 and DA.args_params(args) == dict(occl_radius=3, occl_tol=0.1)
    cli = DA.make_parser().parse_args(['--data_dir', 'd', '--depth_sup_type', 'lidar', '--occl_radius', '4', '--views', '6',
                                       '--gin_bindings', 'Config.factor = 2'])
    assert cli.views == 6 and DA.args_params(cli, '') == dict(occl_radius=4, occl_tol=0.05) and cli.gin_bindings == ['Config.factor = 2']
    T_.validate_args(T_.config_parser().parse_args(base + ['--use_depth', '--depth_acc_views', '16']))
    for bad, text in ((['--use_depth', '--depth_acc_views', '17'], r'--depth_acc_views = 17: expected 0 \(off\) .. 16'),
                      (['--use_depth', '--depth_acc_views', '-1'], '--depth_acc_views = -1'), (['--depth_acc_views', '4'], 'it needs --use_depth')):
        with pytest.raises(SystemExit, match=text):
            T_.validate_args(T_.config_parser().parse_args(base + bad))

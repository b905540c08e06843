"""GPU: the chain of the depth-prior stages with every compatible stage on at once (outdoor_nerf_depth_amd/depth_prior_stages.py,
DESIGN 8.14), on both trainers' loaders, against the same stages composed by hand from their public calls in the documented order.
Two chains, each a 'gnll' run without a folder or a constant for the standard deviation:
  (a) the `noisy` prior, the reconstruction's points as the alignment's anchor, then alignment, accumulation, check, completion;
  (b) the prior computed by the plane sweep (`mvs`), then accumulation, check, completion.
Every stage is deterministic and the chain adds no arithmetic of its own, so depth_sup, depth_std and every stage's rows must be
EQUAL (torch.equal / array_equal): there is no tolerance.  The scenes are the suites' analytic scene at its smallest size, 10 frames
of 8 x 10.  The MipNeRF-360 equalities hold on the commit before the table as well: they pin what the loaders computed, not the table.
"""
import numpy as np
import pytest

torch = pytest.importorskip('torch')
pytestmark = pytest.mark.gpu

from tests.test_gpu_mip360 import dev                                                     # noqa: E402
from tests.test_depth_consistency import write_nerfpp_scene                               # noqa: E402
from tests.test_gpu_depth_points import _colmap, _gin                                     # noqa: E402

SHAPE = (10, 8, 10)
REPAIRS = ['Config.depth_acc_views = 2', 'Config.depth_cons_views = 2', 'Config.depth_cons_std_floor = 0.01', 'Config.depth_comp_iters = 2',
           'Config.depth_comp_std_floor = 0.02']
CHAIN_A = ["Config.depth_sup_type = 'noisy'", "Config.depth_points_vis = 'track'", 'Config.depth_points_min_track = 2',
           "Config.depth_align_anchor = 'points'", 'Config.depth_align_min_points = 4'] + REPAIRS
CHAIN_B = ["Config.depth_sup_type = 'mvs'", 'Config.depth_mvs_views = 2', 'Config.depth_mvs_planes = 16', 'Config.depth_mvs_near = 3.0',
           'Config.depth_mvs_far = 12.0', 'Config.depth_mvs_std_floor = 0.01'] + REPAIRS
GNLL = ["Config.depth_loss_type = 'gnll'"]


@pytest.fixture(scope='module')
def mods():
    dev()
    from outdoor_nerf_depth_amd import depth_mvs, depth_points, depth_align, depth_accumulate, depth_consistency, depth_complete
    return depth_mvs, depth_points, depth_align, depth_accumulate, depth_consistency, depth_complete


@pytest.fixture(scope='module')
def colmap_scene(tmp_path_factory):
    root = tmp_path_factory.mktemp('chain_colmap') / 'scene'
    _colmap(root, SHAPE)                                                                   # depths_noisy/ and the cloud; no depths_mvs/
    return root


def _repairs(mods, scene, idx, depth, std, rgb):
    """accumulation, check and completion by hand on (depth, std); the check's own spread is not the run's source in either chain"""
    _, _, _, DA, DC, DCP = mods
    depth, _, acc = DA.accumulate_priors(depth, DA.cams_from_scene(scene, idx), scene.depth_acc_views, **DA.scene_params(scene.depth_acc_cfg))
    depth, _, cons = DC.filter_priors(depth, DC.cams_from_scene(scene, idx), scene.depth_cons_views, **DC.scene_params(scene.depth_cons_cfg, scene.scale))
    depth, std, _, comp = DCP.complete_priors(depth, rgb, std.contiguous(), **scene.depth_comp_prm)
    return depth, std, dict(depth_acc_rows=acc, depth_cons_rows=cons, depth_comp_rows=comp)


def _assert_frames(train, depth, std, rows, tag):
    assert sorted(k for k in train if k.endswith('_rows')) == sorted(rows), (tag, sorted(train))
    for k, v in rows.items():
        print('%s %s total %s' % (tag, k, v.sum(0).tolist()))
        assert train[k].dtype == v.dtype and torch.equal(train[k], v), (tag, k)
    assert torch.equal(train['depth_sup'], depth), tag
    assert torch.equal(train['depth_std'], std), tag
    print('%s: %d of %d prior pixels, std in [%g, %g]' % (tag, int((depth > 0).sum()), depth.numel(), float(std[depth > 0].min()) if bool((depth > 0).any())
                                                         else float('nan'), float(std.max())))


def test_mip360_chain_on_a_prior_aligned_to_the_points(mods, colmap_scene):
    from outdoor_nerf_depth_amd import mip360_data as D
    _, DP, DAL, _, _, _ = mods
    raw = D.Scene(D.parse_gin(bindings=_gin(colmap_scene, "Config.depth_sup_type = 'noisy'"))).device_frames('train', dev())
    scene = D.Scene(D.parse_gin(bindings=_gin(colmap_scene, *CHAIN_A) + GNLL))
    assert scene.depth_std_source == 'alignment' and scene.depth_points_target == 'anchor' and scene.depths_anchor is None
    train = scene.device_frames('train', dev())
    anchor, _, _, points = DP.splat_scene(scene, scene.train, dev(), scene.depth_points_prm)
    depth, std, align = DAL.align_priors(raw['depth_sup'], anchor, **scene.depth_align_prm)
    depth, std, rows = _repairs(mods, scene, scene.train, depth, std, raw['rgb_u8'])
    _assert_frames(train, depth, std, dict(rows, depth_points_rows=points, depth_align_rows=align), 'mip360 (a)')
    test = scene.device_frames('test', dev())
    assert not [k for k in test if k.endswith('_rows')] and 'depth_std' not in test


def test_mip360_chain_on_a_swept_prior(mods, colmap_scene):
    from outdoor_nerf_depth_amd import mip360_data as D
    DM, _, _, _, DC, _ = mods
    scene = D.Scene(D.parse_gin(bindings=_gin(colmap_scene, *CHAIN_B) + GNLL))
    assert scene.depth_std_source == 'mvs' and not scene.depths_sup.any()
    train = scene.device_frames('train', dev())
    depth, std, _, mvs = DM.sweep_priors(train['rgb_u8'], DC.cams_from_scene(scene, scene.train), **scene.depth_mvs_prm)
    depth, std, rows = _repairs(mods, scene, scene.train, depth, std, train['rgb_u8'])
    _assert_frames(train, depth, std, dict(rows, depth_mvs_rows=mvs), 'mip360 (b)')


def test_mip360_totals_lines_come_in_the_trainers_print_order(mods, colmap_scene):
    from outdoor_nerf_depth_amd import depth_prior_stages as PS
    from outdoor_nerf_depth_amd import mip360_data as D
    DM, DP, DAL, DA, DC, DCP = mods
    H = lambda t: t.cpu().numpy()
    scene = D.Scene(D.parse_gin(bindings=_gin(colmap_scene, *CHAIN_A) + GNLL))
    train = scene.device_frames('train', dev())
    assert PS.totals_lines(scene, train) == [DP.totals_line(H(train['depth_points_rows']), 'track'), DAL.totals_line(H(train['depth_align_rows']), 'points'),
                                             DA.totals_line(H(train['depth_acc_rows']), 2), DC.totals_line(H(train['depth_cons_rows']), 2),
                                             DCP.totals_line(H(train['depth_comp_rows']), 2)]
    scene = D.Scene(D.parse_gin(bindings=_gin(colmap_scene, *CHAIN_B) + GNLL))
    train = scene.device_frames('train', dev())
    assert PS.totals_lines(scene, train) == [DA.totals_line(H(train['depth_acc_rows']), 2), DC.totals_line(H(train['depth_cons_rows']), 2),
                                             DM.totals_line(H(train['depth_mvs_rows']), 2, 16), DCP.totals_line(H(train['depth_comp_rows']), 2)]
    assert PS.totals_lines(scene, scene.device_frames('test', dev())) == []


# -------------------------------------------------------------------------------------------------------------- NeRF++
NERFPP_REPAIRS = ['--depth_acc_views', '2', '--depth_cons_views', '2', '--depth_cons_std_floor', '0.01', '--depth_comp_iters', '2',
                  '--depth_comp_std_floor', '0.02']


@pytest.fixture(scope='module')
def nerfpp_scene(tmp_path_factory):
    root = tmp_path_factory.mktemp('chain_nerfpp')
    F, H, W = SHAPE
    write_nerfpp_scene(str(root), F=F, H=H, W=W)
    _colmap(root / 'colmap', SHAPE, box=False, stems=['%06d' % i for i in range(F)])
    return root, str(root / 'colmap' / 'sparse' / '0')


def _nerfpp(root, sup_type, argv):
    from outdoor_nerf_depth_amd import ddp_train_nerf as T_
    from outdoor_nerf_depth_amd.data_loader_split import load_data_split
    args = T_.config_parser().parse_args(['--expname', 'x', '--datadir', str(root), '--scene', 'scene', '--use_depth', '--depth_loss_type', 'gnll',
                                          '--depth_sup_type', sup_type] + argv + NERFPP_REPAIRS)
    T_.validate_args(args)
    load = lambda: load_data_split(str(root), 'scene', 'train', depth_sup_type=sup_type, depth_std=0.0, depth_std_optional=True)
    return args, load(), load()


def _never(sup_type):
    raise AssertionError('no anchor is read from disk in these chains: %r' % sup_type)


def _assert_samplers(got, want, tag):
    for i, (a, b) in enumerate(zip(got, want)):
        np.testing.assert_array_equal(a.depth_sup.view(np.int32), b.depth_sup.view(np.int32), err_msg='%s depth_sup %d' % (tag, i))
        np.testing.assert_array_equal(a.depth_std.view(np.int32), b.depth_std.view(np.int32), err_msg='%s depth_std %d' % (tag, i))
    print('%s: %d prior pixels in %d frames' % (tag, sum(int((s.depth_sup > 0).sum()) for s in got), len(got)))


def _nerfpp_repairs(mods, args, samplers, scale):
    _, _, _, DA, DC, DCP = mods
    acc = DA.accumulate_samplers(samplers, dev(), 2, **DA.args_params(args))
    cons = DC.filter_samplers(samplers, dev(), 2, want_std=True, **DC.args_params(args, scale))
    comp = DCP.complete_samplers(samplers, dev(), want_std=True, **DCP.args_params(args, scale))
    return [('acc', acc, DA.totals_line(acc, 2)), ('cons', cons, DC.totals_line(cons, 2)), ('comp', comp, DCP.totals_line(comp, 2))]


def _assert_chain(done, lines, want, tag):
    assert list(done) == [name for name, _, _ in want], (tag, list(done))                  # run order
    for name, rows, _ in want:
        np.testing.assert_array_equal(done[name], rows, err_msg='%s %s' % (tag, name))
    assert lines == [line for _, _, line in want], (tag, lines)                              # each stage's line as it ends, in run order
    print('\n'.join(lines))


def test_nerfpp_chain_on_a_prior_aligned_to_the_points(mods, nerfpp_scene):
    from outdoor_nerf_depth_amd import depth_prior_stages as PS
    _, DP, DAL, _, _, _ = mods
    root, model = nerfpp_scene
    args, got, want = _nerfpp(root, 'noisy', ['--depth_points_model', model, '--depth_points_min_track', '2', '--depth_align_anchor', 'points',
                                              '--depth_align_min_points', '4'])
    scale = want[0].depth_scale
    points, depth = DP.splat_samplers(want, dev(), model, 'track', 'anchor', **DP.args_params(args, scale))
    assert all(s.depth_std is None for s in want)                                             # the points as the anchor give the prior none
    align = DAL.align_samplers(want, DP.anchors_of(want, depth), dev(), want_std=True, **DAL.args_params(args, scale))
    by_hand = [('points', points, DP.totals_line(points, 'track')), ('align', align, DAL.totals_line(align, 'points'))]
    by_hand += _nerfpp_repairs(mods, args, want, scale)
    lines = []
    done = PS.run_samplers(args, got, dev(), scale, True, _never, lines.append)
    _assert_chain(done, lines, by_hand, 'nerfpp (a)')
    _assert_samplers(got, want, 'nerfpp (a)')


def test_nerfpp_chain_on_a_swept_prior(mods, nerfpp_scene):
    from outdoor_nerf_depth_amd import depth_prior_stages as PS
    DM = mods[0]
    root, _ = nerfpp_scene
    args, got, want = _nerfpp(root, 'mvs', ['--depth_mvs_views', '2', '--depth_mvs_planes', '16', '--depth_mvs_near', '3', '--depth_mvs_far', '12',
                                            '--depth_mvs_std_floor', '0.01'])
    assert all(s.depth_sup is None for s in want)                                             # no depth_mvs/ on disk
    scale = want[0].depth_scale
    mvs = DM.sweep_samplers(want, dev(), 2, want_std=True, **DM.args_params(args, scale))
    by_hand = [('mvs', mvs, DM.totals_line(mvs, 2, 16))] + _nerfpp_repairs(mods, args, want, scale)
    lines = []
    done = PS.run_samplers(args, got, dev(), scale, True, _never, lines.append)
    _assert_chain(done, lines, by_hand, 'nerfpp (b)')
    _assert_samplers(got, want, 'nerfpp (b)')

"""GPU: the plane sweep with semi-global smoothing (depthsgm_sweep, csrc/depthsgm_kernels.hip and the slab instantiation of
csrc/depthmvs_sweep.h) against tests/depth_mvs_smooth_reference.py, through depth_mvs's calls, the CLI on both on-disk
layouts and the load-time flags of both trainers.

Gates.  Everything the smoothing adds is integer arithmetic, and the refinement is the plain sweep's float64 in the reference's order,
rounded to float32 once.  So EVERY output -- depth and std as their int32 bits, status, plane, cost, second, census and rows -- must
be EQUAL to the reference.  There is no tolerance.  The scene, the shapes and the hand-built cases are those of
tests/test_depth_mvs.py.

Measured on an MI355X (reported figures, not gates).  Every case: equal.  One call on 295 frames of 375 x 1242 with 4 views and 64
planes (tools/depth_mvs_bench.py --smooth_paths 4 8, profiles/depth_mvs_smooth_time.json), the library call between device events,
medians of 10: 239.17 ms plain, 397.78 ms with 4 paths, 479.17 ms with 8 (in a kernel trace of another run: census 3.07, the sweep
into the slab 246.6, the paths 100.0 / 181.5, select 47.6, rows 0.009); 82.4 % / 95.2 % / 95.3 % of the pixels accepted; 4.85 GB of
workspace for slabs of 24 frames.  Flags off, the `mse` step against the parent commit, medians of 3 alternating runs per side:
MipNeRF-360 7.540 against 7.537 ms (the parent's spread 0.040), NeRF++ 2.0671 against 2.0610 ms (the parent's runs 2.0607 .. 2.0712).
Training effect on the band scene as a COLMAP scene, mean |rendered - true depth| over the last 50 of 400 batches, three seeds, +-
standard error: `mse` on the `mvs` prior 0.2190 +- 0.0009, with Config.depth_mvs_smooth_paths = 8 0.2140 +- 0.0009.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

torch = pytest.importorskip('torch')
pytestmark = pytest.mark.gpu

from tests import depth_mvs_reference as R                                               # noqa: E402
from tests import depth_mvs_smooth_reference as SR                                       # noqa: E402
from tests.test_gpu_mip360 import T, N, dev                                              # noqa: E402
from tests.test_depth_consistency import analytic_cameras, analytic_depth, write_colmap_scene, write_nerfpp_scene   # noqa: E402
from tests.test_depth_mvs import SHAPES, HAND_CASES, hand_case, scene, nbr_of, textured_images                     # noqa: E402
from tests.test_depth_mvs_smooth import scene_reference, smooth_reference                                          # noqa: E402
from tests.test_gpu_depth_mvs import (NAMES, ROOT, MVS_FLAGS, assert_equal, bits, _retexture_colmap, _retexture_nerfpp,   # noqa: E402
                                      _report)


@pytest.fixture(scope='module')
def DM():
    dev()
    from outdoor_nerf_depth_amd import depth_mvs
    return depth_mvs


def run(DM, rgb, cams, nbr, table, **kw):
    """the device call on a table, every output asked for"""
    kw.setdefault('smooth_paths', 8)
    return DM.sweep_async(T(rgb), cams, nbr, inv_depth=table, census=True, **kw).get()


# ------------------------------------------------------------------------------------------------ 1. equality
@pytest.mark.parametrize('paths', (4, 8))
@pytest.mark.parametrize('shape', SHAPES)
def test_equal_to_the_reference(DM, shape, paths):
    s = scene(shape)
    rgb = T(s['rgb'])
    for views in (1, 4):
        for radius in (0, 2):
            for edge in (0, 8):
                got = DM.sweep_async(rgb, s['cams'], nbr_of(shape, views), inv_depth=s['inv_depth'], census=True, agg_radius=radius,
                                     smooth_paths=paths, smooth_edge=edge).get()
                tot = got['rows'].sum(0)
                print('%s %d paths, %d views, radius %d, edge %d: rows total %s' % (shape, paths, views, radius, edge, tot.tolist()))
                assert got['cost'].dtype == np.uint32 and got['second'].dtype == np.uint32
                assert_equal(got, scene_reference(shape, views, radius, paths, edge), '%s P %d V %d a %d e %d' % (shape, paths, views, radius, edge))
                assert tot[0] > 0 and tot[1:].sum() > 0                                        # the case has decisions to make


@pytest.mark.parametrize('planes', (4, 64, 65, 256))                                           # a full wave; the second plane of a lane; the most
def test_numbers_of_planes(DM, planes):
    shape = SHAPES[0]
    s, nbr = scene(shape), nbr_of(shape, 2)
    table = DM.planes_table(2.0, 12.0, planes)
    for paths, edge in ((8, 0), (4, 8)):
        got = run(DM, s['rgb'], s['cams'], nbr, table, smooth_paths=paths, smooth_edge=edge, smooth_p1=2, smooth_p2=7)
        ref = smooth_reference(('planes', planes, paths, edge), s['rgb'], s['cams'], nbr, table, smooth_paths=paths, smooth_edge=edge,
                               smooth_p1=2, smooth_p2=7)
        print(planes, paths, edge, got['rows'].sum(0).tolist())
        assert_equal(got, ref, '%d planes, %d paths, edge %d' % (planes, paths, edge))


def test_other_tables_and_parameters(DM):
    shape = SHAPES[1]
    s, nbr = scene(shape), nbr_of(shape, 4)
    uneven = np.concatenate([[0.0], np.sort(np.random.RandomState(3).uniform(0.05, 0.6, 20))])
    for tag, table, kw in (('a non-uniform table', uneven, {}), ('far = inf', DM.planes_table(2.0, float('inf'), 16), {}),
                           ('uniqueness 1', s['inv_depth'], dict(uniqueness=1.0)), ('std_planes 2', s['inv_depth'], dict(std_planes=2.0)),
                           ('P1 = P2', s['inv_depth'], dict(smooth_p1=4, smooth_p2=4)),
                           ('the largest P2', s['inv_depth'], dict(agg_radius=4, best_views=4, smooth_p1=100, smooth_p2=101, smooth_edge=1)),
                           ('best_views 1', s['inv_depth'], dict(best_views=1, smooth_edge=255))):
        got = run(DM, s['rgb'], s['cams'], nbr, table, **kw)
        print(tag, got['rows'].sum(0).tolist())
        assert_equal(got, SR.sweep(s['rgb'], s['cams'], nbr, table, **kw), tag)


@pytest.mark.parametrize('name', HAND_CASES)
def test_hand_built_cases_on_the_device(DM, name):
    rgb, cams, nbr, table, prm = hand_case(name)
    got = run(DM, rgb, cams, nbr, table, **prm)
    assert_equal(got, SR.sweep(rgb, cams, nbr, table, **prm), name)
    assert (got['rows'].sum(1) == got['status'][0].size).all()
    assert not got['depth'][got['status'] != R.ACCEPTED].any() and not got['std'][got['status'] != R.ACCEPTED].any()


@pytest.mark.parametrize('hw', ((1, 70), (70, 1), (17, 33)))                  # paths of length 1; diagonals entering on two borders; one past the tile
def test_frames_of_one_row_or_column(DM, hw):
    H, W = hw
    K, c2w = analytic_cameras(3, H, W)
    K[0, 0] = K[1, 1] = 30.0
    rgb = textured_images(K, c2w, analytic_depth(K, c2w, H, W, box=True))
    from outdoor_nerf_depth_amd import depth_consistency as DC
    cams, nbr, table = DC.pack_cams(K, c2w), DC.neighbours(c2w[:, :, 3], 2), DM.planes_table(2.0, 12.0, 12)
    for paths, radius, edge in ((8, 2, 0), (8, 0, 8), (4, 4, 8)):
        got = run(DM, rgb, cams, nbr, table, agg_radius=radius, smooth_paths=paths, smooth_edge=edge)
        assert_equal(got, SR.sweep(rgb, cams, nbr, table, agg_radius=radius, smooth_paths=paths, smooth_edge=edge), '%s P %d a %d' % (hw, paths, radius))
        print(hw, paths, radius, edge, got['rows'].sum(0).tolist())


# ------------------------------------------------------------------------------------------------ 2. chunks, outputs, reproducibility
def test_results_do_not_depend_on_the_slab(DM):
    shape = SHAPES[0]
    assert shape[0] == 6
    s, nbr = scene(shape), nbr_of(shape, 4)
    ref = scene_reference(shape, 4, 2, 8, 8)
    from outdoor_nerf_depth_amd import depth_mvs_smooth as MS
    for kw in (dict(slab_frames=1), dict(slab_frames=4), dict(slab_frames=6), dict(slab_frames=60), dict(slab_bytes=0),
               dict(slab_bytes=2 * MS.SLAB_ENTRY_BYTES * 16 * 24 * 32), {}):
        assert_equal(run(DM, s['rgb'], s['cams'], nbr, s['inv_depth'], smooth_edge=8, **kw), ref, 'slab %s' % kw)
    with pytest.raises(DM.DepthMvsError, match='slab_frames = 0'):
        run(DM, s['rgb'], s['cams'], nbr, s['inv_depth'], slab_frames=0)
    with pytest.raises(DM.DepthMvsError, match='slab_frames: the plain sweep keeps no slab'):
        run(DM, s['rgb'], s['cams'], nbr, s['inv_depth'], smooth_paths=0, slab_frames=2)


def test_a_frame_alone_with_its_neighbours_and_two_calls(DM):
    shape = SHAPES[2]
    s, nbr = scene(shape), nbr_of(shape, 4)
    whole = run(DM, s['rgb'], s['cams'], nbr, s['inv_depth'])
    again = run(DM, s['rgb'], s['cams'], nbr, s['inv_depth'])
    assert_equal(again, whole, 'two calls')
    assert_equal(whole, scene_reference(shape, 4, 2, 8, 0), 'the batch')
    for i in (0, 3, shape[0] - 1):
        keep = [i] + [int(j) for j in nbr[i]]                                                  # the frame and its neighbours, remapped
        sub_nbr = np.full((len(keep), 4), -1, np.int32)
        sub_nbr[0] = np.arange(1, 5)
        part = run(DM, s['rgb'][keep], s['cams'][keep], sub_nbr, s['inv_depth'], slab_frames=2)
        for name in NAMES:
            np.testing.assert_array_equal(bits(part[name][0]), bits(whole[name][i]), err_msg='frame %d alone: %s' % (i, name))
        assert (part['status'][1:] == R.UNSEEN).all()


def test_left_out_outputs_change_nothing_and_out_is_reused(DM):
    shape = SHAPES[1]
    s, nbr = scene(shape), nbr_of(shape, 4)
    rgb = T(s['rgb'])
    ref = scene_reference(shape, 4, 2, 8, 0)
    full = DM.sweep_async(rgb, s['cams'], nbr, inv_depth=s['inv_depth'], census=True, smooth_paths=8)
    assert_equal(full.get(), ref, 'every output')
    bare = DM.sweep_async(rgb, s['cams'], nbr, inv_depth=s['inv_depth'], plane=False, cost=False, second=False, census=False, rows=False,
                          smooth_paths=8)
    assert sorted(bare.tensors) == ['depth', 'status', 'std']
    assert_equal(bare.get(), ref, 'no optional output', ('depth', 'std', 'status'))
    ptrs = {k: t.data_ptr() for k, t in full.tensors.items()}
    for t in full.tensors.values():
        t.zero_()
    other = DM.sweep_async(rgb, s['cams'], nbr, inv_depth=s['inv_depth'], census=True, out=full.tensors, smooth_paths=8)
    assert {k: t.data_ptr() for k, t in other.tensors.items()} == ptrs
    assert_equal(other.get(), ref, 'out= reused')
    depth, std, status, rows = DM.sweep_priors(rgb, s['cams'], 4, planes=12, near=2.0, far=12.0, std_floor=0.3, smooth_paths=8)
    acc = ref['status'] == R.ACCEPTED
    np.testing.assert_array_equal(N(depth).view(np.int32), ref['depth'].view(np.int32))
    np.testing.assert_array_equal(N(std), np.where(acc, np.maximum(ref['std'], np.float32(0.3)), np.float32(0)))
    np.testing.assert_array_equal(rows.cpu().numpy(), ref['rows'])
    with pytest.raises(DM.DepthMvsError, match='rgb: expected a CUDA/HIP uint8 tensor'):
        DM.sweep_async(rgb.cpu(), s['cams'], nbr, smooth_paths=8)


# ------------------------------------------------------------------------------------------------ 3. the CLI on both layouts
SMOOTH_FLAGS = ['--smooth_paths', '8', '--smooth_edge', '8']
SMOOTH = dict(smooth_paths=8, smooth_edge=8)


def _scene_ref(DM, sc, idx, views, **kw):
    """the smoothed reference on frames idx of a loaded COLMAP scene, at the CLI's planes"""
    from outdoor_nerf_depth_amd import depth_consistency as DC
    cams = DC.cams_from_scene(sc, idx)
    table = DM.planes_table(2.0 * sc.scale, 12.0 * sc.scale, 12)
    return SR.sweep(sc.images[idx], cams, DC.neighbours(cams[:, [7, 11, 15]], views), table, **kw)


def test_cli_on_a_colmap_scene(DM, tmp_path):
    from outdoor_nerf_depth_amd import mip360_data as D
    names, _ = write_colmap_scene(str(tmp_path), F=12, H=32, W=40, box=True)
    _retexture_colmap(tmp_path, 12, 32, 40)
    rows = DM.main(['--data_dir', str(tmp_path), '--views', '3'] + MVS_FLAGS + SMOOTH_FLAGS)
    sc = D.Scene(D.parse_gin(bindings=["Config.data_dir = '%s'" % tmp_path, "Config.depth_sup_type = 'mvs'", 'Config.sample_every = 1',
                                       "Config.depth_loss_type = 'gnll'"]))
    ref = _scene_ref(DM, sc, np.arange(len(names)), 3, **SMOOTH)
    np.testing.assert_array_equal(rows, ref['rows'])
    acc = ref['status'] == R.ACCEPTED
    assert 0.3 < acc.mean() < 1.0
    assert sorted(d for d in os.listdir(str(tmp_path)) if d.startswith('depths_mvs')) == ['depths_mvs', 'depths_mvs_std']
    np.testing.assert_array_equal(sc.depths_sup > 0, acc)                                    # read back through the loader
    metres = np.rint(ref['depth'].astype(np.float64) / sc.scale * 256.0) / 256.0             # the device values rounded to 1 / 256 m
    np.testing.assert_allclose(sc.depths_sup[acc] / sc.scale, metres[acc], rtol=1e-6)
    assert sc.depth_std_source == 'folder' and ((sc.depths_std > 0) == acc).all()
    coverage, absrel = _report(tmp_path / 'mvs.txt', names, rows)                            # the report keeps its format
    assert abs(coverage - acc.mean()) < 1e-6 and absrel < 0.1


def test_cli_on_a_nerfpp_scene(DM, tmp_path):
    from outdoor_nerf_depth_amd import depth_consistency as DC
    from outdoor_nerf_depth_amd.data_loader_split import load_data_split
    from outdoor_nerf_depth_amd.depth_complete import guide_u8
    scale = write_nerfpp_scene(str(tmp_path), F=8)
    _retexture_nerfpp(tmp_path, 8, 24, 32)
    done = DM.main(['--datadir', str(tmp_path), '--scene', 'scene', '--views', '2'] + MVS_FLAGS + SMOOTH_FLAGS)
    assert sorted(done) == ['test', 'train']
    for split in ('train', 'test'):
        after = load_data_split(str(tmp_path), 'scene', split, depth_sup_type='mvs', depth_std=0.0)
        H, W = after[0].H, after[0].W
        cams = DC.cams_from_samplers(after)
        rgb = np.stack([guide_u8(s.img).reshape(H, W, 3) for s in after], 0)
        ref = SR.sweep(rgb, cams, DC.neighbours(cams[:, [7, 11, 15]], 2), DM.planes_table(2.0 * scale, 12.0 * scale, 12), **SMOOTH)
        np.testing.assert_array_equal(done[split], ref['rows'])
        acc = ref['status'] == R.ACCEPTED
        got = np.stack([s.depth_sup.reshape(H, W) for s in after], 0)
        np.testing.assert_array_equal(got > 0, acc)
        metres = np.rint(ref['depth'].astype(np.float64) / scale * 256.0) / 256.0
        np.testing.assert_allclose(got[acc] / scale, metres[acc], rtol=1e-6)
        std = np.stack([s.depth_std.reshape(H, W) for s in after], 0)
        assert ((std > 0) == acc).all() and 0 < acc.sum() < acc.size
        names = sorted(os.listdir(str(tmp_path / 'scene' / split / 'depth_mvs')))
        assert len(_report(tmp_path / 'scene' / split / 'mvs.txt', names, ref['rows'])) == 2


# ------------------------------------------------------------------------------------------------ 4. the load-time flags
def test_mip360_flag_gives_the_smoothed_prior(DM, tmp_path):
    from outdoor_nerf_depth_amd import depth_prior_stages as PS
    from outdoor_nerf_depth_amd import mip360_data as D
    data = tmp_path / 'scene'
    write_colmap_scene(str(data), F=12, H=32, W=40, box=True)
    _retexture_colmap(data, 12, 32, 40)
    base = ["Config.data_dir = '%s'" % data, 'Config.sample_every = 1', 'Config.batch_size = 256', "Config.depth_sup_type = 'mvs'",
            'Config.depth_mvs_views = 3', 'Config.depth_mvs_planes = 12', 'Config.depth_mvs_near = 2.0', 'Config.depth_mvs_far = 12.0']
    sc = D.Scene(D.parse_gin(bindings=base + ['Config.depth_mvs_smooth_paths = 8', 'Config.depth_mvs_smooth_edge = 8',
                                              "Config.depth_loss_type = 'gnll'", 'Config.depth_mvs_std_floor = 0.05']))
    train = sc.device_frames('train', dev())
    ref = _scene_ref(DM, sc, sc.train, 3, **SMOOTH)
    np.testing.assert_array_equal(N(train['depth_sup']).view(np.int32), ref['depth'].view(np.int32))
    np.testing.assert_array_equal(train['depth_mvs_rows'].cpu().numpy(), ref['rows'])
    acc = ref['status'] == R.ACCEPTED
    assert acc.any() and sc.depth_std_source == 'mvs'
    np.testing.assert_array_equal(N(train['depth_std']), np.where(acc, np.maximum(ref['std'], np.float32(0.05 * sc.scale)), np.float32(0)))
    assert PS.totals_lines(sc, train) == [DM.totals_line(ref['rows'], 3, 12)]                     # the totals line keeps its format
    plain = D.Scene(D.parse_gin(bindings=base)).device_frames('train', dev())
    assert not torch.equal(plain['depth_sup'], train['depth_sup'])


def test_nerfpp_flag_gives_the_smoothed_prior_in_the_samplers(DM, tmp_path):
    from outdoor_nerf_depth_amd import ddp_train_nerf as T_
    from outdoor_nerf_depth_amd import depth_consistency as DC
    from outdoor_nerf_depth_amd import depth_prior_stages as PS
    from outdoor_nerf_depth_amd.data_loader_split import load_data_split
    from outdoor_nerf_depth_amd.depth_complete import guide_u8
    scale = write_nerfpp_scene(str(tmp_path), F=8)
    _retexture_nerfpp(tmp_path, 8, 24, 32)
    samplers = load_data_split(str(tmp_path), 'scene', 'train', depth_sup_type='mvs')
    H, W = samplers[0].H, samplers[0].W
    cams = DC.cams_from_samplers(samplers)
    rgb = np.stack([guide_u8(s.img).reshape(H, W, 3) for s in samplers], 0)
    ref = SR.sweep(rgb, cams, DC.neighbours(cams[:, [7, 11, 15]], 2), DM.planes_table(2.0 * scale, 12.0 * scale, 12), **SMOOTH)
    args = T_.config_parser().parse_args(['--expname', 'x', '--datadir', str(tmp_path), '--scene', 'scene', '--use_depth', '--depth_sup_type',
                                          'mvs', '--depth_mvs_views', '2', '--depth_mvs_planes', '12', '--depth_mvs_near', '2',
                                          '--depth_mvs_far', '12', '--depth_mvs_std_floor', '0.01', '--depth_mvs_smooth_paths', '8',
                                          '--depth_mvs_smooth_edge', '8'])
    T_.validate_args(args)
    lines = []
    done = PS.run_samplers(args, samplers, dev(), scale, True, None, lines.append)
    np.testing.assert_array_equal(done['mvs'], ref['rows'])
    assert lines == [DM.totals_line(ref['rows'], 2, 12)]
    acc = ref['status'] == R.ACCEPTED
    assert acc.any()
    for i, s in enumerate(samplers):
        np.testing.assert_array_equal(s.depth_sup.view(np.int32), ref['depth'][i].reshape(-1).view(np.int32))
        np.testing.assert_array_equal(s.depth_std, np.where(acc[i], np.maximum(ref['std'][i], np.float32(0.01 * scale)), np.float32(0)).reshape(-1))


CHILD = r'''
import sys
sys.path.insert(0, %(root)r)
import numpy as np
import torch
from outdoor_nerf_depth_amd import depth_mvs as M
from outdoor_nerf_depth_amd import depth_consistency as DC
from tests.test_depth_mvs import SHAPES, scene, nbr_of
s, nbr = scene(SHAPES[0]), nbr_of(SHAPES[0], 4)
rgb = torch.from_numpy(s['rgb']).to('cuda:0')
a = M.sweep_async(rgb, s['cams'], nbr, inv_depth=s['inv_depth'], census=True).get()
b = M.sweep_async(rgb, s['cams'], nbr, inv_depth=s['inv_depth'], census=True, smooth_paths=0, smooth_p1=3, smooth_edge=9).get()
d, sd, st, rows = M.sweep_priors(rgb, s['cams'], 4, planes=12, near=2.0, far=12.0, smooth_paths=0)
torch.cuda.synchronize()
for k in a:
    assert a[k].dtype == b[k].dtype and np.array_equal(a[k], b[k]), k
assert a['cost'].dtype == np.uint16 and np.array_equal(d.cpu().numpy().view(np.int32), a['depth'].view(np.int32))
loaded = [m for m in sys.modules if m.endswith('depth_mvs_smooth')]
mapped = [l for l in open('/proc/self/maps') if 'libdepthsgm' in l]
assert not loaded and not mapped, (loaded, mapped)
assert [l for l in open('/proc/self/maps') if 'libdepthmvs' in l]
M.sweep_async(rgb, s['cams'], nbr, inv_depth=s['inv_depth'], smooth_paths=4).get()
assert [m for m in sys.modules if m.endswith('depth_mvs_smooth')] and [l for l in open('/proc/self/maps') if 'libdepthsgm' in l]
print('smooth_paths 0: nothing of the smoothing is loaded')
'''


def test_with_smooth_paths_0_nothing_of_the_smoothing_is_loaded(DM):
    p = subprocess.run([sys.executable, '-c', CHILD % dict(root=ROOT)], cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0 and 'smooth_paths 0: nothing of the smoothing is loaded' in p.stdout, p.stdout[-2000:] + p.stderr[-3000:]

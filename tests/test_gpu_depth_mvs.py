"""GPU: the plane-sweep multi-view stereo depth prior (depthmvs_sweep, csrc/depthmvs_kernels.hip) against
tests/depth_mvs_reference.py, through the CLI on both on-disk layouts and through the load-time flags of both trainers.

Gates.  Everything discrete is integer arithmetic; the kernel does the reference's float64 geometry and refinement in the reference's
order without contraction and rounds depth and std to float32 once each, as the reference does.  Nothing is rounded differently, so
EVERY output -- depth and std as their int32 bits, status, plane, cost, second, census and rows -- must be EQUAL to the reference.
There is no tolerance.  The scene, the shapes and the hand-built cases are those of tests/test_depth_mvs.py.

Measured on an MI355X (reported figures, not gates).  Every case: equal.  One call on 295 frames of 375 x 1242 with 4 views and 64
planes (tools/depth_mvs_bench.py, profiles/depth_mvs_time.json), against device events around the call: 237.08 ms in its launches
(census 3.08, sweep 235.99, rows 0.009 in a kernel trace of another run) and 238.50 ms through the binding, 428 times its compulsory
3.43 GB at 6.2 TB/s, 50.9 G steps (cell, view, plane), 713 G written float64 operations; bound by VALU issue (about 171 instructions
per step, from the assembly).  Flag off, the `mse` step against the parent commit, medians of 3 alternating runs per side:
MipNeRF-360 7.663 against 7.656 ms (the parent's spread 0.055), NeRF++ 2.1131 against 2.1161 ms (spread 0.012).  Training effect on
the textured box scene as a COLMAP scene, mean |rendered - true depth| over the last 50 of 400 batches, three seeds, +- standard
error: `mse` on the `mvs` prior 0.1678 +- 0.0007, with Config.depth_cons_views = 4 0.2070 +- 0.0008, with Config.depth_comp_iters = 3
0.1612 +- 0.0007, `gnll` with the sweep's standard deviation 0.1560 +- 0.0007, rgb-only 0.2996 +- 0.0026.
"""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

torch = pytest.importorskip('torch')
pytestmark = pytest.mark.gpu

from tests import depth_mvs_reference as R                                               # noqa: E402
from tests.test_gpu_mip360 import T, N, dev                                              # noqa: E402
from tests.test_depth_consistency import analytic_cameras, analytic_depth, write_colmap_scene, write_nerfpp_scene   # noqa: E402
from tests.test_depth_mvs import (SHAPES, HAND_CASES, hand_case, check_hand_case, scene, nbr_of, reference,        # noqa: E402
                                  textured_images)

NAMES = ('depth', 'std', 'status', 'plane', 'cost', 'second', 'census', 'rows')
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope='module')
def DM():
    dev()
    from outdoor_nerf_depth_amd import depth_mvs
    return depth_mvs


def bits(a):
    return a.view(np.int32) if a.dtype == np.float32 else a


def assert_equal(got, ref, tag='', names=NAMES):
    """the call's host outputs against the reference's: equal, the float32 planes as bits"""
    for name in names:
        a, b = got[name], ref[name]
        assert a.dtype == b.dtype and a.shape == b.shape, (tag, name, a.dtype, b.dtype, a.shape, b.shape)
        np.testing.assert_array_equal(bits(a), bits(b), err_msg='%s: %s' % (tag, name))


def run(DM, rgb, cams, nbr, table, **kw):
    """the device call on a table, every output asked for"""
    return DM.sweep_async(T(rgb), cams, nbr, inv_depth=table, census=True, **kw).get()


# ------------------------------------------------------------------------------------------------ 1. equality
@pytest.mark.parametrize('views', (1, 2, 4))
@pytest.mark.parametrize('shape', SHAPES)
def test_equal_to_the_reference(DM, shape, views):
    s = scene(shape)
    rgb = T(s['rgb'])
    for best in sorted(set((1, (views + 1) // 2, views))):
        for radius in (0, 1, 4):
            got = DM.sweep_async(rgb, s['cams'], nbr_of(shape, views), inv_depth=s['inv_depth'], census=True, best_views=best,
                                 agg_radius=radius).get()
            tot = got['rows'].sum(0)
            print('%s %d views, best %d, radius %d: rows total %s' % (shape, views, best, radius, tot.tolist()))
            assert_equal(got, reference(shape, views, best, radius), '%s V %d m %d a %d' % (shape, views, best, radius))
            assert tot[0] > 0 and tot[1:].sum() > 0                                            # the case has decisions to make


def test_other_tables_and_parameters(DM):
    shape = SHAPES[1]
    s, nbr = scene(shape), nbr_of(shape, 4)
    uneven = np.concatenate([[0.0], np.sort(np.random.RandomState(3).uniform(0.05, 0.6, 20))])
    for tag, table, kw in (('4 planes', DM.planes_table(2.0, 12.0, 4), {}), ('256 planes', DM.planes_table(2.0, 12.0, 256), {}),
                           ('a non-uniform table', uneven, {}), ('far = inf', DM.planes_table(2.0, float('inf'), 16), {}),
                           ('uniqueness 1', s['inv_depth'], dict(uniqueness=1.0)), ('std_planes 2', s['inv_depth'], dict(std_planes=2.0))):
        got = run(DM, s['rgb'], s['cams'], nbr, table, **kw)
        print(tag, got['rows'].sum(0).tolist())
        assert_equal(got, R.sweep(s['rgb'], s['cams'], nbr, table, **kw), tag)
    got = DM.sweep_async(T(s['rgb']), s['cams'], nbr, near=2.0, far=float('inf'), planes=16, census=True).get()     # the binding's own table
    assert_equal(got, R.sweep(s['rgb'], s['cams'], nbr, DM.planes_table(2.0, float('inf'), 16)), 'near / far / planes')


@pytest.mark.parametrize('name', HAND_CASES)
def test_hand_built_cases_on_the_device(DM, name):
    rgb, cams, nbr, table, prm = hand_case(name)
    got = run(DM, rgb, cams, nbr, table, **prm)
    assert_equal(got, R.sweep(rgb, cams, nbr, table, **prm), name)
    check_hand_case(name, got)


@pytest.mark.parametrize('hw', ((1, 70), (70, 1), (17, 33)))                                   # a row, a column, one past the tile both ways
def test_frames_of_one_row_or_column(DM, hw):
    H, W = hw
    K, c2w = analytic_cameras(3, H, W)
    K[0, 0] = K[1, 1] = 30.0
    rgb = textured_images(K, c2w, analytic_depth(K, c2w, H, W, box=True))
    from outdoor_nerf_depth_amd import depth_consistency as DC
    cams, nbr, table = DC.pack_cams(K, c2w), DC.neighbours(c2w[:, :, 3], 2), DM.planes_table(2.0, 12.0, 12)
    for radius in (0, 2, 4):
        got = run(DM, rgb, cams, nbr, table, agg_radius=radius)
        assert_equal(got, R.sweep(rgb, cams, nbr, table, agg_radius=radius), '%s a %d' % (hw, radius))
        print(hw, radius, got['rows'].sum(0).tolist())


# ------------------------------------------------------------------------------------------------ 2. outputs and reproducibility
def test_a_frame_alone_with_its_neighbours_and_two_calls(DM):
    shape = SHAPES[2]
    s, nbr = scene(shape), nbr_of(shape, 4)
    whole = run(DM, s['rgb'], s['cams'], nbr, s['inv_depth'])
    again = run(DM, s['rgb'], s['cams'], nbr, s['inv_depth'])
    assert_equal(again, whole, 'two calls')
    for i in (0, 3, shape[0] - 1):
        keep = [i] + [int(j) for j in nbr[i]]                                                  # the frame and its neighbours, remapped
        sub_nbr = np.full((len(keep), 4), -1, np.int32)
        sub_nbr[0] = np.arange(1, 5)
        part = run(DM, s['rgb'][keep], s['cams'][keep], sub_nbr, s['inv_depth'])
        for name in NAMES:
            np.testing.assert_array_equal(bits(part[name][0]), bits(whole[name][i]), err_msg='frame %d alone: %s' % (i, name))
        assert (part['status'][1:] == R.UNSEEN).all()


def test_left_out_outputs_change_nothing_and_out_is_reused(DM):
    shape = SHAPES[1]
    s, nbr = scene(shape), nbr_of(shape, 2)
    rgb = T(s['rgb'])
    ref = reference(shape, 2, None, 2)
    full = DM.sweep_async(rgb, s['cams'], nbr, inv_depth=s['inv_depth'], census=True)
    assert_equal(full.get(), ref, 'every output')
    bare = DM.sweep_async(rgb, s['cams'], nbr, inv_depth=s['inv_depth'], plane=False, cost=False, second=False, census=False, rows=False)
    assert sorted(bare.tensors) == ['depth', 'status', 'std']
    assert_equal(bare.get(), ref, 'no optional output', ('depth', 'std', 'status'))
    ptrs = {k: t.data_ptr() for k, t in full.tensors.items()}
    for t in full.tensors.values():
        t.zero_()
    other = DM.sweep_async(rgb, s['cams'], nbr, inv_depth=s['inv_depth'], census=True, out=full.tensors)
    assert {k: t.data_ptr() for k, t in other.tensors.items()} == ptrs
    assert_equal(other.get(), ref, 'out= reused')
    depth, std, status, rows = DM.sweep_priors(rgb, s['cams'], 2, planes=12, near=2.0, far=12.0, std_floor=0.3)
    acc = ref['status'] == R.ACCEPTED
    np.testing.assert_array_equal(N(depth).view(np.int32), ref['depth'].view(np.int32))
    np.testing.assert_array_equal(N(std), np.where(acc, np.maximum(ref['std'], np.float32(0.3)), np.float32(0)))
    np.testing.assert_array_equal(rows.cpu().numpy(), ref['rows'])
    with pytest.raises(DM.DepthMvsError, match='rgb: expected a CUDA/HIP uint8 tensor'):
        DM.sweep_async(rgb.cpu(), s['cams'], nbr)


# ------------------------------------------------------------------------------------------------ 3. the CLI on both layouts
def _retexture_colmap(root, F, H, W):
    from PIL import Image
    K, c2w = analytic_cameras(F, H, W)
    rgb = textured_images(K, c2w, analytic_depth(K, c2w, H, W, box=True))
    for i in range(F):
        Image.fromarray(rgb[i]).save(os.path.join(str(root), 'images', 'frame_%03d.png' % i))


def _retexture_nerfpp(root, F, H, W):
    from PIL import Image
    K, c2w = analytic_cameras(F, H, W)
    rgb = textured_images(K, c2w, analytic_depth(K, c2w, H, W))
    for i in range(F):
        Image.fromarray(rgb[i]).save(os.path.join(str(root), 'scene', 'train' if i % 2 == 0 else 'test', 'rgb', '%06d.png' % i))


MVS_FLAGS = ['--planes', '12', '--near', '2', '--far', '12']


def _scene_ref(DM, sc, idx, views, **kw):
    """the reference on frames idx of a loaded COLMAP scene, at the CLI's planes"""
    from outdoor_nerf_depth_amd import depth_consistency as DC
    cams = DC.cams_from_scene(sc, idx)
    table = DM.planes_table(2.0 * sc.scale, 12.0 * sc.scale, 12)
    return R.sweep(sc.images[idx], cams, DC.neighbours(cams[:, [7, 11, 15]], views), table, **kw)


def _report(path, names, rows):
    lines = open(str(path)).read().splitlines()
    assert len(lines) == 2 + len(names) and lines[-1].split()[:5] == ['total'] + [str(v) for v in rows.sum(0)]
    return [float(v) for v in lines[-1].split()[5:]]


@pytest.fixture(scope='module')
def colmap_scene(tmp_path_factory):
    root = tmp_path_factory.mktemp('mvs_colmap')
    names, _ = write_colmap_scene(str(root), F=12, H=32, W=40, box=True)
    _retexture_colmap(root, 12, 32, 40)
    return root, names


def test_cli_on_a_colmap_scene(DM, colmap_scene):
    from outdoor_nerf_depth_amd import mip360_data as D
    data, names = colmap_scene
    rows = DM.main(['--data_dir', str(data), '--views', '3'] + MVS_FLAGS)
    sc = D.Scene(D.parse_gin(bindings=["Config.data_dir = '%s'" % data, "Config.depth_sup_type = 'mvs'", 'Config.sample_every = 1',
                                       "Config.depth_loss_type = 'gnll'"]))
    ref = _scene_ref(DM, sc, np.arange(len(names)), 3)
    np.testing.assert_array_equal(rows, ref['rows'])
    acc = ref['status'] == R.ACCEPTED
    assert 0.3 < acc.mean() < 1.0
    assert sorted(d for d in os.listdir(str(data)) if d.startswith('depths_mvs')) == ['depths_mvs', 'depths_mvs_std']
    np.testing.assert_array_equal(sc.depths_sup > 0, acc)                                    # read back through the loader
    metres = np.rint(ref['depth'].astype(np.float64) / sc.scale * 256.0) / 256.0             # the device values rounded to 1 / 256 m
    np.testing.assert_allclose(sc.depths_sup[acc] / sc.scale, metres[acc], rtol=1e-6)
    assert sc.depth_std_source == 'folder' and ((sc.depths_std > 0) == acc).all()
    coverage, absrel = _report(data / 'mvs.txt', names, rows)
    print('colmap CLI: totals %s, coverage %.3f, AbsRel of the accepted %.4f' % (rows.sum(0).tolist(), coverage, absrel))
    assert abs(coverage - acc.mean()) < 1e-6 and absrel < 0.1


def test_cli_on_a_nerfpp_scene(DM, tmp_path):
    from outdoor_nerf_depth_amd import depth_consistency as DC
    from outdoor_nerf_depth_amd.data_loader_split import load_data_split
    from outdoor_nerf_depth_amd.depth_complete import guide_u8
    scale = write_nerfpp_scene(str(tmp_path), F=8)
    _retexture_nerfpp(tmp_path, 8, 24, 32)
    done = DM.main(['--datadir', str(tmp_path), '--scene', 'scene', '--views', '2'] + MVS_FLAGS)
    assert sorted(done) == ['test', 'train']
    for split in ('train', 'test'):
        after = load_data_split(str(tmp_path), 'scene', split, depth_sup_type='mvs', depth_std=0.0)
        H, W = after[0].H, after[0].W
        cams = DC.cams_from_samplers(after)
        rgb = np.stack([guide_u8(s.img).reshape(H, W, 3) for s in after], 0)
        ref = R.sweep(rgb, cams, DC.neighbours(cams[:, [7, 11, 15]], 2), DM.planes_table(2.0 * scale, 12.0 * scale, 12))
        np.testing.assert_array_equal(done[split], ref['rows'])
        acc = ref['status'] == R.ACCEPTED
        got = np.stack([s.depth_sup.reshape(H, W) for s in after], 0)
        np.testing.assert_array_equal(got > 0, acc)
        metres = np.rint(ref['depth'].astype(np.float64) / scale * 256.0) / 256.0
        np.testing.assert_allclose(got[acc] / scale, metres[acc], rtol=1e-6)
        std = np.stack([s.depth_std.reshape(H, W) for s in after], 0)                          # the _std twin, found by the loader
        assert ((std > 0) == acc).all() and 0 < acc.sum() < acc.size
        names = sorted(os.listdir(str(tmp_path / 'scene' / split / 'depth_mvs')))
        assert len(_report(tmp_path / 'scene' / split / 'mvs.txt', names, ref['rows'])) == 2
        print('nerfpp CLI %s: totals %s' % (split, ref['rows'].sum(0).tolist()))


# ------------------------------------------------------------------------------------------------ 4. the load-time flags
MVS = ["Config.depth_sup_type = 'mvs'", 'Config.depth_mvs_views = 3', 'Config.depth_mvs_planes = 12', 'Config.depth_mvs_near = 2.0',
       'Config.depth_mvs_far = 12.0']


def test_mip360_flag_computes_the_training_split_only_and_first(DM, tmp_path):
    from outdoor_nerf_depth_amd import mip360_data as D
    from tests.test_gpu_depth_consistency import _one_mip360_step
    from tests.test_gpu_mip360_app import _run
    data = tmp_path / 'scene'
    write_colmap_scene(str(data), F=12, H=32, W=40, box=True)
    _retexture_colmap(data, 12, 32, 40)
    assert not os.path.isdir(str(data / 'depths_mvs'))                                         # the folder is not read and need not exist
    base = ["Config.data_dir = '%s'" % data, 'Config.sample_every = 1', 'Config.batch_size = 256']
    cfg = D.parse_gin(bindings=base + MVS)
    sc = D.Scene(cfg)
    train = sc.device_frames('train', dev())
    ref = _scene_ref(DM, sc, sc.train, 3)
    np.testing.assert_array_equal(N(train['depth_sup']).view(np.int32), ref['depth'].view(np.int32))       # the float32 value, unquantised
    np.testing.assert_array_equal(train['depth_mvs_rows'].cpu().numpy(), ref['rows'])
    assert ref['rows'][:, 0].sum() > 0 and 'depth_std' not in train
    test = sc.device_frames('test', dev())
    assert not test['depth_sup'].any() and 'depth_mvs_rows' not in test
    b, scalars = _one_mip360_step(sc, train, cfg)
    f, x, y = b['pix'].long().unbind(1)
    assert torch.equal(b['depth_sup'].reshape(-1), train['depth_sup'][f, y, x]) and np.isfinite(scalars).all()
    # before the consistency check: it filters the sweep's prior
    cons = D.Scene(D.parse_gin(bindings=base + MVS + ['Config.depth_cons_views = 3'])).device_frames('train', dev())
    kept = N(cons['depth_sup']) > 0
    assert (kept <= (ref['depth'] > 0)).all() and kept.any() and np.array_equal(N(cons['depth_sup'])[kept], ref['depth'][kept])
    assert torch.equal(cons['depth_mvs_rows'], train['depth_mvs_rows'])
    # a gnll run without another source: the sweep's standard deviation, floored
    gn = D.Scene(D.parse_gin(bindings=base + MVS + ["Config.depth_loss_type = 'gnll'", 'Config.depth_mvs_std_floor = 0.05']))
    assert gn.depth_std_source == 'mvs'
    g = gn.device_frames('train', dev())
    acc = ref['status'] == R.ACCEPTED
    np.testing.assert_array_equal(N(g['depth_std']), np.where(acc, np.maximum(ref['std'], np.float32(0.05 * gn.scale)), np.float32(0)))
    # the trainer: a few steps, one log line with the totals
    bind = base + MVS + ["Config.checkpoint_dir = '%s'" % (tmp_path / 'run'), 'Config.max_steps = 3', 'Config.checkpoint_every = 100',
                         'Config.print_every = 1', 'Config.lr_delay_steps = 0', 'Config.render_chunk_size = 1024']
    out = _run('mip360_train', sum([['--gin_bindings', x] for x in bind], []))
    lines = [l for l in out.splitlines() if l.startswith('depth ')]
    print(lines)
    assert lines == [DM.totals_line(ref['rows'], 3, 12)], out[-2000:]
    assert 'step 3/3' in out


def test_nerfpp_flag_computes_the_samplers_prior(DM, tmp_path):
    from outdoor_nerf_depth_amd import depth_consistency as DC
    from outdoor_nerf_depth_amd.data_loader_split import load_data_split
    from outdoor_nerf_depth_amd.depth_complete import guide_u8
    from tests.test_gpu_depth_consistency import _run_nerfpp
    scale = write_nerfpp_scene(str(tmp_path), F=8)
    _retexture_nerfpp(tmp_path, 8, 24, 32)
    assert not os.path.isdir(str(tmp_path / 'scene' / 'train' / 'depth_mvs'))
    samplers = load_data_split(str(tmp_path), 'scene', 'train', depth_sup_type='mvs')
    assert all(s.depth_sup is None for s in samplers)
    H, W = samplers[0].H, samplers[0].W
    cams = DC.cams_from_samplers(samplers)
    rgb = np.stack([guide_u8(s.img).reshape(H, W, 3) for s in samplers], 0)
    ref = R.sweep(rgb, cams, DC.neighbours(cams[:, [7, 11, 15]], 2), DM.planes_table(2.0 * scale, 12.0 * scale, 12))
    prm = dict(planes=12, near=2.0 * scale, far=12.0 * scale)
    rows = DM.sweep_samplers(samplers, dev(), 2, want_std=True, std_floor=0.01 * scale, **prm)
    np.testing.assert_array_equal(rows, ref['rows'])
    acc = ref['status'] == R.ACCEPTED
    for i, s in enumerate(samplers):                                                           # host sampling reads these
        np.testing.assert_array_equal(s.depth_sup.view(np.int32), ref['depth'][i].reshape(-1).view(np.int32))
        np.testing.assert_array_equal(s.depth_std, np.where(acc[i], np.maximum(ref['std'][i], np.float32(0.01 * scale)), np.float32(0)).reshape(-1))
    argv = ['--expname', 'mvs', '--basedir', str(tmp_path), '--datadir', str(tmp_path), '--scene', 'scene', '--cascade_samples', '16,16',
            '--use_depth', '--depth_sup_type', 'mvs', '--lambda_depth', '0.1', '--world_size', '1', '--N_rand_override', '128', '--i_weights',
            '100', '--i_test', '100', '--i_print', '1', '--N_iters', '3', '--testskip', '1', '--depth_mvs_views', '2', '--depth_mvs_planes', '12',
            '--depth_mvs_near', '2', '--depth_mvs_far', '12']
    text = _run_nerfpp(argv)
    found = [l for l in text.splitlines() if l.startswith('depth ')]
    print(found)
    assert found == [DM.totals_line(ref['rows'], 2, 12)], text[-2000:]
    assert len(re.findall(r'step: \d+ .*level_1/loss_depth: [-\d.e+]+ ', text)) == 3, text[-2000:]


CHILD = r'''
import sys
sys.path.insert(0, %(root)r)
import torch
from outdoor_nerf_depth_amd import mip360_data as D
from outdoor_nerf_depth_amd import ddp_train_nerf as T_
cfg = D.parse_gin(bindings=["Config.data_dir = %(data)r", "Config.depth_sup_type = 'noisy'", 'Config.sample_every = 1'])
train = D.Scene(cfg).device_frames('train', torch.device('cuda:0'))
assert 'depth_mvs_rows' not in train
args = T_.config_parser().parse_args(%(argv)r)
T_.validate_args(args)
args.world_size = 1
T_.ddp_train_nerf(0, args)
torch.cuda.synchronize()
loaded = [m for m in sys.modules if m.endswith('depth_mvs')]
mapped = [l for l in open('/proc/self/maps') if 'libdepthmvs' in l]
assert not loaded and not mapped, (loaded, mapped)
assert 'outdoor_nerf_depth_amd.depth_mvs_flags' in sys.modules
print('flag off: nothing of the sweep is loaded')
'''


def test_without_the_flag_nothing_of_the_sweep_is_loaded(DM, tmp_path):
    from tests.test_gpu_depth_consistency import _nerfpp_argv
    write_colmap_scene(str(tmp_path / 'scene'), F=10, H=16, W=20)
    code = CHILD % dict(root=ROOT, data=str(tmp_path / 'scene'), argv=_nerfpp_argv(tmp_path))
    p = subprocess.run([sys.executable, '-c', code], cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0 and 'flag off: nothing of the sweep is loaded' in p.stdout, p.stdout[-2000:] + p.stderr[-3000:]

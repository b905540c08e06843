"""GPU: completing sparse depth priors by image-guided filtering (depthcomp_complete, csrc/depthcomp_kernels.hip)
against tests/depth_complete_reference.py, through the CLI on both on-disk layouts and through the load-time flags of both trainers.

Gates.  The kernel does the reference's float64 arithmetic in the reference's order without contraction and rounds z, c, v and
std_out to float32 once each, as the reference does; the weight tables are the caller's, so no exp is evaluated on the device.
Nothing is rounded differently, so EVERY output -- depth and std as their int32 bits (NaN payloads included), conf, origin, pass
and rows -- must be EQUAL to the reference.  There is no tolerance.  The scene, the shapes and the priors are those of
tests/test_depth_accumulate.py; the guide image follows the scene's surfaces (tests/test_depth_complete.py).

Measured on an MI355X (reported figures, not gates).  Every case: equal.  One call on 295 frames of 375 x 1242
(tools/depth_complete_bench.py, profiles/depth_complete_time.json): a 5 % prior at the defaults (radius 4, 3 passes) 17.52 ms in its
launches (pass 1 9.22, pass 2 4.15, pass 3 4.09, rows 0.009) and 17.59 ms through the binding, 10.9 times its compulsory 10.0 GB at
6.2 TB/s, 55.9 G written float64 operations and 367 GB of LDS reads; at radius 8 57.01 ms (30.67, 13.45, 12.71) and 57.18 ms; a
dense prior 3.46 ms (0.74, 1.13, 1.12 in another run) and 3.57 ms, 2.2 times.  The first pass is bound by VALU issue (about 30 instructions per tap),
the later ones by latency.  Flag off, the `mse` step against the parent commit, medians of 6 alternating runs: MipNeRF-360 7.484
against 7.503 ms (the parent's spread 0.084), NeRF++ 2.0502 against 2.0534 ms (spread 0.013).  Training effect on the analytic box
scene as a COLMAP scene with a 5 % prior, mean |rendered - true depth| over the last 50 of 400 batches, three seeds, +- standard
error: `mse` with Config.depth_comp_iters = 3 0.0449 +- 0.0002, after Config.depth_acc_views = 4 as well 0.0441 +- 0.0002, plain
`mse` 0.1572 +- 0.0008, `gnll` with the completion's standard deviation 0.0308 +- 0.0004; rgb-only did not converge on that scene
(7.2 .. 34.8: its guide image is flat within a surface).
"""
import os
import re

import numpy as np
import pytest

torch = pytest.importorskip('torch')
pytestmark = pytest.mark.gpu

from tests import depth_complete_reference as R                                          # noqa: E402
from tests.test_gpu_mip360 import T, N, dev                                              # noqa: E402
from tests.test_depth_consistency import SHAPES, write_colmap_scene, write_nerfpp_scene   # noqa: E402
from tests.test_depth_accumulate import prior_of                                         # noqa: E402
from tests.test_depth_complete import CASES, FILLED, guide_of, std_of, bits          # noqa: E402

KINDS = ('sparse', 'invalids', 'exact')
RADII = (1, 4, 8)
ITERS = (1, 3, 16)
NAMES = ('depth', 'std', 'conf', 'origin', 'pass', 'rows')
_refs = {}


@pytest.fixture(scope='module')
def DCP():
    dev()
    from outdoor_nerf_depth_amd import depth_complete
    return depth_complete


def reference(shape, kind, with_std, radius):
    """{iters: the reference's outputs} for ITERS, from one run, computed once and shared (read-only).  With a standard deviation
    the guide is weak (sigma_colour 300), so that the spread gate has windows to refuse; without, it is the default 20."""
    key = (shape, kind, with_std, radius)
    if key not in _refs:
        ws, wc = R.tables(radius, 2.0, 300.0 if with_std else 20.0)
        _refs[key] = R.complete(prior_of(kind, shape), guide_of(shape), std_of(shape) if with_std else None, ws, wc, radius, max(ITERS),
                                snapshots=ITERS)
        for out in _refs[key].values():
            for a in out.values():
                a.setflags(write=False)
    return _refs[key]


def assert_equal(got, ref, tag=''):
    """the call's host outputs against the reference's: equal, the float32 planes as bits"""
    for name in NAMES:
        a, b = got[name], ref[name]
        assert a.dtype == b.dtype and a.shape == b.shape, (tag, name, a.dtype, b.dtype, a.shape, b.shape)
        np.testing.assert_array_equal(bits(a), bits(b), err_msg='%s: %s' % (tag, name))


def make_run(DCP):
    """the device call with the reference's signature; every result is also held against the reference"""
    def run(depth, rgb, std_in, w_space, w_colour, radius, iters, **kw):
        got = DCP.complete_async(T(depth), T(rgb), None if std_in is None else T(std_in), w_space=w_space, w_colour=w_colour, radius=radius,
                                 iters=iters, **kw).get()
        assert_equal(got, R.complete(depth, rgb, std_in, w_space, w_colour, radius, iters, **kw), 'r = %d, %d passes' % (radius, iters))
        return got
    return run


# ------------------------------------------------------------------------------------------------ 1. equality
@pytest.mark.parametrize('radius', RADII)
@pytest.mark.parametrize('with_std', (False, True), ids=('no_std', 'std'))
@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('shape', SHAPES)
def test_equal_to_the_reference(DCP, shape, kind, with_std, radius):
    refs = reference(shape, kind, with_std, radius)
    prior, rgb = T(prior_of(kind, shape)), T(guide_of(shape))
    std = T(std_of(shape)) if with_std else None
    for iters in ITERS:
        got = DCP.complete_async(prior, rgb, std, radius=radius, iters=iters, sigma_colour=300.0 if with_std else 20.0).get()
        tot = got['rows'].sum(0)
        print('%s %s std %s r = %d, %d passes: rows total %s' % (shape, kind, with_std, radius, iters, tot.tolist()))
        assert_equal(got, refs[iters], '%s %s r = %d, %d passes' % (shape, kind, radius, iters))
        if kind == 'sparse':
            assert tot[1] > 0 and tot[2] + tot[3] > 0                                          # the case has decisions to make
        if kind == 'exact':
            assert tot[1:].sum() == 0                                                          # a dense prior has nothing to fill


@pytest.mark.parametrize('case', CASES, ids=lambda c: c.__name__)
def test_hand_built_cases_on_the_device(DCP, case):
    case(make_run(DCP))


def test_other_parameters_and_frames_of_one_row_or_column(DCP):
    run = make_run(DCP)
    shape = SHAPES[1]
    prior, rgb, std = prior_of('sparse', shape), guide_of(shape), std_of(shape)
    ws, wc = R.tables(3, 1.0, 60.0)
    for kw in (dict(min_points=1, min_conf=0.0, max_rel_spread=float('inf'), decay=1.0), dict(min_points=5, min_conf=0.3, max_rel_spread=0.0, decay=0.25),
               dict(min_points=1, min_conf=0.0, max_rel_spread=0.02, decay=1e-30)):
        got = run(prior, rgb, std, ws, wc, 3, 4, **kw)
        print(kw, got['rows'].sum(0).tolist())
    for hw in ((1, 70), (70, 1), (17, 33)):                                                    # a row, a column, one past the tile both ways
        rs = np.random.RandomState(hw[0])
        depth = np.where(rs.rand(2, *hw) < 0.2, 3.0 + rs.rand(2, *hw), 0).astype(np.float32)
        got = run(depth, rs.randint(0, 256, (2,) + hw + (3,)).astype(np.uint8), None, ws, R.tables(3, 1.0, 200.0)[1], 3, 2,
                  min_points=1, min_conf=0.0, max_rel_spread=0.5, decay=0.5)
        assert got['rows'][:, 1].sum() > 0


# ------------------------------------------------------------------------------------------------ 2. outputs and reproducibility
def test_nullable_outputs_absent_and_depth_out_given(DCP):
    shape = SHAPES[1]
    prior, rgb = T(prior_of('sparse', shape)), T(guide_of(shape))
    for iters in (1, 2, 3):                                                                    # both parities of the ping-pong
        ref = R.complete(prior_of('sparse', shape), guide_of(shape), None, *R.tables(4, 2.0, 20.0), 4, iters)
        bare = DCP.complete_async(prior, rgb, iters=iters, conf=False, passes=False, rows=False)
        assert sorted(bare.tensors) == ['depth', 'origin', 'std']
        got = bare.get()
        for name in ('depth', 'std', 'origin'):
            np.testing.assert_array_equal(bits(got[name]), bits(ref[name]), err_msg=name)
        out = torch.empty_like(prior)
        full = DCP.complete_async(prior, rgb, iters=iters, depth_out=out)
        assert full.tensors['depth'] is out
        assert_equal(full.get(), ref, 'depth_out given, %d passes' % iters)
        d, s, o, rw = DCP.complete_priors(prior, rgb, iters=iters, std_floor=0.25)
        have = ref['conf'] > 0
        np.testing.assert_array_equal(N(d).view(np.int32), ref['depth'].view(np.int32))
        np.testing.assert_array_equal(N(s), np.where(have, np.maximum(ref['std'], np.float32(0.25)), np.float32(0)))
        np.testing.assert_array_equal(N(rw), ref['rows'])
    std = torch.ones_like(prior)
    for out, text in ((prior, 'depth_out overlaps depth'), (std, 'depth_out overlaps std_in'),
                      (torch.empty(prior.shape), 'depth_out on cpu: expected the device')):
        with pytest.raises(DCP.DepthCompError, match=text):
            DCP.complete_async(prior, rgb, std, depth_out=out)
    with pytest.raises(DCP.DepthCompError, match='w_space: 9 entries, expected 81'):
        DCP.complete_async(prior, rgb, w_space=np.ones(9))
    with pytest.raises(DCP.DepthCompError, match='w_colour: every entry must be finite and >= 0'):
        DCP.complete_async(prior, rgb, w_colour=-np.ones(766))


def test_same_call_twice_and_a_frame_alone_are_bit_identical(DCP):
    shape = SHAPES[2]
    prior, rgb, std = prior_of('invalids', shape), guide_of(shape), std_of(shape)
    kw = dict(radius=4, iters=3, sigma_colour=300.0)
    a = DCP.complete_async(T(prior), T(rgb), T(std), **kw).get()
    b = DCP.complete_async(T(prior), T(rgb), T(std), **kw).get()
    for k in a:
        np.testing.assert_array_equal(a[k].view(np.uint8), b[k].view(np.uint8), err_msg=k)
    for i in (0, 3, 7):
        c = DCP.complete_async(T(prior[i:i + 1]), T(rgb[i:i + 1]), T(std[i:i + 1]), **kw).get()
        for k in a:
            np.testing.assert_array_equal(a[k][i].view(np.uint8), c[k][0].view(np.uint8), err_msg='frame %d, %s' % (i, k))


# ------------------------------------------------------------------------------------------------ 3. the CLI on both layouts
def _sparsen(folder_in, folder_out, share=0.05, seed=7):
    """folder_out: the PNGs of folder_in with a `share` of their pixels kept and the others 0 (a sparse prior written by the test)"""
    from PIL import Image
    os.makedirs(str(folder_out), exist_ok=True)
    rs = np.random.RandomState(seed)
    for name in sorted(os.listdir(str(folder_in))):
        raw = np.asarray(Image.open(os.path.join(str(folder_in), name)))
        Image.fromarray(np.where(rs.rand(*raw.shape) < share, raw, 0).astype(np.uint16)).save(os.path.join(str(folder_out), name))


def _repaint(image_dir, depth_dir):
    """the images of a written scene replaced by guides that follow its surfaces (the textures the writers paint guide nothing)"""
    from PIL import Image
    for img, dep in zip(sorted(os.listdir(str(image_dir))), sorted(os.listdir(str(depth_dir)))):
        metres = np.asarray(Image.open(os.path.join(str(depth_dir), dep))).astype(np.float64) / 256.0
        Image.fromarray(R.guide(metres, seed=3)).save(os.path.join(str(image_dir), img))


@pytest.fixture(scope='module')
def colmap_scene(tmp_path_factory):
    dev()
    root = tmp_path_factory.mktemp('depth_comp_colmap') / 'scene'
    names, _ = write_colmap_scene(str(root), box=True)
    _repaint(root / 'images', root / 'depths_gt')
    _sparsen(root / 'depths_gt', root / 'depths_lidar')
    return root, names


def _nerfpp_scene(root):
    write_nerfpp_scene(str(root), F=8)
    for split in ('train', 'test'):
        _repaint(root / 'scene' / split / 'rgb', root / 'scene' / split / 'depth')
        _sparsen(root / 'scene' / split / 'depth', root / 'scene' / split / 'depth_lidar')


def _scene(data, sup_type, extra=()):
    from outdoor_nerf_depth_amd import mip360_data as D
    return D.Scene(D.parse_gin(bindings=["Config.data_dir = '%s'" % data, "Config.depth_sup_type = '%s'" % sup_type, 'Config.sample_every = 1'] + list(extra)))


def _report(path, names, rows):
    lines = open(str(path)).read().splitlines()
    assert len(lines) == 2 + len(names) and lines[-1].split()[:5] == ['total'] + [str(v) for v in rows.sum(0)]
    for i, name in enumerate(names):
        assert lines[1 + i].split()[:5] == [name] + [str(v) for v in rows[i]]
    return [float(v) for v in lines[-1].split()[5:]]


def _defaults(depth, rgb, std=None, **kw):
    """the reference at the binding's defaults, but for kw"""
    p = dict(R.DEFAULTS, **kw)
    ws, wc = R.tables(p['radius'], p['sigma_space'], p['sigma_colour'])
    return R.complete(depth, rgb, std, ws, wc, p['radius'], p['iters'], p['min_points'], p['min_conf'], p['max_rel_spread'], p['decay'])


def test_cli_on_a_colmap_scene(DCP, colmap_scene):
    from PIL import Image
    data, names = colmap_scene
    rows = DCP.main(['--data_dir', str(data), '--depth_sup_type', 'lidar', '--iters', '2', '--radius', '3'])
    scene = _scene(data, 'lidar')
    ref = _defaults(scene.depths_sup, scene.images, iters=2, radius=3)
    np.testing.assert_array_equal(rows, ref['rows'])
    filled, have = ref['origin'] == FILLED, ref['conf'] > 0
    assert filled.sum() > 5 * (scene.depths_sup > 0).sum()
    assert sorted(d for d in os.listdir(str(data)) if d.startswith('depths_lidar')) == ['depths_lidar', 'depths_lidar_comp', 'depths_lidar_comp_std']
    # the folders, read back through the loader under T_comp: own pixels exactly, filled ones within half a PNG step; the _std twin
    comp = _scene(data, 'lidar_comp', ["Config.depth_loss_type = 'gnll'"])
    np.testing.assert_array_equal(comp.depths_sup > 0, have)
    np.testing.assert_array_equal(comp.depths_sup[~filled], scene.depths_sup[~filled])
    err = np.abs(comp.depths_sup.astype(np.float64) - ref['depth'])[filled] / scene.scale
    print('colmap CLI: totals %s; filled pixels read back within %.3g m (half a PNG step is %.3g m)' % (rows.sum(0).tolist(), err.max(), 0.5 / 256))
    assert err.max() <= 0.5 / 256 + 1e-5
    assert comp.depth_std_source == 'folder' and ((comp.depths_std > 0) == have).all()
    want = np.maximum(ref['std'].astype(np.float64) / scene.scale, 2.0 / 256)
    assert (np.abs(comp.depths_std.astype(np.float64) / scene.scale - want)[have]).max() <= 0.5 / 256 + 1e-5
    for i, name in enumerate(scene.names):
        raw = np.asarray(Image.open(str(data / 'depths_lidar' / name)))
        out = np.asarray(Image.open(str(data / 'depths_lidar_comp' / name)))
        np.testing.assert_array_equal(out[~filled[i]], raw[~filled[i]])
        assert out.dtype == raw.dtype and (out[filled[i]] >= 2).all()
    cov_before, cov_after, absrel_filled = _report(data / 'complete_lidar.txt', scene.names, rows)
    print('colmap CLI: coverage %.3f -> %.3f, AbsRel of the filled %.5f' % (cov_before, cov_after, absrel_filled))
    assert abs(cov_before - (scene.depths_sup > 0).mean()) < 1e-6 and abs(cov_after - have.mean()) < 1e-6
    true = scene.depths_gt[filled].astype(np.float64)
    assert abs(absrel_filled - np.mean(np.abs(ref['depth'][filled] - true) / true)) < 1e-6


def test_cli_on_a_nerfpp_scene(DCP, tmp_path):
    from outdoor_nerf_depth_amd.data_loader_split import load_data_split
    _nerfpp_scene(tmp_path)
    done = DCP.main(['--datadir', str(tmp_path), '--scene', 'scene', '--depth_sup_type', 'lidar'])
    assert sorted(done) == ['test', 'train']
    for split in ('train', 'test'):
        before = load_data_split(str(tmp_path), 'scene', split, depth_sup_type='lidar')
        H, W, scale = before[0].H, before[0].W, before[0].depth_scale
        prior, rgb, _ = DCP._stack(before, split)
        ref = _defaults(prior, rgb)
        np.testing.assert_array_equal(done[split], ref['rows'])
        filled, have = ref['origin'] == FILLED, ref['conf'] > 0
        print('nerfpp CLI %s: totals %s' % (split, ref['rows'].sum(0).tolist()))
        assert filled.sum() > 5 * (prior > 0).sum()
        after = load_data_split(str(tmp_path), 'scene', split, depth_sup_type='lidar_comp', depth_std=0.0)
        got = np.stack([s.depth_sup.reshape(H, W) for s in after], 0)
        np.testing.assert_array_equal(got[~filled], prior[~filled])
        assert (np.abs(got.astype(np.float64) - ref['depth'])[filled] / scale).max() <= 0.5 / 256 + 1e-5
        std = np.stack([s.depth_std.reshape(H, W) for s in after], 0)                          # the _std twin, found by the loader
        assert ((std > 0) == have).all()
        assert sorted(d for d in os.listdir(str(tmp_path / 'scene' / split)) if d.startswith('depth_lidar')) == \
            ['depth_lidar', 'depth_lidar_comp', 'depth_lidar_comp_std']
        names = sorted(os.listdir(str(tmp_path / 'scene' / split / 'depth_lidar_comp')))
        assert len(_report(tmp_path / 'scene' / split / 'complete_lidar.txt', names, ref['rows'])) == 3


# ------------------------------------------------------------------------------------------------ 4. the load-time flags
COMP = ['Config.depth_comp_iters = 2', 'Config.depth_comp_radius = 3']


def test_mip360_flag_completes_the_training_split_only_and_last(DCP, colmap_scene, tmp_path):
    from outdoor_nerf_depth_amd import depth_accumulate as DA
    from outdoor_nerf_depth_amd import mip360_data as D
    from tests.test_gpu_depth_consistency import _one_mip360_step
    from tests.test_gpu_mip360_app import _run
    data = colmap_scene[0]
    base = ["Config.data_dir = '%s'" % data, "Config.depth_sup_type = 'lidar'", 'Config.sample_every = 1', 'Config.batch_size = 256']
    plain = D.Scene(D.parse_gin(bindings=base))
    raw = plain.device_frames('train', dev())
    assert 'depth_comp_rows' not in raw
    cfg = D.parse_gin(bindings=base + COMP)
    scene = D.Scene(cfg)
    train = scene.device_frames('train', dev())
    ref = _defaults(N(raw['depth_sup']), N(raw['rgb_u8']), iters=2, radius=3)
    np.testing.assert_array_equal(N(train['depth_sup']).view(np.int32), ref['depth'].view(np.int32))       # the float32 value, unquantised
    np.testing.assert_array_equal(N(train['depth_comp_rows']), ref['rows'])
    assert ref['rows'][:, 1].sum() > 0 and 'depth_std' not in train
    test = scene.device_frames('test', dev())
    assert torch.equal(test['depth_sup'], plain.device_frames('test', dev())['depth_sup']) and 'depth_comp_rows' not in test
    b, sc = _one_mip360_step(scene, train, cfg)                                              # the step's prior is the completed one
    f, x, y = b['pix'].long().unbind(1)
    assert torch.equal(b['depth_sup'].reshape(-1), train['depth_sup'][f, y, x]) and np.isfinite(sc).all()
    assert int((raw['depth_sup'][f, y, x] != train['depth_sup'][f, y, x]).sum()) > 0
    # after the accumulation: the completion sees the accumulated prior
    acc = ['Config.depth_acc_views = 2']
    both = D.Scene(D.parse_gin(bindings=base + acc + COMP)).device_frames('train', dev())
    denser, _, acc_rows = DA.accumulate_priors(raw['depth_sup'], DA.cams_from_scene(plain, plain.train), 2)
    ref_both = _defaults(N(denser), N(raw['rgb_u8']), iters=2, radius=3)
    np.testing.assert_array_equal(N(both['depth_sup']).view(np.int32), ref_both['depth'].view(np.int32))
    np.testing.assert_array_equal(N(both['depth_comp_rows']), ref_both['rows'])
    assert torch.equal(both['depth_acc_rows'], acc_rows) and ref_both['rows'][:, 0].sum() > ref['rows'][:, 0].sum()
    # a gnll run: a constant goes in as the measurements' standard deviation, the completion's, floored, comes out
    gn = ["Config.depth_loss_type = 'gnll'", 'Config.depth_gnll_std = 0.05', 'Config.depth_comp_std_floor = 0.02']
    g_scene = D.Scene(D.parse_gin(bindings=base + COMP + gn))
    g = g_scene.device_frames('train', dev())
    const = np.full(ref['depth'].shape, g_scene.depth_std_const, np.float32)
    ref_g = _defaults(N(raw['depth_sup']), N(raw['rgb_u8']), const, iters=2, radius=3)
    floor = np.float32(0.02 * g_scene.scale)
    np.testing.assert_array_equal(N(g['depth_std']), np.where(ref_g['conf'] > 0, np.maximum(ref_g['std'], floor), np.float32(0)))
    np.testing.assert_array_equal(N(g['depth_sup']).view(np.int32), ref['depth'].view(np.int32))
    alone = D.Scene(D.parse_gin(bindings=base + COMP + gn[:1])).device_frames('train', dev())   # no other source: the completion's own
    np.testing.assert_array_equal(N(alone['depth_std']), ref['std'])
    # the trainer: one log line with the totals, the flag alone and after the accumulation's
    tail = ['Config.max_steps = 2', 'Config.checkpoint_every = 100', 'Config.print_every = 1', 'Config.lr_delay_steps = 0',
            'Config.render_chunk_size = 1024']
    for extra, want in ((COMP, [DCP.totals_line(ref['rows'], 2)]),
                        (acc + COMP, [DA.totals_line(N(acc_rows), 2), DCP.totals_line(ref_both['rows'], 2)])):
        bind = base + extra + ["Config.checkpoint_dir = '%s'" % (tmp_path / ('run%d' % len(extra)))] + tail
        out = _run('mip360_train', sum([['--gin_bindings', x] for x in bind], []))
        lines = [l for l in out.splitlines() if l.startswith('depth ')]
        print(lines)
        assert lines == want, out[-2000:]
        assert 'step 2/2' in out


def test_nerfpp_flag_completes_the_samplers(DCP, tmp_path):
    from outdoor_nerf_depth_amd import depth_accumulate as DA
    from outdoor_nerf_depth_amd.data_loader_split import load_data_split
    from outdoor_nerf_depth_amd.device_sampler import DeviceRaySamplers
    from tests.test_gpu_depth_consistency import _run_nerfpp
    _nerfpp_scene(tmp_path)
    samplers = load_data_split(str(tmp_path), 'scene', 'train', depth_sup_type='lidar')
    held_out = load_data_split(str(tmp_path), 'scene', 'test', depth_sup_type='lidar')
    untouched = [s.depth_sup.copy() for s in held_out]
    prior, rgb, _ = DCP._stack(samplers, 'train')
    ref = _defaults(prior, rgb, radius=2)
    rows = DCP.complete_samplers(samplers, dev(), radius=2)
    np.testing.assert_array_equal(rows, ref['rows'])
    assert rows[:, 1].sum() > 0 and all(s.depth_std is None for s in samplers)
    for i, s in enumerate(samplers):                                                           # host sampling reads these
        np.testing.assert_array_equal(s.depth_sup.view(np.int32), ref['depth'][i].reshape(-1).view(np.int32))
    ds = DeviceRaySamplers(samplers, dev(), seed=1)                                            # and so does the device sampler
    np.testing.assert_array_equal(N(ds.depth_sup).reshape(len(samplers), -1), ref['depth'].reshape(len(samplers), -1))
    assert all(np.array_equal(s.depth_sup, u) for s, u in zip(held_out, untouched))
    fresh = load_data_split(str(tmp_path), 'scene', 'train', depth_sup_type='lidar')
    DCP.complete_samplers(fresh, dev(), want_std=True, radius=2, std_floor=0.01)               # no source: the completion's own, floored
    want = np.where(ref['conf'] > 0, np.maximum(ref['std'], np.float32(0.01)), np.float32(0))
    for i, s in enumerate(fresh):
        np.testing.assert_array_equal(s.depth_std, want[i].reshape(-1))
    # the trainer's own flags on the written scene: one log line with the totals, alone and after the accumulation's
    cams = DA.cams_from_samplers(samplers)
    denser, _, acc_rows = DA.accumulate_priors(T(prior), cams, 2)
    ref_both = _defaults(N(denser), rgb)
    argv = ['--basedir', str(tmp_path), '--datadir', str(tmp_path), '--scene', 'scene', '--cascade_samples', '16,16', '--use_depth',
            '--depth_sup_type', 'lidar', '--lambda_depth', '0.1', '--world_size', '1', '--N_rand_override', '128', '--i_weights', '100',
            '--i_test', '100', '--i_print', '1', '--N_iters', '2', '--testskip', '1', '--depth_comp_iters', '3']
    for extra, want in ((['--expname', 'comp'], [DCP.totals_line(_defaults(prior, rgb)['rows'], 3)]),
                        (['--expname', 'both', '--depth_acc_views', '2'], [DA.totals_line(N(acc_rows), 2), DCP.totals_line(ref_both['rows'], 3)])):
        text = _run_nerfpp(argv + extra)
        found = [l for l in text.splitlines() if l.startswith('depth ')]
        print(found)
        assert found == want, text[-2000:]
        assert len(re.findall(r'step: \d+ .*level_1/loss_depth: [-\d.e+]+ ', text)) == 2, text[-2000:]


def test_without_the_flags_the_library_is_never_loaded(DCP, colmap_scene, monkeypatch, tmp_path):
    """with the library unloaded and its path pointing nowhere, both trainers load their frames and step; with the flags they do not"""
    from outdoor_nerf_depth_amd import mip360_data as D
    from tests.test_gpu_depth_consistency import _one_mip360_step, _run_nerfpp, _nerfpp_argv
    monkeypatch.setattr(DCP, '_lib', None)
    monkeypatch.setattr(DCP, 'LIB_PATH', str(tmp_path / 'libdepthcomp_hip.so'))
    base = ["Config.data_dir = '%s'" % colmap_scene[0], "Config.depth_sup_type = 'lidar'", 'Config.sample_every = 1', 'Config.batch_size = 256']
    cfg = D.parse_gin(bindings=base)
    scene = D.Scene(cfg)
    _, sc = _one_mip360_step(scene, scene.device_frames('train', dev()), cfg)
    assert np.isfinite(sc).all()
    text = _run_nerfpp(_nerfpp_argv(tmp_path))
    assert 'depth completion' not in text and len(re.findall(r'step: \d+ ', text)) == 2
    assert DCP._lib is None
    with pytest.raises(DCP.DepthCompError, match='libdepthcomp_hip.so not found'):
        D.Scene(D.parse_gin(bindings=base + COMP)).device_frames('train', dev())
    with pytest.raises(DCP.DepthCompError, match='libdepthcomp_hip.so not found'):
        _run_nerfpp(_nerfpp_argv(tmp_path, 'l1', ['--depth_comp_iters', '2']))
    assert DCP._lib is None

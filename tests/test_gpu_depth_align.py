"""GPU: aligning relative depth priors to sparse metric depth (depthalign_fit_apply, csrc/depthalign_kernels.hip) against
tests/depth_align_reference.py, through the CLI on both on-disk layouts and through the load-time flags of both trainers.

Gates.  The kernels evaluate the reference's float64 expressions without contraction; their sums run in another (fixed) order.
  rows       s, b, sigma and rms within rtol 1e-9 (b relative to |b| + |s| max |x|): three orders over the order sensitivity that
             tests/test_depth_align.py measures and asserts (<= 1e-11) on these very inputs; n_pairs, n_inliers, status and iterations
             EQUAL (no residual of these inputs lies within 1e-6 of the 3 sigma bound, asserted there too).
  pixels     depth_out and std_out BIT-EQUAL to the reference's apply step evaluated with the device's own row: the apply step has no
             sum in it; and within 2 float32 ulp of the full reference.
The inputs are tests/test_depth_align.py's CASES: 0.2 % noise, 30 % of the anchors multiplied by 1.3 .. 2.5, a tenth of the other
pixels each 0, negative and NaN.

Measured on an MI355X (reported figures, not gates).  Rows within 4.5e-11 of the reference at worst (the on-disk scenes; 1.2e-12 on
CASES), every depth_out and std_out 0 ulp from the full reference.  One call on 295 frames of 375 x 1242 in disparity space
(tools/depth_align_bench.py, profiles/depth_align_time.json): a 5 % anchor 1.35 ms in its launches (count 0.20, scan 0.005, pairs
0.21, fit 0.49, apply 0.44) and 1.34 ms through the binding, 3.8 times its compulsory 2.20 GB at 6.2 TB/s; a dense anchor 10.64 ms
(fit 9.6: float64 divides, one CU per frame), 30 times.  Flags off, the `mse` step against the parent commit, medians of 3
alternating runs: MipNeRF-360 7.280 against 7.306 ms (the parent's spread 0.030), NeRF++ 2.0084 against 2.0114 ms (spread 0.012).
Training effect on the scene whose priors are distorted per frame, mean |rendered - true depth| over the last 50 of 400 batches, three
seeds: `mse` on the aligned prior 0.194, on the raw prior 0.876, rgb-only 2.16 and 1.98 with one seed diverged.
"""
import os
import re

import numpy as np
import pytest

torch = pytest.importorskip('torch')
pytestmark = pytest.mark.gpu

from tests import depth_align_reference as R                                             # noqa: E402
from tests.test_gpu_mip360 import T, N, dev                                              # noqa: E402
from tests.test_depth_consistency import write_colmap_scene, write_nerfpp_scene         # noqa: E402
from tests.test_depth_align import CASES, inputs, reference, statuses_batch, absrel     # noqa: E402


@pytest.fixture(scope='module')
def DAL():
    dev()
    from outdoor_nerf_depth_amd import depth_align
    return depth_align


def ulps(a, b):
    """distance in float32 steps between two float32 arrays of positive or zero values"""
    return np.abs(a.view(np.int32).astype(np.int64) - b.view(np.int32).astype(np.int64))


def assert_rows(rows, want, prior, anchor, tag, space='depth'):
    """the rows gate; returns the worst relative difference of s, b, sigma, rms"""
    assert rows.dtype == np.float64 and rows.shape == want.shape
    np.testing.assert_array_equal(rows[:, 3:7], want[:, 3:7], err_msg='%s: n_pairs, n_inliers, status, iterations' % tag)
    worst = 0.0
    for f in range(len(rows)):
        x, _ = R.pairs(prior[f], anchor[f], space)
        if want[f, 5] != 0:
            assert not rows[f, [0, 1, 2, 7]].any(), (tag, f)
            continue
        scale = np.array([abs(want[f, 0]), abs(want[f, 1]) + abs(want[f, 0]) * x.max(), want[f, 2], want[f, 7]])
        err = np.abs(rows[f, [0, 1, 2, 7]] - want[f, [0, 1, 2, 7]]) / scale
        worst = max(worst, err.max())
    assert worst <= 1e-9, (tag, worst)
    return worst


def assert_matches(got, prior, anchor, ref, tag, **params):
    """the call's host outputs against the reference's under the gates of this file's docstring"""
    rows = got['rows']
    worst = assert_rows(rows, ref['rows'], prior, anchor, tag, params.get('space', 'depth'))
    apply_kw = {k: v for k, v in params.items() if k in ('space', 'max_depth', 'keep_anchor', 'std_floor')}
    d_own, s_own = R.apply(prior, anchor, rows, **apply_kw)
    far = int(ulps(got['depth'], ref['depth_out']).max())
    print('%s: rows within %.2g of the reference (gate 1e-9), depth_out within %d ulp of the full reference' % (tag, worst, far))
    np.testing.assert_array_equal(got['depth'].view(np.int32), d_own.view(np.int32), err_msg='%s: depth_out under the device\'s row' % tag)
    if 'std' in got:
        np.testing.assert_array_equal(got['std'].view(np.int32), s_own.view(np.int32), err_msg='%s: std_out under the device\'s row' % tag)
        assert ulps(got['std'], ref['std_out']).max() <= 2, tag
    assert far <= 2, tag


# ------------------------------------------------------------------------------------------------ 1. against the reference
@pytest.mark.parametrize('iters', (0, 10))
@pytest.mark.parametrize('space', R.SPACES)
@pytest.mark.parametrize('case', sorted(CASES))
def test_matches_the_reference(DAL, case, space, iters):
    p, a, _ = inputs(case, space)
    got = DAL.align_async(T(p), T(a), space=space, iters=iters).get()
    assert_matches(got, p, a, reference(case, space, iters=iters), '%s %s K = %d' % (case, space, iters), space=space)
    counts = [c if c >= 0 else p.shape[1] * p.shape[2] for c in CASES[case][1]]
    assert got['rows'][:, 3].tolist() == counts


@pytest.mark.parametrize('space', R.SPACES)
def test_one_frame_of_each_status_in_one_batch(DAL, space):
    p, a = statuses_batch(space)
    got = DAL.align_async(T(p), T(a), space=space).get()
    assert got['rows'][:, 5].tolist() == [0, 1, 2, 3]
    assert_matches(got, p, a, R.align(p, a, space=space), 'statuses %s' % space, space=space)
    assert not got['depth'][1:].any() and not got['std'][1:].any() and (got['depth'][0] > 0).all()


def test_keep_anchor_max_depth_std_floor_and_other_parameters(DAL):
    for space, case in (('depth', 'tile'), ('disparity', 'tile'), ('depth', 'few')):
        p, a, _ = inputs(case, space)
        for kw in (dict(keep_anchor=True), dict(max_depth=30.0), dict(keep_anchor=True, max_depth=20.0, std_floor=0.5), dict(c=2.0, min_points=2, iters=3),
                   dict(std_floor=0.01)):
            got = DAL.align_async(T(p), T(a), space=space, **kw).get()
            assert_matches(got, p, a, R.align(p, a, space=space, **kw), '%s %s %s' % (case, space, kw), space=space, **kw)
            if kw.get('keep_anchor'):
                own = a > 0
                np.testing.assert_array_equal(got['depth'][own].view(np.int32), a[own].view(np.int32))
                assert (got['std'][own] == np.float32(kw.get('std_floor', 0.0))).all()
            if 'max_depth' in kw and not kw.get('keep_anchor') and case == 'tile':
                assert got['depth'].max() <= kw['max_depth'] and (got['depth'] > 0).sum() < (R.align(p, a, space=space)['depth_out'] > 0).sum()


def test_null_std_out_and_sentinels_are_fully_overwritten(DAL):
    p, a, _ = inputs('tile', 'disparity')
    ref = reference('tile', 'disparity')
    bare = DAL.align_async(T(p), T(a), std=False, space='disparity')
    assert sorted(bare.tensors) == ['depth', 'rows']
    full = DAL.align_async(T(p), T(a), space='disparity')
    assert torch.equal(bare.tensors['depth'].view(torch.int32), full.tensors['depth'].view(torch.int32))
    assert torch.equal(bare.tensors['rows'].view(torch.int64), full.tensors['rows'].view(torch.int64))
    out = {'depth': torch.full(p.shape, -7.0, device=dev()), 'std': torch.full(p.shape, -7.0, device=dev()),
           'rows': torch.full((p.shape[0], 8), -7.0, dtype=torch.float64, device=dev())}
    again = DAL.enqueue(T(p), T(a), DAL.check_params(space='disparity'), out=out)
    assert again.tensors is out
    for k in out:
        assert torch.equal(out[k].view(torch.uint8), full.tensors[k].view(torch.uint8)), k
    assert not (N(out['depth']) == -7.0).any() and not (N(out['std']) == -7.0).any()
    assert_matches(again.get(), p, a, ref, 'sentinels', space='disparity')


def test_a_batch_equals_single_calls_and_a_call_repeats_bit_for_bit(DAL):
    for space in R.SPACES:
        p, a, _ = inputs('tile', space)
        x = DAL.align_async(T(p), T(a), space=space).get()
        y = DAL.align_async(T(p), T(a), space=space).get()
        for k in x:
            np.testing.assert_array_equal(x[k].view(np.uint8), y[k].view(np.uint8), err_msg='twice: %s' % k)
        for f in range(p.shape[0]):                                                          # a frame alone: its base is aligned, in the batch
            one = DAL.align_async(T(p[f:f + 1]), T(a[f:f + 1]), space=space).get()             # frames 1 and 3 start 8 bytes off 16
            for k in x:
                np.testing.assert_array_equal(x[k][f].view(np.uint8), one[k][0].view(np.uint8), err_msg='frame %d alone: %s' % (f, k))
        pair = DAL.align_async(T(p[[4, 2]]), T(a[[4, 2]]), space=space).get()                  # and in another batch, in another slot
        for k in x:
            np.testing.assert_array_equal(x[k][[4, 2]].view(np.uint8), pair[k].view(np.uint8), err_msg='reordered: %s' % k)


def test_misaligned_bases_take_the_4_byte_path_with_the_same_bits(DAL):
    p, a, _ = inputs('tile', 'depth')
    x = DAL.align_async(T(p), T(a)).tensors
    n = p.size
    bufs = [torch.zeros(n + 4, device=dev()) for _ in range(2)]
    views = []
    for b, src in zip(bufs, (p, a)):
        v = b[1:1 + n].view(p.shape)                                                         # 4 bytes off a 16-byte boundary
        v.copy_(T(src))
        views.append(v)
    assert views[0].data_ptr() % 16 == 4
    y = DAL.align_async(views[0], views[1]).tensors
    for k in x:
        assert torch.equal(x[k].view(torch.uint8), y[k].view(torch.uint8)), k


def test_workspace_reuse_and_refusals_on_the_device(DAL):
    for case in ('tile', 'waves', 'tile'):
        p, a, _ = inputs(case, 'depth')
        assert_matches(DAL.align_async(T(p), T(a)).get(), p, a, reference(case, 'depth'), 'reuse %s' % case)
    assert len(DAL._workspaces) == 2
    p, a, _ = inputs('tiny', 'depth')
    with pytest.raises(DAL.DepthAlignError, match='prior and anchor live on different devices'):
        DAL.align_async(T(p), torch.from_numpy(np.array(a)))
    with pytest.raises(DAL.DepthAlignError, match=r'prior \(1, 7, 13\) and anchor \(1, 13, 7\) differ in shape'):
        DAL.align_async(T(p), T(a).reshape(1, 13, 7))
    with pytest.raises(DAL.DepthAlignError, match='iters = 33'):
        DAL.align_async(T(p), T(a), iters=33)
    d, s, rows = DAL.align_priors(T(p), T(a))
    assert d.shape == s.shape == p.shape and rows.shape == (1, 8) and rows.dtype == torch.float64


# ------------------------------------------------------------------------------------------------ 2. the CLI on both layouts
def _distort_folder(folder_gt, folder_out, space, seed):
    """folder_out: every PNG of folder_gt distorted by a random (alpha, beta) of its own -- in depth space p = (z - beta) / alpha,
    in disparity space p = 100 (1 / z + beta) / alpha -- written like a prior (uint16 of the value x 256)"""
    from PIL import Image
    os.makedirs(str(folder_out), exist_ok=True)
    rs = np.random.RandomState(seed)
    for name in sorted(os.listdir(str(folder_gt))):
        z = np.asarray(Image.open(os.path.join(str(folder_gt), name))).astype(np.float64) / 256.0
        alpha, beta = rs.uniform(0.5, 2.0), rs.uniform(0.1, 1.0)
        p = (z - beta) / alpha if space == 'depth' else 100.0 * (1.0 / z + 0.05 * beta) / alpha
        Image.fromarray(np.clip(np.rint(p * 256.0), 2, 65535).astype(np.uint16)).save(os.path.join(str(folder_out), name))


def _sparsen(folder_in, folder_out, share=0.1, seed=7):
    from PIL import Image
    os.makedirs(str(folder_out), exist_ok=True)
    rs = np.random.RandomState(seed)
    for name in sorted(os.listdir(str(folder_in))):
        raw = np.asarray(Image.open(os.path.join(str(folder_in), name)))
        Image.fromarray(np.where(rs.rand(*raw.shape) < share, raw, 0).astype(np.uint16)).save(os.path.join(str(folder_out), name))


def _colmap(root, F):
    names, _ = write_colmap_scene(str(root), F=F, box=True)
    _distort_folder(root / 'depths_gt', root / 'depths_mono', 'depth', 3)
    _sparsen(root / 'depths_gt', root / 'depths_lidar')
    return names


def _scene(data, sup_type, extra=()):
    from outdoor_nerf_depth_amd import mip360_data as D
    return D.Scene(D.parse_gin(bindings=["Config.data_dir = '%s'" % data, "Config.depth_sup_type = '%s'" % sup_type, 'Config.sample_every = 1'] + list(extra)))


def _report_rows(path, names):
    lines = open(str(path)).read().splitlines()
    assert lines[0].startswith('# frame s b sigma n_pairs') and [l.split()[0] for l in lines[1:1 + len(names)]] == list(names)
    return np.array([[float(v) for v in l.split()[1:]] for l in lines[1:1 + len(names)]]), lines[1 + len(names):]


def test_cli_on_a_colmap_scene(DAL, tmp_path):
    data = tmp_path / 'scene'
    names = _colmap(data, 4)
    rows = DAL.main(['--data_dir', str(data), '--depth_sup_type', 'mono', '--anchor_sup_type', 'lidar', '--std_floor', '0.01'])
    raw, lidar = _scene(data, 'mono'), _scene(data, 'lidar')
    ref = R.align(raw.depths_sup, lidar.depths_sup, std_floor=0.01 * raw.scale)
    print('colmap CLI: rows within %.2g of the reference' % assert_rows(rows, ref['rows'], raw.depths_sup, lidar.depths_sup, 'colmap CLI'))
    assert (rows[:, 5] == 0).all()
    got = _scene(data, 'mono_aligned', ["Config.depth_loss_type = 'gnll'"])                # the folder and its _std twin, through the loader
    valid = ref['depth_out'] > 0
    np.testing.assert_array_equal(got.depths_sup > 0, valid)
    assert (np.abs(got.depths_sup.astype(np.float64) - ref['depth_out'])[valid] / raw.scale).max() <= 0.5 / 256 + 1e-5
    assert got.depth_std_source == 'folder' and (got.depths_std[valid] >= 0.01 * raw.scale * (1 - 1e-6)).all()
    before, after = absrel(raw.depths_sup, raw.depths_gt, raw.depths_sup > 0), absrel(got.depths_sup, got.depths_gt, got.depths_sup > 0)
    print('colmap CLI: AbsRel against ground truth %.4f before, %.4f after' % (before, after))
    assert after < 0.01 < before
    table, tail = _report_rows(data / 'align_mono.txt', raw.names)
    np.testing.assert_allclose(table[:, :8], rows, rtol=1e-10)
    assert (table[:, 9] < table[:, 8]).all() and tail[0].startswith('total 4 fitted of 4 ') and len(tail) == 1


def test_cli_on_a_nerfpp_scene_in_disparity_space_names_the_frame_that_is_not_fitted(DAL, tmp_path):
    from PIL import Image
    from outdoor_nerf_depth_amd.data_loader_split import load_data_split
    write_nerfpp_scene(str(tmp_path), F=8)
    for split in ('train', 'test'):
        _distort_folder(tmp_path / 'scene' / split / 'depth', tmp_path / 'scene' / split / 'depth_mono', 'disparity', 4)
        _sparsen(tmp_path / 'scene' / split / 'depth', tmp_path / 'scene' / split / 'depth_lidar')
    first = sorted(os.listdir(str(tmp_path / 'scene' / 'test' / 'depth_lidar')))[0]
    blank = tmp_path / 'scene' / 'test' / 'depth_lidar' / first                              # one test frame without a single measurement
    Image.fromarray(np.zeros_like(np.asarray(Image.open(str(blank))))).save(str(blank))
    done = DAL.main(['--datadir', str(tmp_path), '--scene', 'scene', '--depth_sup_type', 'mono', '--anchor_sup_type', 'lidar', '--space', 'disparity'])
    assert sorted(done) == ['test', 'train'] and done['train'].shape == (4, 8)
    for split in ('train', 'test'):
        before = load_data_split(str(tmp_path), 'scene', split, depth_sup_type='mono')
        anchors = load_data_split(str(tmp_path), 'scene', split, depth_sup_type='lidar')
        H, W, scale = before[0].H, before[0].W, before[0].depth_scale
        stack = lambda ss, key: np.stack([getattr(s, key).reshape(H, W) for s in ss], 0)
        prior, anchor, gt = stack(before, 'depth_sup'), stack(anchors, 'depth_sup'), stack(before, 'depth_gt')
        ref = R.align(prior, anchor, space='disparity')
        assert_rows(done[split], ref['rows'], prior, anchor, 'nerfpp CLI %s' % split, 'disparity')
        after = stack(load_data_split(str(tmp_path), 'scene', split, depth_sup_type='mono_aligned', depth_std=0.0), 'depth_sup')
        valid = ref['depth_out'] > 0
        np.testing.assert_array_equal(after > 0, valid)
        assert (np.abs(after.astype(np.float64) - ref['depth_out'])[valid] / scale).max() <= 0.5 / 256 + 1e-5
        e0, e1 = absrel(prior, gt, prior > 0), absrel(after, gt, after > 0)
        print('nerfpp CLI %s: AbsRel against ground truth %.4f before, %.4f after' % (split, e0, e1))
        assert e1 < 0.02 < e0
        names = sorted(os.listdir(str(tmp_path / 'scene' / split / 'depth_mono_aligned')))
        assert names == sorted(os.listdir(str(tmp_path / 'scene' / split / 'depth_mono_aligned_std')))
        table, tail = _report_rows(tmp_path / 'scene' / split / 'align_mono.txt', names)
        np.testing.assert_allclose(table[:, :8], done[split], rtol=1e-10)
        if split == 'test':
            assert done[split][0, 5] == 1 and not after[0].any() and tail[1:] == ['not fitted: %s (too few pairs)' % first]
        else:
            assert (done[split][:, 5] == 0).all() and len(tail) == 1
    with pytest.raises(DAL.DepthAlignError, match="--anchor_sup_type = 'mono' is the prior itself"):
        DAL.main(['--datadir', str(tmp_path), '--scene', 'scene', '--depth_sup_type', 'mono', '--anchor_sup_type', 'mono'])


# ------------------------------------------------------------------------------------------------ 3. the load-time flags
ALIGN = ["Config.depth_align_anchor = 'lidar'", 'Config.depth_align_iters = 8']


@pytest.fixture(scope='module')
def colmap_scene(tmp_path_factory):
    dev()
    root = tmp_path_factory.mktemp('depth_align_colmap') / 'scene'
    return root, _colmap(root, 12)


def test_mip360_flag_aligns_the_training_split_only_and_before_the_accumulation(DAL, colmap_scene, tmp_path):
    from outdoor_nerf_depth_amd import depth_accumulate as DA
    from outdoor_nerf_depth_amd import mip360_data as D
    from tests.test_gpu_depth_consistency import _one_mip360_step
    data = colmap_scene[0]
    base = ["Config.data_dir = '%s'" % data, "Config.depth_sup_type = 'mono'", 'Config.sample_every = 1', 'Config.batch_size = 256']
    plain = D.Scene(D.parse_gin(bindings=base))
    raw = plain.device_frames('train', dev())
    assert 'depth_align_rows' not in raw
    cfg = D.parse_gin(bindings=base + ALIGN)
    scene = D.Scene(cfg)
    train = scene.device_frames('train', dev())
    anchor = _scene(data, 'lidar').depths_sup[plain.train]
    ref = R.align(N(raw['depth_sup']), anchor, iters=8)
    got = dict(depth=N(train['depth_sup']), rows=train['depth_align_rows'].cpu().numpy())
    assert_matches(got, N(raw['depth_sup']), anchor, ref, 'mip360 flag', iters=8)              # the float32 value, unquantised
    assert (got['rows'][:, 5] == 0).all() and 'depth_std' not in train
    test = scene.device_frames('test', dev())
    assert torch.equal(test['depth_sup'], plain.device_frames('test', dev())['depth_sup']) and 'depth_align_rows' not in test
    b, sc = _one_mip360_step(scene, train, cfg)                                            # the step's prior is the aligned one
    f, x, y = b['pix'].long().unbind(1)
    assert torch.equal(b['depth_sup'].reshape(-1), train['depth_sup'][f, y, x]) and np.isfinite(sc).all()
    e0 = absrel(N(raw['depth_sup']), N(raw['depth_gt']), N(raw['depth_sup']) > 0)
    e1 = absrel(got['depth'], N(train['depth_gt']), got['depth'] > 0)
    print('mip360 flag: AbsRel of the training prior %.4f -> %.4f' % (e0, e1))
    assert e1 < 0.01 < e0
    # a gnll run without folder or constant takes the fit's standard deviation, ahead of the consistency check's
    g = D.Scene(D.parse_gin(bindings=base + ALIGN + ["Config.depth_loss_type = 'gnll'", 'Config.depth_cons_views = 2'])).device_frames('train', dev())
    want_d, want_s, _ = DAL.align_priors(raw['depth_sup'], T(anchor), iters=8)
    assert g['depth_std'].shape == want_s.shape and 'depth_cons_rows' in g
    assert torch.equal(g['depth_std'], want_s) and float(want_s.max()) > 0
    # with the accumulation also on, it sees the aligned prior
    both = D.Scene(D.parse_gin(bindings=base + ALIGN + ['Config.depth_acc_views = 2'])).device_frames('train', dev())
    want, _, rows = DA.accumulate_priors(want_d, DA.cams_from_scene(plain, plain.train), 2)
    assert torch.equal(both['depth_sup'], want) and torch.equal(both['depth_acc_rows'], rows)
    # the trainer: one log line with the totals, before the accumulation's
    from tests.test_gpu_mip360_app import _run
    bind = base + ALIGN + ['Config.depth_acc_views = 2', "Config.checkpoint_dir = '%s'" % (tmp_path / 'run'), 'Config.max_steps = 2',
                           'Config.checkpoint_every = 100', 'Config.print_every = 1', 'Config.lr_delay_steps = 0', 'Config.render_chunk_size = 1024']
    out = _run('mip360_train', sum([['--gin_bindings', x] for x in bind], []))
    lines = [l for l in out.splitlines() if l.startswith('depth ')]
    print(lines)
    assert lines[0] == DAL.totals_line(got['rows'], 'lidar') and lines[1].startswith('depth accumulation (2 views)') and len(lines) == 2, out[-2000:]
    assert 'step 2/2' in out


def _nerfpp_scene(tmp_path):
    write_nerfpp_scene(str(tmp_path), F=8)
    for split in ('train', 'test'):
        _distort_folder(tmp_path / 'scene' / split / 'depth', tmp_path / 'scene' / split / 'depth_mono', 'depth', 5)
        _sparsen(tmp_path / 'scene' / split / 'depth', tmp_path / 'scene' / split / 'depth_lidar')


def test_nerfpp_flag_aligns_the_samplers(DAL, tmp_path):
    from outdoor_nerf_depth_amd.data_loader_split import load_data_split
    from outdoor_nerf_depth_amd.device_sampler import DeviceRaySamplers
    from tests.test_gpu_depth_consistency import _run_nerfpp
    _nerfpp_scene(tmp_path)
    samplers = load_data_split(str(tmp_path), 'scene', 'train', depth_sup_type='mono', depth_std=0.0, depth_std_optional=True)
    anchors = load_data_split(str(tmp_path), 'scene', 'train', depth_sup_type='lidar')
    H, W = samplers[0].H, samplers[0].W
    stack = lambda ss: np.stack([s.depth_sup.reshape(H, W) for s in ss], 0)
    prior, anchor = stack(samplers), stack(anchors)
    ref = R.align(prior, anchor)
    rows = DAL.align_samplers(samplers, anchors, dev(), want_std=True)
    got = dict(rows=rows, depth=stack(samplers), std=np.stack([s.depth_std.reshape(H, W) for s in samplers], 0))
    assert_matches(got, prior, anchor, ref, 'nerfpp flag')
    assert (rows[:, 5] == 0).all() and set(samplers[0].random_sample(16)) >= {'depth_sup', 'depth_std'}
    ds = DeviceRaySamplers(samplers, dev(), seed=1)                                            # the device sampler reads the aligned prior
    np.testing.assert_array_equal(N(ds.depth_sup).reshape(len(samplers), -1), got['depth'].reshape(len(samplers), -1))
    # the trainer's own flags on the written scene: one log line with the totals, before the accumulation's when both are on
    argv = ['--basedir', str(tmp_path), '--datadir', str(tmp_path), '--scene', 'scene', '--cascade_samples', '16,16', '--use_depth',
            '--depth_sup_type', 'mono', '--lambda_depth', '0.1', '--world_size', '1', '--N_rand_override', '128', '--i_weights', '100',
            '--i_test', '100', '--i_print', '1', '--N_iters', '2', '--testskip', '1', '--expname', 'align', '--depth_align_anchor', 'lidar',
            '--depth_acc_views', '2']
    text = _run_nerfpp(argv)
    found = [l for l in text.splitlines() if l.startswith('depth ')]
    print(found)
    assert found[0] == DAL.totals_line(rows, 'lidar') and found[1].startswith('depth accumulation (2 views)') and len(found) == 2, text[-2000:]
    n_own = int(re.match(r'depth accumulation \(2 views\): \d+ frames, (\d+) own prior pixels', found[1]).group(1))
    assert n_own == (ref['depth_out'] > 0).sum()                                               # the accumulation saw the aligned prior
    assert len(re.findall(r'step: \d+ .*level_1/loss_depth: [-\d.e+]+ ', text)) == 2, text[-2000:]


def test_without_the_flags_the_library_is_never_loaded(DAL, colmap_scene, monkeypatch, tmp_path):
    """with the library unloaded and its path pointing nowhere, both trainers load their frames and step; with the flags they do not"""
    from outdoor_nerf_depth_amd import mip360_data as D
    from tests.test_gpu_depth_consistency import _one_mip360_step, _run_nerfpp, _nerfpp_argv
    monkeypatch.setattr(DAL, '_lib', None)
    monkeypatch.setattr(DAL, 'LIB_PATH', str(tmp_path / 'libdepthalign_hip.so'))
    base = ["Config.data_dir = '%s'" % colmap_scene[0], "Config.depth_sup_type = 'mono'", 'Config.sample_every = 1', 'Config.batch_size = 256']
    cfg = D.parse_gin(bindings=base)
    scene = D.Scene(cfg)
    _, sc = _one_mip360_step(scene, scene.device_frames('train', dev()), cfg)
    assert np.isfinite(sc).all()
    text = _run_nerfpp(_nerfpp_argv(tmp_path))
    assert 'depth alignment' not in text and len(re.findall(r'step: \d+ ', text)) == 2
    assert DAL._lib is None
    with pytest.raises(DAL.DepthAlignError, match='libdepthalign_hip.so not found'):
        D.Scene(D.parse_gin(bindings=base + ALIGN)).device_frames('train', dev())
    with pytest.raises(DAL.DepthAlignError, match='libdepthalign_hip.so not found'):
        _run_nerfpp(_nerfpp_argv(tmp_path, 'l1', ['--depth_align_anchor', 'gt']))
    assert DAL._lib is None

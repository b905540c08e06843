"""No GPU: what the command lines of the six depth-prior tools share (outdoor_nerf_depth_amd/depth_prior_io.py).  The
expected values are worked out from the definitions, not from the code: a PNG value is rint(metres x 256) -- numpy's rint, halves
to the even neighbour -- clamped to [2, 65535] under the mask and 0 off it."""
import os
from types import SimpleNamespace

import numpy as np
import pytest

from outdoor_nerf_depth_amd import data_loader_split
from outdoor_nerf_depth_amd import depth_prior_io as IO

# metres, and the value under the mask: 0 and what rounds to 1 are lifted to 2; 2.5 and 4.5 are ties that go down to the even 2
# and 4, 3.5 a tie that goes up to the even 4; 3.25 -> 3, 3.75 -> 4; 255.998 m = 65535.488 -> 65535; 256 m = 65536 and 1000 m clamp
METRES = np.array([0.0, 1.4 / 256, 2.5 / 256, 3.25 / 256, 3.5 / 256, 3.75 / 256, 4.5 / 256, 1.0, 255.998, 256.0, 1000.0, 10.0])
VALUES = np.array([2, 2, 2, 3, 4, 4, 4, 256, 65535, 65535, 65535, 2560], np.uint16)


def test_encode_metres_rounds_clamps_and_masks():
    mask = np.ones(len(METRES), bool)
    mask[-1] = False                                                                         # 10 m off the mask: 0, not 2560
    got = IO.encode_metres(METRES, mask)
    assert got.dtype == np.uint16
    np.testing.assert_array_equal(got, np.where(mask, VALUES, 0))
    np.testing.assert_array_equal(IO.encode_metres(METRES.astype(np.float32).reshape(3, 4), mask.reshape(3, 4)),
                                  IO.encode_metres(METRES.astype(np.float32).astype(np.float64), mask).reshape(3, 4))
    np.testing.assert_array_equal(IO.encode_metres(METRES, np.ones(len(METRES), bool)), VALUES)


def test_encode_metres_sanitised_takes_nan_and_inf():
    metres = np.concatenate([METRES, [np.nan, np.inf, np.nan]])
    mask = np.ones(len(metres), bool)
    mask[-1] = False
    with np.errstate(all='raise'):                                                           # and warns of nothing on the way
        got = IO.encode_metres(metres, mask, sanitise=True)
    np.testing.assert_array_equal(got, np.concatenate([VALUES, [2, 65535, 0]]).astype(np.uint16))   # NaN -> 0 m -> 2; +inf clamps
    finite = np.ones(len(METRES), bool)
    np.testing.assert_array_equal(IO.encode_metres(METRES, finite, sanitise=True), IO.encode_metres(METRES, finite))


def test_absrel_over_mask_and_positive_ground_truth():
    depth, gt = np.array([1.0, 2.0, 4.0], np.float32), np.array([2.0, 2.0, 0.0], np.float32)
    assert IO.absrel(depth, gt, np.ones(3, bool)) == 0.25                                    # (0.5 + 0) / 2: the third has no ground truth
    assert IO.absrel(depth, gt, np.array([True, False, True])) == 0.5
    assert np.isnan(IO.absrel(depth, gt, np.zeros(3, bool)))
    assert np.isnan(IO.absrel(depth, gt, np.array([False, False, True])))                    # masked in, but no ground truth there


def test_pick_layout_exits_by_message():
    args = lambda **kw: SimpleNamespace(**dict(dict(data_dir=None, datadir=None, scene=None), **kw))
    either = r'give either --data_dir \(COLMAP layout\) or --datadir with --scene \(NeRF\+\+ layout\)$'
    with pytest.raises(SystemExit, match=either):
        IO.pick_layout(args())
    with pytest.raises(SystemExit, match=either):
        IO.pick_layout(args(data_dir='a', datadir='b', scene='s'))
    with pytest.raises(SystemExit, match=r'--datadir with --scene and --points_model \(NeRF\+\+ layout\)$'):
        IO.pick_layout(args(), ' and --points_model')
    for scene in (None, ''):
        with pytest.raises(SystemExit, match='^--datadir needs --scene$'):
            IO.pick_layout(args(datadir='b', scene=scene))
    assert IO.pick_layout(args(data_dir='a')) == 'colmap' and IO.pick_layout(args(datadir='b', scene='s')) == 'nerfpp'
    assert IO.pick_layout(args(data_dir='a', scene='ignored')) == 'colmap'


def test_colmap_suffix():
    assert [IO.colmap_suffix({'factor': f}) for f in (0, 4, '8')] == ['', '_4', '_8']


def test_write_rows_report_frames_then_total(tmp_path):
    path = str(tmp_path / 'report.txt')
    rows = np.array([[3, 1, 2, 0], [5, 0, 4, 1]])
    IO.write_rows_report(path, ['a.png', 'b.png'], rows, 'n_one n_two n_three n_four')
    assert open(path).read() == '# frame n_one n_two n_three n_four\na.png 3 1 2 0\nb.png 5 0 4 1\ntotal 8 1 6 1\n'
    depth, gt = np.array([[1.0, 3.0], [2.0, 2.0]]), np.array([[2.0, 2.0], [4.0, 0.0]])      # absrel 0.5 and 0.5 | 0.5 | all three 0.5
    seen = []

    def tail(sel, r, n):
        seen.append((sel, r.tolist(), n))
        return ' %.6f %.6f' % (r[0] / (10 * n), IO.absrel(depth[sel], gt[sel], depth[sel] > 0))
    IO.write_rows_report(path, ['a.png', 'b.png'], rows.tolist(), 'n_one n_two n_three n_four coverage absrel', tail)
    assert open(path).read() == ('# frame n_one n_two n_three n_four coverage absrel\na.png 3 1 2 0 0.300000 0.500000\n'
                                 'b.png 5 0 4 1 0.500000 0.500000\ntotal 8 1 6 1 0.400000 0.500000\n')
    assert seen == [(0, [3, 1, 2, 0], 1), (1, [5, 0, 4, 1], 1), (slice(None), [8, 1, 6, 1], 2)]


def test_nerfpp_splits_skips_an_empty_split_and_loads_the_other(tmp_path, monkeypatch, capsys):
    root = str(tmp_path) + '/'                                                               # a trailing slash, as a shell completes it
    os.makedirs(os.path.join(root, 'scene', 'train', 'depth_lidar'))                         # train: the folder, nothing in it
    test_dir = os.path.join(str(tmp_path), 'scene', 'test', 'depth_lidar')
    os.makedirs(test_dir)
    for name in ('b.png', 'a.jpg', 'c.txt'):
        open(os.path.join(test_dir, name), 'w').close()
    calls = []

    def load(basedir, scene, split, **kw):
        calls.append((basedir, scene, split, kw))
        return ['sampler of ' + split]
    monkeypatch.setattr(data_loader_split, 'load_data_split', load)
    args = SimpleNamespace(datadir=root, scene='scene')
    got = list(IO.nerfpp_splits(args, 'depth_lidar', ['*.png', '*.jpg'], depth_sup_type='lidar'))
    split_dir = os.path.join(str(tmp_path), 'scene', 'test')
    assert got == [('test', split_dir, [os.path.join(test_dir, 'a.jpg'), os.path.join(test_dir, 'b.png')], ['sampler of test'])]
    assert calls == [(root, 'scene', 'test', {'depth_sup_type': 'lidar'})]                   # the empty split is not loaded
    assert capsys.readouterr().out == 'train: no prior in %s\n' % os.path.join(str(tmp_path), 'scene', 'train', 'depth_lidar')
    assert IO.png_names(got[0][2]) == ['a.png', 'b.png']
    assert list(IO.nerfpp_splits(SimpleNamespace(datadir=root, scene='nowhere'), 'pose', ['*.txt'], '{split}: no frames in {split_dir}')) == []
    assert capsys.readouterr().out == ''.join('%s: no frames in %s\n' % (s, os.path.join(str(tmp_path), 'nowhere', s)) for s in ('train', 'test'))


def test_stack_frames_one_size_or_the_callers_error():
    class Refused(RuntimeError):
        pass
    s = lambda H, W, v: SimpleNamespace(H=H, W=W, depth_sup=np.full(H * W, v, np.float64), depth_gt=np.full(H * W, v + 1, np.float32))
    frames = IO.stack_frames([s(2, 3, 1.5), s(2, 3, 2.5)], 'depth_sup', 'unused', Refused)
    assert frames.dtype == np.float32 and frames.shape == (2, 2, 3) and frames[1, 1, 2] == 2.5
    with pytest.raises(Refused, match='^the frames differ$'):
        IO.stack_frames([s(2, 3, 1.0), s(3, 2, 1.0)], 'depth_sup', 'the frames differ', Refused)
    gt = IO.stack_gt([s(2, 3, 1.0), s(2, 3, 2.0)])
    assert gt.shape == (2, 2, 3) and gt[1, 0, 0] == 3.0
    one_without = s(2, 3, 2.0)
    one_without.depth_gt = None
    assert IO.stack_gt([s(2, 3, 1.0), one_without]) is None


def test_stack_priors_refuses_a_missing_prior_and_differing_sizes_in_the_stages_words():
    class Refused(RuntimeError):
        pass
    s = lambda H, W, v: SimpleNamespace(H=H, W=W, depth_sup=None if v is None else np.full(H * W, v, np.float32))
    assert IO.stack_priors([s(2, 3, 1.0), s(2, 3, 2.0)], '--depth_acc_views', 'accumulate', 'accumulation', Refused).shape == (2, 2, 3)
    with pytest.raises(Refused, match='^--depth_acc_views: the training frames carry no depth prior to accumulate$'):
        IO.stack_priors([s(2, 3, 1.0), s(2, 3, None)], '--depth_acc_views', 'accumulate', 'accumulation', Refused)
    with pytest.raises(Refused, match='^--depth_cons_views: the frames differ in size; the check takes frames of one size$'):
        IO.stack_priors([s(2, 3, 1.0), s(3, 2, 1.0)], '--depth_cons_views', 'check', 'check', Refused)


def test_write_back_fills_the_std_where_there_is_none_or_replaces_it():
    s = lambda std: SimpleNamespace(depth_sup=np.zeros(6, np.float32), depth_std=std)
    kept = np.full(6, 9.0, np.float32)
    depth, std = np.arange(12, dtype=np.float32).reshape(2, 2, 3), np.arange(12, dtype=np.float32).reshape(2, 2, 3) + 100
    a, b = s(None), s(kept)
    IO.write_back([a, b], depth)                                                  # no std given: depth_sup alone
    assert a.depth_sup.shape == (6,) and a.depth_sup[5] == 5 and b.depth_sup[0] == 6 and a.depth_std is None and b.depth_std is kept
    IO.write_back([a, b], depth, std)                                             # where a sampler carries none
    assert a.depth_std.shape == (6,) and a.depth_std[0] == 100 and b.depth_std is kept
    IO.write_back([a, b], depth, std, replace_std=True)                           # always
    assert b.depth_std[0] == 106 and a.depth_std[5] == 105

"""GPU: --depth_vis of the three evaluators end to end on the small synthetic scenes of the other CLI tests.  The new files exist,
have the frame's size and equal tests/depth_vis_reference.py applied to the tensors the same run handed to the library (recorded
at depth_vis's entry points) and to the TIFFs it wrote; without the flag a folder's listing is unchanged; eval_images
--depth_vis reproduces the mean and median pictures byte for byte from the folder alone."""
import os

import numpy as np
import pytest
import torch

from tests import depth_vis_reference as R
from tests.test_gpu_depth_vis import check_picture, order_gate
from tests.test_gpu_mip360_app import _run, dev
from tests.test_mip360_scene import write_scene

pytestmark = pytest.mark.gpu

SUITE = ('depth_mean', 'depth_median', 'depth_triplet', 'color_matte', 'coords_mod')


def _png(path):
    from PIL import Image
    return np.asarray(Image.open(str(path)))


def _tiff(path):
    from PIL import Image
    return np.asarray(Image.open(str(path)))


def _record(monkeypatch, module, name, store):
    real = getattr(module, name)

    def wrapper(*args, **kw):
        store.append([a.detach().cpu().numpy() for a in args if torch.is_tensor(a)])
        return real(*args, **kw)
    monkeypatch.setattr(module, name, wrapper)


def test_mip360_eval_depth_vis(tmp_path, monkeypatch):
    dev()
    from outdoor_nerf_depth_amd import depth_vis as DV, eval_images, mip360_eval
    H, W = 32, 40
    data, ckpt = tmp_path / 'scene', tmp_path / 'run'
    write_scene(str(data), n_frames=20, H=H, W=W)                                      # test frames: indices 9 and 19
    gin = tmp_path / '360.gin'
    gin.write_text("Config.dataset_loader = 'llff'\nConfig.near = 0.2\nConfig.far = 1e6\nConfig.batch_size = 4096\n"
                   'Config.compute_disp_metrics = True\nConfig.auto_adjust_near_far = True\n\n'
                   'Model.raydist_fn = @jnp.reciprocal\nModel.opaque_background = True\n'
                   'PropMLP.warp_fn = @coord.contract\nPropMLP.net_depth = 4\nPropMLP.net_width = 256\n'
                   'NerfMLP.warp_fn = @coord.contract\nNerfMLP.net_depth = 8\nNerfMLP.net_width = 1024\n')
    b = ["Config.data_dir = '%s'" % data, "Config.checkpoint_dir = '%s'" % ckpt, 'Config.max_steps = 12',
         'Config.checkpoint_every = 12', 'Config.print_every = 12', 'Config.batch_size = 1024', 'Config.lr_delay_steps = 0',
         "Config.depth_sup_type = 'mono_crop'", 'Config.render_chunk_size = 1024', 'Config.sample_every = 1',
         'Config.compute_disp_metrics = True', "Config.depth_loss_type = 'mse'"]
    bind = lambda extra: sum([['--gin_bindings', x] for x in b + list(extra)], [])
    _run('mip360_train', ['--gin_configs', str(gin)] + bind([]))
    mip360_eval.main(['--gin_configs', str(gin)] + bind(["Config.eval_suffix = 'plain'"]))
    plain = sorted(os.listdir(str(ckpt / 'test_eval_preds_plain')))
    assert not [f for f in plain if f.startswith('vis_')]
    calls = []
    _record(monkeypatch, DV, 'mip360_suite_async', calls)
    mip360_eval.main(['--gin_configs', str(gin), '--depth_vis'] + bind(["Config.eval_suffix = 'vis'"]))
    d = ckpt / 'test_eval_preds_vis'
    new = {'vis_%s_%03d.png' % (k, i) for k in SUITE for i in (0, 1)}
    assert sorted(os.listdir(str(d))) == sorted(set(plain) | new)                     # the flag adds these and nothing else
    assert len(calls) == 1                                                            # one call for the split
    rgb, acc, dmean, dmedian, p5, p95, org, dirs = calls[0]
    assert rgb.shape == (2, H, W, 3) and org.shape == (2, H, W, 3) and acc.shape == (2, H, W)
    for i in (0, 1):
        np.testing.assert_array_equal(np.nan_to_num(dmean[i]), _tiff(d / ('distance_mean_%03d.tiff' % i)))
        np.testing.assert_array_equal(np.nan_to_num(dmedian[i]), _tiff(d / ('distance_median_%03d.tiff' % i)))
        np.testing.assert_array_equal(np.nan_to_num(acc[i]), _tiff(d / ('acc_%03d.tiff' % i)))
        ref = R.mip360_suite(rgb[i], acc[i], dmean[i], dmedian[i], p5[i], p95[i], org[i], dirs[i])
        for k in SUITE:
            got = _png(d / ('vis_%s_%03d.png' % (k, i)))
            assert got.shape == (H, W, 3)
            check_picture(got, ref[k][0], ref[k][1], '%s frame %d' % (k, i))
    # the percentile bounds of the same tensors, under the gate of another summation order
    got = DV.mip360_suite_async(*[torch.from_numpy(a).cuda() for a in calls[0]]).get()
    for i in (0, 1):
        a = R.effective_acc(acc[i], dmean[i])
        trip = R.triplet_value(dmedian[i], p5[i], p95[i])
        for k, v, w in (('mean', dmean[i], a), ('median', dmedian[i], a), ('triplet', trip, np.repeat(a[..., None], 3, -1))):
            ref, gate = order_gate(v, w, R.SUITE_PS)
            err = np.abs(got['lohi_' + k][i] - ref)
            print('frame %d %s: dev %s ref %s err %s gate %s' % (i, k, got['lohi_' + k][i], ref, err, gate))
            assert np.all(err <= gate), (k, err, gate)
    # eval_images --depth_vis: the same two pictures from the folder's TIFFs alone
    keep = {f: (d / f).read_bytes() for f in new if 'depth_mean' in f or 'depth_median' in f}
    for f in keep:
        os.remove(str(d / f))
    eval_images.main(['--pred_dir', str(d), '--method', 'mipnerf360', '--depth_vis'])
    assert sorted(os.listdir(str(d))) == sorted(set(plain) | new)
    for f, data_ in keep.items():
        assert (d / f).read_bytes() == data_, f


def test_ddp_test_nerf_depth_vis(tmp_path, monkeypatch):
    dev()
    from outdoor_nerf_depth_amd import ddp_train_nerf as T
    from outdoor_nerf_depth_amd import ddp_test_nerf as TT
    from outdoor_nerf_depth_amd import depth_vis as DV, eval_images
    H, W = 24, 32
    base = ['--expname', 'run', '--basedir', str(tmp_path), '--synthetic', '--synthetic_hw', '%d,%d' % (H, W),
            '--synthetic_frames', '20', '--cascade_samples', '64,128', '--use_depth', '--depth_loss_type', 'mse',
            '--depth_sup_type', 'mono_crop', '--lambda_depth', '0.1', '--sample_every', '2', '--world_size', '1',
            '--N_rand_override', '256', '--i_weights', '5', '--i_test', '5', '--testskip', '1', '--i_print', '1']
    calls = []
    _record(monkeypatch, DV, 'minmax_colorize_async', calls)
    args = T.config_parser().parse_args(base + ['--N_iters', '6', '--depth_vis'])
    T.validate_args(args)
    args.world_size = 1
    T.ddp_train_nerf(0, args)                                                         # the in-loop test render, through write_eval_images
    rdir = tmp_path / 'run' / 'render_test_000005'
    today = {pre + '%06d.png' % i for i in (0, 1) for pre in ('', 'fg_', 'bg_', 'depth_', 'error_rgb_', 'absrel_')}
    today |= {'psnr_000005.txt', 'rmse_000005.txt', 'absrel_000005.txt'}
    new = {pre + '%06d.png' % i for i in (0, 1) for pre in ('fg_depth_', 'bg_depth_')} | {'depth_range_000005.txt'}

    def check_folder(what):
        assert set(os.listdir(str(rdir))) == today | new, what
        assert len(calls) == 1, what                                                  # one call for the split
        x = calls.pop()[0]
        assert x.shape == (4, H, W)                                                   # fg of both frames, then bg
        rows = [[float(v) for v in line.split()] for line in (rdir / 'depth_range_000005.txt').read_text().splitlines()]
        assert len(rows) == 2
        for i in (0, 1):
            for j, pre in ((i, 'fg_depth_'), (2 + i, 'bg_depth_')):
                b, fr, (vmin, vmax) = R.colorize_minmax(x[j])
                got = _png(rdir / (pre + '%06d.png' % i))
                assert got.shape == (H, W, 3)
                check_picture(got, b, fr, '%s %s %d' % (what, pre, i))
                assert rows[i][2 * (j // 2):2 * (j // 2) + 2] == [vmin, vmax]

    check_folder('in-loop')
    for f in os.listdir(str(rdir)):
        os.remove(str(rdir / f))
    targs = T.config_parser().parse_args(base + ['--render_splits', 'test'])          # without the flag: exactly today's files
    targs.world_size = 1
    TT.ddp_test_nerf(0, targs)
    assert set(os.listdir(str(rdir))) == today and not calls
    targs = T.config_parser().parse_args(base + ['--render_splits', 'test', '--depth_vis'])
    targs.world_size = 1
    TT.ddp_test_nerf(0, targs)
    check_folder('ddp_test_nerf')
    # eval_images --depth_vis on a NeRF++ folder: depth_*.png -> vis_depth_*.png, min-max jet
    eval_images.main(['--pred_dir', str(rdir), '--method', 'nerfpp', '--depth_vis'])
    assert set(os.listdir(str(rdir))) == today | new | {'vis_depth_%06d.png' % i for i in (0, 1)}
    for i in (0, 1):
        b, fr, _ = R.colorize_minmax(_png(rdir / ('depth_%06d.png' % i)).astype(np.float32))
        check_picture(_png(rdir / ('vis_depth_%06d.png' % i)), b, fr, 'eval_images nerfpp %d' % i)

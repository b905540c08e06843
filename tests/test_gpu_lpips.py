"""GPU: liblpips_hip.so (LPIPS v0.1 on VGG-16 features from user-supplied weights, include/lpips_hip.h) against the float64
torch-CPU statement in tests/lpips_reference.py, one layer at a time and end to end, its bit-reproducibility, and the
--lpips_weights flag of ddp_test_nerf, mip360_eval and eval_images.  Weights are random, seeded and made here.

Gates (derived, not measured): the paper's tables print three decimals, so an error below 5e-4 cannot move a printed digit
except at a tie; a tenth of that: |total - float64 reference| <= 5e-5, and each of the five contributions within 1e-5 (they
add up to the total).  tests/test_lpips.py asserts that the reference totals of the strongly differing pairs lie in
[0.05, 1.5], so the absolute gate means something; the pairs whose total is below that range (pred = gt is 0 by definition,
sigma-2 noise gives 1e-4 .. 2e-2: the set spans four decades, which no single scale of the lin weights brings into one
range) are also held to the relative error the absolute gate asks at the bottom of the range, 5e-5 / 0.05 = 1e-3.  A single layer (float32 MFMA: the same arithmetic class as a float32 CPU convolution, another
summation order) is held to 4x the error the float32 torch-CPU convolution shows against float64 on the same input.
Every figure is printed before it is asserted; profiles/r09_lpips_error.json records a run.
"""
import ctypes as C
import glob
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import lpips_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu
TOL_TOTAL, TOL_TAP = 5e-5, 1e-5
REL_BELOW_RANGE = TOL_TOTAL / R.RANGE[0]          # 1e-3: what the absolute gate asks at the bottom of the range
_cache = {}


def dev():
    if not torch.cuda.is_available():
        pytest.skip('needs a GPU')
    return torch.device('cuda:0')


def weights():
    """(reference dict, lpips.Weights) of the seeded random weights, once per session"""
    if 'w' not in _cache:
        from outdoor_nerf_depth_amd.lpips import Weights
        ref = R.random_weights(R.WEIGHT_SEED, R.LIN_SCALE)
        _cache['w'] = (ref, Weights(ref))
    return _cache['w']


def gpu_lpips(gts, preds):
    from outdoor_nerf_depth_amd.lpips import lpips_u8
    d = dev()
    up = lambda a: torch.from_numpy(np.ascontiguousarray(np.stack(a))).to(d)
    return lpips_u8(up(gts), up(preds), weights()[1])


def _check_pairs(pairs):
    """gate every pair against float64; returns (worst kernel error, worst float32-CPU error) of total and taps"""
    ref_w = weights()[0]
    got_t, got_p = gpu_lpips([g for _, g, _ in pairs], [p for _, _, p in pairs])
    worst = {'kernel_total': 0.0, 'kernel_tap': 0.0, 'cpu32_total': 0.0, 'cpu32_tap': 0.0}
    fails = []
    for i, (label, g, p) in enumerate(pairs):
        want_t, want_p = R.lpips(g, p, ref_w, torch.float64)
        f32_t, f32_p = R.lpips(g, p, ref_w, torch.float32)
        et, ep = abs(got_t[i] - want_t[0]), np.abs(got_p[i] - want_p[0]).max()
        ct, cp = abs(f32_t[0] - want_t[0]), np.abs(f32_p[0] - want_p[0]).max()
        print('%-28s ref64 %.9f gpu %.9f | err total %.3g tap %.3g | float32 CPU err total %.3g tap %.3g'
              % (label, want_t[0], got_t[i], et, ep, ct, cp))
        worst['kernel_total'] = max(worst['kernel_total'], et)
        worst['kernel_tap'] = max(worst['kernel_tap'], ep)
        worst['cpu32_total'] = max(worst['cpu32_total'], ct)
        worst['cpu32_tap'] = max(worst['cpu32_tap'], cp)
        if not (et <= TOL_TOTAL and ep <= TOL_TAP):
            fails.append(label)
        if 0 < want_t[0] < R.RANGE[0] and not et <= REL_BELOW_RANGE * want_t[0]:    # below the range: the same strictness, relative
            fails.append(label + ' (relative)')
        if label.split('/')[1] == 'same':
            assert got_t[i] == 0.0 and (got_p[i] == 0.0).all(), label
        assert got_t[i] == got_p[i].sum() or abs(got_t[i] - got_p[i].sum()) <= 1e-15
    print('worst', worst)
    assert not fails, fails
    return worst


@pytest.mark.parametrize('hw', [(16, 16), (17, 31), (64, 96)])
def test_accuracy_small(hw):
    dev()
    _check_pairs(R.gated_pairs(hw[0], hw[1], full=True))


def test_accuracy_187x621():
    dev()
    _check_pairs(R.gated_pairs(187, 621, full=False))


def test_accuracy_375x1242_one_pair():
    dev()
    g, p = R.make_pair('smooth', 'noise25', 375, 1242, 77)
    _check_pairs([('smooth/noise25/375x1242', g, p)])


@pytest.mark.parametrize('cin,cout', sorted(set(R.CONV_SHAPES)))
def test_single_layer_against_float64(cin, cout):
    """lpips_conv3x3_relu on an odd-sized map: max |error| <= 4x that of the float32 torch-CPU convolution"""
    d = dev()
    from outdoor_nerf_depth_amd import lpips as P
    rs = np.random.RandomState(cin * 1000 + cout)
    n, H, W = 2, 13, 19
    x = np.maximum(rs.standard_normal((n, H, W, cin)), 0).astype(np.float32) if cin > 3 else rs.standard_normal((n, H, W, cin)).astype(np.float32)
    w = (rs.standard_normal((cout, cin, 3, 3)) * np.sqrt(2.0 / (9 * cin))).astype(np.float32)
    b = (0.05 * rs.standard_normal(cout)).astype(np.float32)
    want = R.conv3x3_relu_nhwc(x, w, b, torch.float64)
    cpu32 = R.conv3x3_relu_nhwc(x, w, b, torch.float32).astype(np.float64)
    L = P.lib()
    xd, wd, bd = (torch.from_numpy(a).to(d) for a in (x, w, b))
    wp = torch.empty(L.lpips_packed_conv_floats(cin, cout), dtype=torch.float32, device=d)
    y = torch.full((n, H, W, cout), float('nan'), dtype=torch.float32, device=d)
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    P.check(L.lpips_pack_conv(st, cin, cout, wd.data_ptr(), wp.data_ptr()), 'lpips_pack_conv')
    P.check(L.lpips_conv3x3_relu(st, n, H, W, cin, cout, xd.data_ptr(), wp.data_ptr(), bd.data_ptr(), y.data_ptr()), 'lpips_conv3x3_relu')
    got = y.cpu().numpy().astype(np.float64)
    e_gpu, e_cpu = np.abs(got - want).max(), np.abs(cpu32 - want).max()
    print('conv %d -> %d: max|y| %.3g  gpu err %.3g  float32 CPU err %.3g  ratio %.2f' % (cin, cout, np.abs(want).max(), e_gpu, e_cpu,
                                                                                        e_gpu / e_cpu))
    assert np.isfinite(got).all()
    assert e_gpu <= 4 * e_cpu


def test_bit_reproducible_and_batch_independent():
    dev()
    pairs = [R.make_pair(c, k, 37, 53, 5 + i) for i, (c, k) in enumerate(
        [('noise', 'noise2'), ('smooth', 'noise25'), ('flat', 'unrelated'), ('saturated', 'same'), ('noise', 'unrelated')])]
    gts, preds = [g for g, _ in pairs], [p for _, p in pairs]
    t1, p1 = gpu_lpips(gts, preds)
    t2, p2 = gpu_lpips(gts, preds)
    assert t1.tobytes() == t2.tobytes() and p1.tobytes() == p2.tobytes()            # call to call
    for i in range(5):                                                              # a batch of 5 against five single calls
        ts, ps = gpu_lpips(gts[i:i + 1], preds[i:i + 1])
        assert ts.tobytes() == t1[i:i + 1].tobytes() and ps.tobytes() == p1[i:i + 1].tobytes(), i
    assert t1[3] == 0.0 and (p1[3] == 0.0).all()                                    # identical images: exactly zero
    assert (t1[[0, 1, 2, 4]] > 0).all()


def test_border_ring_is_seen():
    """a pair that differs only in the outermost pixel ring scores non-zero, on every side"""
    dev()
    g = R.content('smooth', 33, 47, np.random.RandomState(3))
    for name, sl in (('top', np.s_[0, :]), ('bottom', np.s_[-1, :]), ('left', np.s_[:, 0]), ('right', np.s_[:, -1])):
        p = g.copy()
        p[sl] = 255 - p[sl]
        t, per = gpu_lpips([g], [p])
        want = R.lpips(g, p, weights()[0])[0][0]
        print(name, t[0], want)
        assert t[0] > 0 and abs(t[0] - want) <= TOL_TOTAL


# ---- the flag, end to end
def _read_metric(path):
    with open(str(path)) as f:
        return [float(x) for x in f.read().split()]


def _png(path):
    from PIL import Image
    return np.array(Image.open(str(path)))


def _weights_file(tmp_path):
    path = str(tmp_path / 'lpips_weights.npz')
    np.savez(path, **weights()[0])
    return path


def test_ddp_test_nerf_lpips_flag(tmp_path):
    dev()
    from outdoor_nerf_depth_amd import ddp_train_nerf as T
    from outdoor_nerf_depth_amd import ddp_test_nerf as TT
    from outdoor_nerf_depth_amd.data_loader_split import synthetic_ray_samplers
    from outdoor_nerf_depth_amd.image_metrics import to_bytes_nearest
    wfile = _weights_file(tmp_path)
    base = ['--expname', 'run', '--basedir', str(tmp_path), '--synthetic', '--synthetic_hw', '24,32',
            '--synthetic_frames', '20', '--cascade_samples', '64,128', '--use_depth', '--depth_loss_type', 'mse',
            '--depth_sup_type', 'mono_crop', '--lambda_depth', '0.1', '--sample_every', '2', '--world_size', '1',
            '--N_rand_override', '256', '--i_weights', '5', '--i_test', '5', '--testskip', '1', '--i_print', '1']
    args = T.config_parser().parse_args(base + ['--N_iters', '6', '--lpips_weights', wfile])
    T.validate_args(args)
    args.world_size = 1
    T.ddp_train_nerf(0, args)                                                     # the in-loop test render: the flag alone
    rdir = tmp_path / 'run' / 'render_test_000005'
    today = {pre + '%06d.png' % i for i in (0, 1) for pre in ('', 'fg_', 'bg_', 'depth_', 'error_rgb_', 'absrel_')}
    today |= {'psnr_000005.txt', 'rmse_000005.txt', 'absrel_000005.txt'}
    assert set(os.listdir(str(rdir))) == today | {'lpips_000005.txt'}
    gt = np.stack([to_bytes_nearest(s.get_img()) for s in synthetic_ray_samplers('test', 1, 'mono_crop', 20, 24, 32)])

    def check_folder(what):
        pred = np.stack([_png(rdir / ('%06d.png' % i)) for i in (0, 1)])
        want = R.lpips(gt, pred, weights()[0])[0]
        got = _read_metric(rdir / 'lpips_000005.txt')
        print(what, got, list(want))
        assert len(got) == 3 and got[2] == float(np.mean(got[:2]))                # per image, then the mean
        assert np.abs(np.array(got[:2]) - want).max() <= TOL_TOTAL and want.min() > 0

    check_folder('in-loop')
    for f in os.listdir(str(rdir)):
        os.remove(str(rdir / f))
    targs = T.config_parser().parse_args(base + ['--render_splits', 'test'])      # without the flags: exactly today's files
    targs.world_size = 1
    TT.ddp_test_nerf(0, targs)
    assert set(os.listdir(str(rdir))) == today
    targs = T.config_parser().parse_args(base + ['--render_splits', 'test', '--image_metrics', '--lpips_weights', wfile])
    targs.world_size = 1
    TT.ddp_test_nerf(0, targs)
    assert set(os.listdir(str(rdir))) == today | {'ssim_000005.txt', 'psnr8_000005.txt', 'lpips_000005.txt'}
    check_folder('ddp_test_nerf')


def _run(mod, args, timeout=900):
    env = dict(os.environ)
    env['PYTHONPATH'] = ROOT + os.pathsep + env.get('PYTHONPATH', '')
    p = subprocess.run([sys.executable, '-m', 'outdoor_nerf_depth_amd.' + mod] + args, cwd=ROOT, env=env, capture_output=True,
                       text=True, timeout=timeout)
    assert p.returncode == 0, p.stdout[-3000:] + p.stderr[-3000:]
    return p.stdout


def test_mip360_eval_and_eval_images_lpips_flag(tmp_path):
    dev()
    from tests.test_mip360_scene import write_scene
    wfile = _weights_file(tmp_path)
    data, ckpt = tmp_path / 'scene', tmp_path / 'run'
    write_scene(str(data), n_frames=12, H=32, W=40)
    bind = lambda extra=(): sum([['--gin_bindings', x] for x in [
        "Config.data_dir = '%s'" % data, "Config.checkpoint_dir = '%s'" % ckpt, 'Config.max_steps = 4', 'Config.checkpoint_every = 4',
        'Config.print_every = 4', 'Config.batch_size = 1024', 'Config.lr_delay_steps = 0', "Config.depth_sup_type = 'mono_crop'",
        'Config.render_chunk_size = 1024', 'Config.sample_every = 1', 'Config.compute_disp_metrics = True',
        "Config.depth_loss_type = 'mse'"] + list(extra)], [])
    _run('mip360_train', bind() + ['--lpips_weights', wfile])
    gt = np.stack([_png(sorted(glob.glob(str(data / 'images' / '*.png')))[9])])      # the one test frame: index 9
    in_loop = ckpt / 'test_preds_4'
    want = R.lpips(gt, np.stack([_png(in_loop / 'color_000.png')]), weights()[0])[0]
    got = _read_metric(in_loop / 'metric_lpips_4.txt')
    print('in-loop', got, want)
    assert len(got) == 2 and abs(got[0] - want[0]) <= TOL_TOTAL
    assert not [f for f in os.listdir(str(in_loop)) if 'ssim' in f or 'psnr8' in f]   # the flag alone writes only the LPIPS file
    _run('mip360_eval', bind(["Config.eval_suffix = 'plain'"]))
    plain = set(os.listdir(str(ckpt / 'test_eval_preds_plain')))
    assert 'metric_psnr_4.txt' in plain and not [f for f in plain if 'lpips' in f or 'ssim' in f]
    _run('mip360_eval', bind(["Config.eval_suffix = 'lp'"]) + ['--lpips_weights', wfile])
    d = ckpt / 'test_eval_preds_lp'
    assert set(os.listdir(str(d))) == plain | {'metric_lpips_4.txt'}
    want = R.lpips(gt, np.stack([_png(d / 'color_000.png')]), weights()[0])[0]
    got = _read_metric(d / 'metric_lpips_4.txt')
    print('mip360_eval', got, want)
    assert len(got) == 2 and abs(got[0] - want[0]) <= TOL_TOTAL and want[0] > 0
    # the folder scored the way the reference's utils/eval.py scores it gives the same numbers
    ev = ['--gt_dir', str(data / 'images'), '--pred_dir', str(d), '--method', 'mipnerf360', '--split', '1']
    out = _run('eval_images', ev + ['--lpips_weights', wfile])
    assert 'eval_lpips.txt is not written' not in out
    assert _read_metric(d / 'eval_lpips.txt') == got
    os.remove(str(d / 'eval_lpips.txt'))
    out = _run('eval_images', ev)                                                 # without the flag: as before
    assert 'eval_lpips.txt is not written' in out and not (d / 'eval_lpips.txt').exists()

"""GPU: the N > 1 path of the trainer on ONE GPU -- two ranks share cuda:0 and all-reduce with gloo
(the 8-GPU RCCL run is the driver's; this pins the semantics): every rank ends each step with
bit-identical parameters, equal to a single process that averages the two ranks' gradients itself
(DDP semantics of nerf-methods/nerfplusplus/ddp_train_nerf.py:323)."""
import os
import socket

import numpy as np
import pytest

torch = pytest.importorskip('torch')
pytestmark = pytest.mark.gpu


def _free_port():
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _batches(rank, n=64):
    from outdoor_nerf_depth_amd.synthetic import SyntheticKitti
    scene = SyntheticKitti(depth_sup_type='gt')
    rng = np.random.RandomState((rank + 1) * 777)                       # per-rank seeds, :406-408
    out = []
    for _ in range(2):
        b = scene.random_batch(n, rng)
        b['depth_sup'][:8] = np.float32(0.05)
        uni = dict(t_fg=rng.rand(n, 64).astype(np.float32), t_bg=rng.rand(n, 64).astype(np.float32),
                   u_fg=rng.rand(n, 128).astype(np.float32), u_bg=rng.rand(n, 128).astype(np.float32))
        out.append((b, uni))
    return out


def _to_dev(d, dev):
    return {k: torch.from_numpy(np.ascontiguousarray(v)).to(dev) for k, v in d.items() if isinstance(v, np.ndarray)}


def _worker(rank, world, port, out_dir, overlap):
    import torch.distributed as dist
    from outdoor_nerf_depth_amd.trainer import NerfppTrainer
    os.environ['MASTER_ADDR'] = '127.0.0.1'
    os.environ['MASTER_PORT'] = str(port)
    dist.init_process_group('gloo', rank=rank, world_size=world)
    dev = torch.device('cuda:0')
    torch.cuda.set_device(dev)
    tr = NerfppTrainer(dev, precision=2, use_depth=True, depth_loss_type='mse', lambda_depth=0.1, world_size=world,
                       overlap_allreduce=overlap)
    for b, uni in _batches(rank):
        tr.train_step(_to_dev(b, dev), uniforms=_to_dev(uni, dev))
    tr.flush()
    torch.cuda.synchronize()
    np.save(os.path.join(out_dir, 'params_rank%d.npy' % rank),
            np.stack([e.params.cpu().numpy() for e in tr.engines]))
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.parametrize('overlap', [True, False])
def test_two_ranks_share_one_gpu(tmp_path, overlap):
    if not torch.cuda.is_available():
        pytest.skip('needs a GPU')
    import torch.multiprocessing as mp
    mp.spawn(_worker, args=(2, _free_port(), str(tmp_path), overlap), nprocs=2, join=True)
    p0 = np.load(tmp_path / 'params_rank0.npy')
    p1 = np.load(tmp_path / 'params_rank1.npy')
    np.testing.assert_array_equal(p0, p1)                 # identical update on every rank

    # single process: gradients of both ranks' batches averaged by hand, same Adam
    from outdoor_nerf_depth_amd import ops
    from outdoor_nerf_depth_amd.trainer import NerfppTrainer
    dev = torch.device('cuda:0')
    tr = NerfppTrainer(dev, precision=2, use_depth=True, depth_loss_type='mse', lambda_depth=0.1, world_size=1)
    b0, b1 = _batches(0), _batches(1)
    for step in range(2):
        tr.step_count += 1
        grads = [torch.zeros_like(e.params) for e in tr.engines]
        for b, uni in (b0[step], b1[step]):
            bd, ud = _to_dev(b, dev), _to_dev(uni, dev)
            far, fg_z, bg_z = ops.sample_coarse(bd['ray_o'], bd['ray_d'], bd['min_depth'], 64, ud['t_fg'], ud['t_bg'])
            ret = None
            for m, eng in enumerate(tr.engines):
                if m == 1:
                    fg_z = ops.sample_fine(fg_z, ret['fg_weights'], 128, u=ud['u_fg'])
                    bg_z = ops.sample_fine(bg_z, ret['bg_weights'], 128, u=ud['u_bg'])
                ret = eng.forward(bd['ray_o'], bd['ray_d'], far, fg_z, bg_z, training=True)
                sc, g_rgb, g_depth, g_w = ops.loss_and_grads(ret, bd['rgb'], bd['depth_sup'], 'mse', 0.1)
                grads[m] += eng.backward(g_rgb, g_depth, g_w, grad_scale=0.5)
        for m, eng in enumerate(tr.engines):
            ops.adam_step(eng.params, grads[m], tr.exp_avg[m], tr.exp_avg_sq[m], tr.step_count, lr=tr.lrate)
            eng.repack()
    ref = np.stack([e.params.cpu().numpy() for e in tr.engines])
    np.testing.assert_array_equal(p0, ref)


def _worker_ae(rank, world, port, out_dir):
    import torch.distributed as dist
    from outdoor_nerf_depth_amd.trainer import NerfppTrainer
    os.environ['MASTER_ADDR'] = '127.0.0.1'
    os.environ['MASTER_PORT'] = str(port)
    dist.init_process_group('gloo', rank=rank, world_size=world)
    dev = torch.device('cuda:0')
    torch.cuda.set_device(dev)
    names = ['s/train/rgb/%06d.png' % i for i in range(4)]
    tr = NerfppTrainer(dev, precision=2, use_depth=True, depth_loss_type='mse', lambda_depth=0.1, world_size=world,
                       optim_autoexpo=True, img_names=names, lambda_autoexpo=0.5)
    for step, (b, uni) in enumerate(_batches(rank)):
        bd = _to_dev(b, dev)
        bd['img_name'] = names[(rank + 2 * step) % 4]          # step 0: images 0 / 1, step 1: images 2 / 3
        tr.train_step(bd, uniforms=_to_dev(uni, dev))
    tr.flush()
    torch.cuda.synchronize()
    np.save(os.path.join(out_dir, 'ae_rank%d.npy' % rank), np.stack([a.params.cpu().numpy() for a in tr.autoexpo]))
    np.save(os.path.join(out_dir, 'ae_steps_rank%d.npy' % rank), np.stack([a.steps.cpu().numpy() for a in tr.autoexpo]))
    dist.barrier()
    dist.destroy_process_group()


def test_two_ranks_autoexposure(tmp_path):
    """--optim_autoexpo under DP: each rank trains on its own image; the per-image parameters are
    all-reduced like every other gradient, so both ranks hold identical values, every image used by
    either rank has been stepped exactly once and the untouched ones keep their initial value."""
    if not torch.cuda.is_available():
        pytest.skip('needs a GPU')
    import torch.multiprocessing as mp
    mp.spawn(_worker_ae, args=(2, _free_port(), str(tmp_path)), nprocs=2, join=True)
    a0, a1 = np.load(tmp_path / 'ae_rank0.npy'), np.load(tmp_path / 'ae_rank1.npy')
    np.testing.assert_array_equal(a0, a1)
    steps = np.load(tmp_path / 'ae_steps_rank0.npy')
    np.testing.assert_array_equal(steps, np.ones_like(steps))              # images 0..3, both levels: one step each
    assert (np.abs(a0 - np.array([0.5, 0.0], np.float32)).max(-1) > 1e-5).all()


# ---------------------------------------------------------------------------------------------------------------
# round 2: the HIP gradients against the REFERENCE's 2-rank average (tests/golden/ddp2.npz), over gloo on one GPU
# and over RCCL on two; bench.py --gpus N launching its own ranks
# ---------------------------------------------------------------------------------------------------------------
GOLDEN_DDP2 = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'ddp2.npz')
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _worker_ddp2(rank, world, port, out_path, backend, share_gpu):
    """One DDP rank: its own batch of ddp2.npz through the HIP level-0 forward / loss / backward with the
    gradients pre-scaled by 1/world (trainer.py), then ONE all-reduce(SUM) -- DDP's average (ddp_train_nerf.py:323)."""
    import torch.distributed as dist
    from oracle import nerfpp_oracle as O
    from outdoor_nerf_depth_amd import ops
    os.environ['MASTER_ADDR'] = '127.0.0.1'
    os.environ['MASTER_PORT'] = str(port)
    dev = torch.device('cuda', 0 if share_gpu else rank)
    torch.cuda.set_device(dev)
    if backend == 'nccl':
        dist.init_process_group('nccl', rank=rank, world_size=world, device_id=dev)
    else:
        dist.init_process_group(backend, rank=rank, world_size=world)
    g = np.load(GOLDEN_DDP2)
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    level = O.init_params_like_reference(1)[0]
    flat = np.concatenate([level[k].reshape(-1) for k in O.param_order()]).astype(np.float32)
    eng = ops.LevelEngine(T(flat), precision=2)
    pre = 'r%d.' % rank
    far, fg_z, bg_z = ops.sample_coarse(T(g[pre + 'ray_o']), T(g[pre + 'ray_d']), T(g[pre + 'min_depth']), 64,
                                        t_rand_fg=T(g[pre + 't_fg']), t_rand_bg=T(g[pre + 't_bg']))
    ret = eng.forward(T(g[pre + 'ray_o']), T(g[pre + 'ray_d']), far, fg_z, bg_z, training=True)
    sc, g_rgb, g_depth, g_w = ops.loss_and_grads(ret, T(g[pre + 'rgb']), T(g[pre + 'depth_sup']), 'mse', 0.1)
    grads = eng.backward(g_rgb, g_depth, g_w, grad_scale=1.0 / world)
    dist.all_reduce(grads)
    torch.cuda.synchronize()
    np.save(out_path % rank, grads.cpu().numpy())
    dist.barrier()
    dist.destroy_process_group()


def _check_against_ddp2(avg):
    from oracle import nerfpp_oracle as O
    g = np.load(GOLDEN_DDP2)
    shapes, off = {}, 0
    for net, in_ch in (('fg_net', 63), ('bg_net', 84)):
        for k, s in O.mlp_param_shapes(in_ch, 27).items():
            shapes['%s.%s' % (net, k)] = s
    for k in O.param_order():
        n = int(np.prod(shapes[k]))
        mine = avg[off:off + n][g['avg.%s.idx' % k]]
        assert np.abs(mine - g['avg.%s.g' % k]).max() <= 5e-2 * g['avg.%s.rms' % k] + 1e-12, k
        off += n


def test_hip_two_rank_average_matches_reference_ddp2_gloo(tmp_path):
    """a16 on ONE GPU: two processes share cuda:0, all-reduce over gloo; the averaged HIP gradients against the
    reference's own 2-rank emulation (float64 run, tests/golden/ddp2.npz) -- not against HIP itself."""
    if not torch.cuda.is_available():
        pytest.skip('needs a GPU')
    import torch.multiprocessing as mp
    out = str(tmp_path / 'avg_rank%d.npy')
    mp.spawn(_worker_ddp2, args=(2, _free_port(), out, 'gloo', True), nprocs=2, join=True)
    a0, a1 = np.load(out % 0), np.load(out % 1)
    np.testing.assert_array_equal(a0, a1)
    _check_against_ddp2(a0)


def test_hip_two_rank_average_matches_reference_ddp2_rccl(tmp_path):
    """a16 over RCCL: one process per GPU, backend nccl (= RCCL over xGMI).  Skipped on 1-GPU boxes."""
    if not torch.cuda.is_available() or torch.cuda.device_count() < 2:
        pytest.skip('needs 2 GPUs, found %d' % torch.cuda.device_count())
    import torch.multiprocessing as mp
    out = str(tmp_path / 'avg_rank%d.npy')
    mp.spawn(_worker_ddp2, args=(2, _free_port(), out, 'nccl', False), nprocs=2, join=True)
    a0, a1 = np.load(out % 0), np.load(out % 1)
    np.testing.assert_array_equal(a0, a1)
    _check_against_ddp2(a0)


def _run_bench(extra, env_extra, timeout=900):
    import subprocess
    import sys
    env = dict(os.environ, **env_extra)
    env.pop('WORLD_SIZE', None)
    env.pop('RANK', None)
    return subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), '--steps', '3', '--warmup', '1', '--n_rand', '128',
                           '--no_cpu_baseline', '--large_batch', '0', '--full'] + extra, capture_output=True, text=True,
                          timeout=timeout, cwd=ROOT, env=env)


def test_bench_gpus_2_launches_its_own_ranks(tmp_path):
    """`python bench.py --gpus 2` must itself start 2 ranks and print n_gpus: 2.  On a box with
    2+ GPUs this runs RCCL; on a 1-GPU box the two ranks share cuda:0 over gloo (test hook) -- and WITHOUT the hook
    the run must fail loudly rather than report N=1."""
    if not torch.cuda.is_available():
        pytest.skip('needs a GPU')
    import json
    if torch.cuda.device_count() >= 2:
        out = _run_bench(['--gpus', '2'], {})
        assert out.returncode == 0, out.stderr[-2000:]
    else:
        loud = _run_bench(['--gpus', '2'], {})
        assert loud.returncode != 0 and 'only 1 GPU' in (loud.stderr + loud.stdout)
        out = _run_bench(['--gpus', '2'], {'NERFPP_SHARE_GPU': '1', 'NERFPP_DIST_BACKEND': 'gloo'})
        assert out.returncode == 0, out.stderr[-2000:]
    lines = [l for l in out.stdout.strip().splitlines() if l.startswith('{')]
    assert len(lines) == 1
    r = json.loads(lines[0])
    assert r['n_gpus'] == 2 and r['config']['n_rand_per_gpu'] == 128
    assert abs(r['value'] - 2 * 128 / (r['ms_per_step'] * 1e-3)) <= 1e-6 * r['value']
    # a launcher environment that disagrees with --gpus is an error, not a silent N
    import subprocess
    import sys
    bad = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), '--gpus', '2', '--steps', '2', '--warmup', '1'],
                         capture_output=True, text=True, timeout=300, cwd=ROOT,
                         env=dict(os.environ, WORLD_SIZE='1', RANK='0', LOCAL_RANK='0'))
    assert bad.returncode != 0 and 'WORLD_SIZE=1' in (bad.stderr + bad.stdout)


def test_bench_second_transport_cannot_cost_the_line():
    """Round 6: `bench.py --gpus N` runs the job a second time through the library's own RCCL entry point (--grad_comm both) -- a
    path that has never run on more than one GPU.  It runs last, and neither a failure nor a hang there may cost the run its
    torch.distributed number.  On a 1-GPU box both are provoked: two ranks on one device make nerfpp_rccl_comm_init fail (RCCL
    refuses) or block; the line must come out either way, with the reason in config.grad_comm_rccl_abi."""
    if not torch.cuda.is_available():
        pytest.skip('needs a GPU')
    if torch.cuda.device_count() >= 2:
        pytest.skip('provokes the failure paths by sharing one device')
    import json
    hook = {'NERFPP_SHARE_GPU': '1', 'NERFPP_DIST_BACKEND': 'gloo', 'NERFPP_BENCH_FORCE_ABI_SECOND': '1'}
    for extra, expect in (({'NERFPP_BENCH_ABI_TIMEOUT_S': '60'}, None), ({'NERFPP_BENCH_ABI_TIMEOUT_S': '0.05'}, 'timed out')):
        out = _run_bench(['--gpus', '2', '--mip360_rays', '0'], dict(hook, **extra), timeout=600)
        assert out.returncode == 0, out.stderr[-2000:]
        lines = [l for l in out.stdout.strip().splitlines() if l.startswith('{')]
        assert len(lines) == 1, out.stdout[-2000:]
        r = json.loads(lines[0])
        assert r['n_gpus'] == 2 and r['value'] > 0
        second = r['config']['grad_comm_rccl_abi']
        assert second is not None and 'error' in second, second
        if expect:
            assert expect in second['error'], second


# ---------------------------------------------------------------------------------------------------------------
# round 3: the 8-rank code paths -- bench.py --gpus 8 and the ragged inference sharding of a
# 375 x 1242 frame over 8 ranks.  With 8 GPUs every rank has its own device (bench.py: RCCL, BASELINE configs[4]).  With
# fewer the ranks share cuda:0 over gloo (numbers from such a run mean nothing; what is checked is that the ranks
# rendezvous, step in lock-step, report the diagnostics and produce the same frame as one rank), and fewer of them: every
# rank is a process with the GPU open, next to this one (and, for bench.py, its launcher), and a test keeps at most 6
# such processes on one GPU.  4 ranks still shard the frame raggedly (465 750 = 4 x 116 437 + 2); the bench smoke runs 3.
# ---------------------------------------------------------------------------------------------------------------
SHARED_BENCH_RANKS, SHARED_RENDER_RANKS = 3, 4


def _ranks(shared):
    """(number of ranks, one GPU per rank?): 8 on a box with 8 GPUs, else `shared` ranks on cuda:0"""
    return (8, True) if torch.cuda.device_count() >= 8 else (shared, False)


def test_bench_gpus_8_shared_gpu_smoke():
    if not torch.cuda.is_available():
        pytest.skip('needs a GPU')
    import json
    n, spread = _ranks(SHARED_BENCH_RANKS)
    if spread:
        out = _run_bench(['--gpus', str(n), '--mip360_rays', '0'], {}, timeout=1500)
    else:
        out = _run_bench(['--gpus', str(n), '--mip360_rays', '0'], {'NERFPP_SHARE_GPU': '1', 'NERFPP_DIST_BACKEND': 'gloo'}, timeout=1500)
    assert out.returncode == 0, out.stderr[-3000:]
    lines = [l for l in out.stdout.strip().splitlines() if l.startswith('{')]
    assert len(lines) == 1
    r = json.loads(lines[0])
    assert r['n_gpus'] == n and r['scaling'] == 'weak' and r['config']['n_rand_per_gpu'] == 128
    assert abs(r['value'] - n * 128 / (r['ms_per_step'] * 1e-3)) <= 1e-6 * r['value']
    assert r['config']['dist_backend'].split(',')[0] in ('nccl', 'gloo')
    assert 'NCCL_MAX_NCHANNELS=' in r['config']['dist_backend']             # RCCL's footprint is part of the configuration
    per_rank, exposed = r['config']['per_rank_ms_per_step'], r['config']['exposed_update_ms_per_step']
    assert len(per_rank) == n and len(exposed) == n
    assert all(0 < t <= r['ms_per_step'] * 1.001 for t in per_rank)          # the reported time is the slowest rank's
    assert all(e >= 0 for e in exposed)
    assert all(np.isfinite(r['final_loss']))
    # first-contact diagnostics of a scaling run: the gradient all-reduce of each cascade level timed on
    # every rank, the transport named, the channel counts read back from RCCL's INIT log where there is an RCCL
    ar = r['config']['allreduce_ms']
    assert sorted(ar) == ['level0', 'level1'] and all(len(v) == n and all(t > 0 for t in v) for v in ar.values())
    assert r['config']['grad_comm'] == 'torch'
    if r['config']['dist_backend'].startswith('nccl'):
        ch = r['config']['rccl_channels_in_effect']
        assert ch and all(c['coll'] >= 1 for c in ch), ch
        second = r['config']['grad_comm_rccl_abi']                            # --grad_comm both is the default
        assert second and ('error' in second or (second['value'] > 0 and len(second['allreduce_ms']['level1']) == n)), second
    else:
        assert r['config']['rccl_channels_in_effect'] is None and r['config']['grad_comm_rccl_abi'] is None


def _worker_render(rank, world, port, out_path, H, W, spread):
    import torch.distributed as dist
    from outdoor_nerf_depth_amd.trainer import NerfppTrainer
    from outdoor_nerf_depth_amd.ddp_train_nerf import render_single_image
    from outdoor_nerf_depth_amd.data_loader_split import synthetic_ray_samplers
    os.environ['MASTER_ADDR'] = '127.0.0.1'
    os.environ['MASTER_PORT'] = str(port)
    dist.init_process_group('gloo', rank=rank, world_size=world)
    dev = torch.device('cuda', rank if spread else 0)
    torch.cuda.set_device(dev)
    sampler = synthetic_ray_samplers('test', 1, 'gt', 20, H, W)[0]
    tr = NerfppTrainer(dev, precision=1, use_depth=False, world_size=1)      # identical weights on every rank (manual_seed(777))
    ret = render_single_image(rank, world, tr, sampler, 8192, keep_dists=False)
    if rank == 0:
        np.savez(out_path, **{'L%d.%s' % (m, k): v.numpy() for m, lvl in enumerate(ret) for k, v in lvl.items()})
    else:
        assert ret is None
    dist.barrier()
    dist.destroy_process_group()


def test_render_single_image_ragged_over_8_ranks(tmp_path):
    """f-2 with P = 8 (4 ranks sharing cuda:0 on a box with fewer GPUs): 375 * 1242 = 465 750 rays is divisible by neither
    (the reference raises, ddp_train_nerf.py:137-139); here the last rank takes the remainder.  The gathered frame equals
    the one-rank frame bit for bit (same kernels, same chunking inside every shard's own ray range would differ, so the
    comparison frame is rendered with the SAME shards)."""
    if not torch.cuda.is_available():
        pytest.skip('needs a GPU')
    import torch.multiprocessing as mp
    from outdoor_nerf_depth_amd import dist_utils as D
    H, W = 375, 1242
    n, spread = _ranks(SHARED_RENDER_RANKS)
    sizes = D.shard_sizes(H * W, n)
    assert sum(sizes) == H * W and sizes[-1] != sizes[0] and len(set(sizes[:-1])) == 1
    out = str(tmp_path / 'frame.npz')
    mp.spawn(_worker_render, args=(n, _free_port(), out, H, W, spread), nprocs=n, join=True)
    got = np.load(out)
    # one process, the same shards one after the other
    from outdoor_nerf_depth_amd.trainer import NerfppTrainer
    from outdoor_nerf_depth_amd.data_loader_split import synthetic_ray_samplers
    from outdoor_nerf_depth_amd import ops
    dev = torch.device('cuda:0')
    sampler = synthetic_ray_samplers('test', 1, 'gt', 20, H, W)[0]
    tr = NerfppTrainer(dev, precision=1, use_depth=False)
    b = sampler.get_all()
    rgb, depth = [], []
    lo = 0
    for sz in sizes:
        T = lambda a: torch.from_numpy(np.ascontiguousarray(a[lo:lo + sz])).to(dev)
        ray_o, ray_d, md = T(b['ray_o']), T(b['ray_d']), T(b['min_depth'])
        for s in range(0, sz, 8192):
            o, d, m_ = ray_o[s:s + 8192], ray_d[s:s + 8192], md[s:s + 8192]
            far, fg_z, bg_z = ops.sample_coarse(o, d, m_, 64, perturb=False)
            ret = tr.engines[0].forward(o, d, far, fg_z, bg_z)
            fg_z, bg_z = ops.sample_fine_pair(fg_z, ret['fg_weights'], bg_z, ret['bg_weights'], 128, det=True)
            ret = tr.engines[1].forward(o, d, far, fg_z, bg_z)
            rgb.append(ret['rgb'].cpu().numpy())
            depth.append(ret['depth'].cpu().numpy())
        lo += sz
    assert got['L1.rgb'].shape == (H, W, 3) and got['L1.depth'].shape == (H, W)
    np.testing.assert_array_equal(got['L1.rgb'].reshape(-1, 3), np.concatenate(rgb))
    np.testing.assert_array_equal(got['L1.depth'].reshape(-1), np.concatenate(depth))
    assert np.isfinite(got['L1.rgb']).all() and np.isfinite(got['L0.depth']).all()

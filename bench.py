#!/usr/bin/env python
"""Headline benchmark: NeRF++ training ray-steps per second on synthetic KITTI-shaped batches.

  python bench.py --gpus N --steps K --warmup W [--dump-outputs DIR] [--full]

A plain run measures the headline alone: it sets up, warms up, times the K steps, writes --dump-outputs and prints the line
(with the roofline of the headline run's own kernel taps).  --full also runs every other leg listed below (other precisions,
sizes and transports, the MipNeRF-360 step, rendering, the drop-in loop, the CPU baseline, the vendor GEMM), each after the
headline run, so the headline fields are the same with or without it.

--dump-outputs DIR: after the timed steps, the headline run's last step -- the per-level scalars train_step returns and each
level's parameters after that step's update -- as DIR/<name>.npy (float32, ~10 MB).  The inputs are seeded, so two builds run
with the same arguments can be compared output for output.  With N > 1 it is rank 0's step: the scalars of its own batches,
the parameters every rank holds after the gradient all-reduce.

N > 1: when no torch.distributed.run environment is present (no WORLD_SIZE) this process launches the N
ranks itself, one per GPU, the way the reference spawns its workers
(nerf-methods/nerfplusplus/ddp_train_nerf.py:738-745); under `python -m torch.distributed.run ... bench.py
--gpus N` it is one of those ranks.  Either way every rank asserts world_size == N and uses backend nccl
(= RCCL); a box with fewer than N GPUs fails loudly instead of reporting a smaller N.

One "step" = one optimisation step of ddp_train_nerf.py:417-498 for N_rand rays per GPU: stratified +
inverse-CDF sampling, both cascade levels (64 and 64+128 samples per ray, fg + bg networks), loss
(depth_sup_type=gt, depth_loss_type=mse, lambda_depth=0.1 = BASELINE config 2), backward, gradient
all-reduce (N > 1) and Adam.  Ray batches are resident in HBM before the timed region.  Prints ONE JSON
line (rank 0).

Every trainer is set up with SETUP_STEPS untimed steps (code objects, workspaces, and the GPU back at its steady clock:
an MI355X needs ~20 ms of load after any idle, profiles/r03_step_curve.json) before the W warm-up and K timed steps.

value               : single-pass bf16 MFMA operands (the arithmetic north_star names), rays/s over all GPUs
roofline            : SURVEY 8(d): algorithmic dense-layer FLOP (1.797 GFLOP per ray-step) against the dense
                      bf16 MFMA peak -- whole step and dominant kernel group, timed live with HIP events on
                      the launch stream; the HBM view of the weight-gradient GEMM as a sub-object; and, with --full, as
                      context for the nominal peak, what hipBLASLt's 8192^3 bf16 GEMM gets from the same socket (vendor_gemm_same_socket)
gates               : which test gate each of the precisions' numbers has passed

--full only:
end_to_end          : what a user of the drop-in loop gets: ddp_train_nerf() itself on the 295-frame scene (cli_loop.device_sampler),
                      and trained_state_ms = the kernel-only step on that loop's trained state
parity_forward_mode : split-bf16 forward (rendered RGB / depth / loss within 1e-4 of float32) + bf16 backward
fp16_forward_mode   : fp16x2w forward (2 MFMA passes; 1e-4 at initialisation, 3-4e-4 on trained weights: NOT the 1e-4 clause) + bf16 backward
parity_mode         : split-bf16 everywhere (3 MFMA passes): the mode the 1e-4 parity tests run in
large_batch         : the bf16 step at N_rand = --large_batch
config5_mip360      : the MipNeRF-360 step at --mip360_rays (N > 1: data-parallel over the same ranks)
config.grad_comm_rccl_abi : N > 1, --grad_comm both: the bf16 step again through the library's own RCCL entry point
cpu_baseline        : oracle/nerfpp_torch_cpu.py (PyTorch-CPU restatement of the path, the way the reference
                      runs on CPU) on the host cores: N_rand 1024, 2 warm-up + 5 timed steps, median
render              : SURVEY 8 f-2: one 375x1242 frame through render_single_image, whole call and MLP kernels alone
cli_loop            : the drop-in training loop itself (ddp_train_nerf(): per-step frame choice, ray-batch sampling, log lines)
                      with the device sampler and with the reference's host sampler, ms per step beside the kernel-only figure
power               : socket power, power cap and shader clock (amdgpu hwmon) while the end_to_end loop ran: the MLP kernels hold
                      the socket at its cap and the clock gives way (profiles/r06_power_trace.md); null where hwmon is not readable
"""
import argparse
import json
import os
import socket
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

PEAK_BF16_TFLOPS = 2500.0        # MI355X dense bf16 MFMA (MI355X_MICROARCH.md)
PEAK_HBM_GBS = 8000.0            # HBM3E spec (6.3 TB/s measured copy ceiling)
FLOP_PER_RAY_STEP = 1.797e9      # 256 fg+bg sample pairs x 3 510 528 MACs x 2
SURVEY_ALGO_BYTES_PER_RAY = 18.8e3   # inputs + outputs + amortised weights/grads at N_rand = 1024
# algorithmic bytes per sample row read by the weight-gradient GEMMs (every operand once per job):
# sum over jobs of (dZ cols + input cols) * 2 B, fg + bg
EXEC_OVER_ALGO = {'mlp_fwd': 1.0 - 2 * 65536.0 / (593408 + 604160), 'mlp_bwd': 1.0 - 2 * 65536.0 / (2 * 557696), 'dw': 1.0}
DW_BYTES_PER_ROW = (4576 + 4640) * 2        # columns the jobs of nerfpp_common.h: build_all_jobs read per row (fg + bg), bf16
# a bf16 backward: job L1 reads the encoded point (64 / 96 columns) instead of H0 (256) and recomputes it (nerfpp_dw.hip: rc_job);
# job L7 reads [dS | dG] (160 columns) and one 16-byte sign word per lane (32 B per row) instead of dZ7 (256) (rc7_job)
DW_BYTES_PER_ROW_BF16 = (4576 - 192 - 96 + 4640 - 160 - 96) * 2 + 2 * 32
FLOP_PER_RAY_RENDER = 0.613e9    # forward only, both levels
SETUP_STEPS = 12                 # untimed steps run when a trainer is set up, before the W warm-up steps (see run_mode)
# HBM bytes per LEVEL-1 launch group at N_rand = 1024, bf16: PARSED at start-up from the rocprofv3 --pmc passes committed
# under profiles/ (they cannot be collected inside this process: separate --pmc runs, MI355X_MICROARCH.md "HBM").  The
# field is named `traffic_from_profile`-style in the output (`traffic_source`), it is not a live measurement.
PMC_PROFILE = os.path.join('profiles', 'r06_final_kernel_stats_timeline_hbm.md')
PMC_PROFILE_FALLBACK = os.path.join('profiles', 'r05_final_kernel_stats_timeline_hbm.md')
# kernel sources whose change invalidates the committed PMC numbers: the profile records their sha256 (`sources_sha256:` line,
# written by tools/probes/assemble_profile.py); a mismatch turns `traffic` into null with the reason in `traffic_source`, and
# tests/test_host_logic.py::test_committed_pmc_profile_matches_kernel_sources fails the CPU suite until the profile is redone
PMC_SOURCES = ('nerfpp_mlp.hip', 'nerfpp_mlp_split.h', 'nerfpp_dw.hip', 'nerfpp_common.h')


def kernel_sources_sha256():
    import hashlib
    h = hashlib.sha256()
    for f in PMC_SOURCES:
        h.update(open(os.path.join(ROOT, 'outdoor_nerf_depth_amd', 'csrc', f), 'rb').read())
    return h.hexdigest()[:16]
PMC_GROUPS = {            # launch group -> kernel-name prefix of its bf16 training instantiations (both nets / both launches)
    'dw_L1': 'dw_kernel<1,',
    'mlp_fwd_L1': 'mlp_fwd_kernel<',
    'mlp_bwd_L1': 'mlp_bwd_kernel<',
}


def load_pmc_traffic():
    """{'source': file, group: bytes per level-1 launch group} from the `## kernel (dispatches: n)` / `FETCH_SIZE avg x`
    blocks (KB) that tools/rocpd_pmc.py wrote into the round's profile.  Per dispatch: 2 x FETCH_SIZE (gfx950 counts 64 B
    per 128-B request of a wide stream) + WRITE_SIZE; the file averages level-0 and level-1 dispatches (rows 1 : 3), so a
    level-1 launch is 1.5 x the average.  Returns None when no profile is there (then `traffic` is null)."""
    import re
    for rel in (PMC_PROFILE, PMC_PROFILE_FALLBACK):
        path = os.path.join(ROOT, rel)
        if not os.path.exists(path):
            continue
        per = {}
        name = None
        recorded = None
        for line in open(path):
            m = re.match(r'^sources_sha256:\s*([0-9a-f]+)', line)
            if m:
                recorded = m.group(1)
                continue
            m = re.match(r'^## (.+?)\s+\(dispatches: \d+\)', line)
            if m:
                name = m.group(1)
                continue
            m = re.match(r'^\s+(FETCH_SIZE|WRITE_SIZE)\s+avg\s+([0-9.eE+-]+)', line)
            if m and name:
                per.setdefault(name, {})[m.group(1)] = float(m.group(2)) * 1e3
        now = kernel_sources_sha256()
        if recorded != now:
            return {'stale': '%s was measured on kernel sources %s, the tree has %s: traffic withheld until the PMC passes are redone'
                             % (rel, recorded or '(unrecorded)', now)}
        out = {'source': rel + ' (NOT a live measurement: rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE passes of the committed profile, '
                               'measured on kernel sources sha256 ' + now + ', parsed at start-up)', 'kernels': {}}
        for grp, prefix in PMC_GROUPS.items():
            if grp == 'dw_L1':                    # dw_kernel<1, true> (256 x 256 jobs) + dw_kernel<1, false> (narrow jobs)
                ks = [k for k in per if k.startswith(prefix)]
            else:
                # round 4: mlp_fwd_pair_kernel<P = 1, 8 waves, TRAIN = true> / mlp_bwd_pair_kernel<1, 8> (both nets in one launch)
                pair = prefix.replace('_kernel<', '_pair_kernel<')
                ks = [k for k in per if k.startswith(pair + '1, 8') and not k.endswith('false>')]
                if not ks:                        # rounds 1-3: <net, P = 1, 8 waves[, TRAIN = true]>, one launch per net
                    ks = [k for k in per if k.startswith(prefix) and ', 1, 8' in k and not k.endswith('false>')]
            ks = [k for k in ks if 'FETCH_SIZE' in per[k] and 'WRITE_SIZE' in per[k]]
            if not ks:
                return None
            out[grp] = 1.5 * sum(2.0 * per[k]['FETCH_SIZE'] + per[k]['WRITE_SIZE'] for k in ks)
            out['kernels'][grp] = sorted(ks)
        return out
    return None


PMC_TRAFFIC = load_pmc_traffic()
PMC_STALE = PMC_TRAFFIC.get('stale') if PMC_TRAFFIC else None
if PMC_STALE:
    PMC_TRAFFIC = None


def parse():
    p = argparse.ArgumentParser()
    p.add_argument('--gpus', type=int, default=1)
    p.add_argument('--steps', type=int, default=20)
    p.add_argument('--warmup', type=int, default=3)
    p.add_argument('--n_rand', type=int, default=1024, help='rays per GPU per step (reference forces 1024)')
    p.add_argument('--full', action='store_true',
                   help='after the headline run, also run the other legs: split-bf16 / split_fwd / fp16_fwd, --large_batch, '
                        '--mip360_rays, --render_frames, --cli_steps, the CPU baseline, the vendor GEMM and (N > 1) the second '
                        'gradient transport of --grad_comm both.  Without it a run measures the headline alone')
    p.add_argument('--precision', choices=['both', 'bf16', 'split'], default='both',
                   help='headline precision: bf16 (both, bf16) or split-bf16 (split); with --full, both also runs the split-bf16 legs')
    p.add_argument('--no_cpu_baseline', action='store_true')
    p.add_argument('--grad_comm', choices=['torch', 'rccl_abi', 'both'], default='both',
                   help='N > 1: transport of the gradient all-reduce -- torch.distributed (backend nccl = RCCL), the library\'s own RCCL '
                        'entry point (nerfpp_allreduce_mean), or both one after the other in the same job (the headline is torch; the '
                        'second, run with --full only, is reported under config.grad_comm_rccl_abi).  Over gloo (test hook) only torch '
                        'exists')
    p.add_argument('--rccl_channels', type=int, default=-1, help='-1: NCCL_MAX_NCHANNELS=4 (one node), 0: RCCL\'s own choice, N: N')
    p.add_argument('--large_batch', type=int, default=8192, help='also report this N_rand (0 = skip)')
    p.add_argument('--mip360_rays', type=int, default=4096, help='also time the MipNeRF-360 step (config 5) at this many rays (0 = skip)')
    # BASELINE.json configs[1] by default (gt / mse / 0.1); configs[2] = mono_crop / kl, configs[3] = stereo_crop / l1
    p.add_argument('--depth_sup_type', default='gt')
    p.add_argument('--depth_loss_type', default='mse', choices=['mse', 'l1', 'kl'])
    p.add_argument('--lambda_depth', type=float, default=0.1)
    p.add_argument('--cpu_rays', type=int, default=1024, help='N_rand of the CPU baseline (SURVEY 8d: 1024)')
    p.add_argument('--render_frames', type=int, default=1,
                   help='375x1242 frames rendered per precision by the inference leg (`render`; 0 = skip)')
    p.add_argument('--render_chunk', type=int, default=8192, help='rays per render chunk (ddp_train_nerf.py --chunk_size)')
    p.add_argument('--cli_frames', type=int, default=295, help='frames of the synthetic sequence the drop-in loop trains on (config 2: 295)')
    p.add_argument('--cli_steps', type=int, default=800,
                   help='steps of the drop-in training loop (outdoor_nerf_depth_amd/ddp_train_nerf.py) timed by `cli_loop` (0 = skip)')
    p.add_argument('--dump-outputs', dest='dump_outputs', metavar='DIR', default=None,
                   help='write what the headline run computed in its last timed step as DIR/<name>.npy (float32): the per-level '
                        'scalars train_step returns and each level\'s parameters after that step\'s update.  With --gpus N > 1: rank 0\'s '
                        '(its own batches\' scalars; the parameters are the same on every rank after the all-reduce)')
    a = p.parse_args()
    if a.steps < 1 or a.warmup < 0:
        p.error('--steps must be >= 1 and --warmup >= 0')
    return a


def _free_port():
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    port = s.getsockname()[1]
    s.close()
    return port


def rccl_env_defaults(channels=-1):
    """environment defaults of an N > 1 run (one node by construction: this script spawns / is launched with one rank per local
    GPU): the channel cap (dist_utils.py) and RCCL's INIT lines to a per-process file, from which the channel count the
    communicators actually got is read back (config.rccl_channels_in_effect)"""
    from outdoor_nerf_depth_amd.dist_utils import RCCL_ENV_DEFAULTS, rccl_debug_file_env
    env = {} if channels == 0 else dict(RCCL_ENV_DEFAULTS) if channels < 0 else \
        {'NCCL_MAX_NCHANNELS': str(channels), 'NCCL_MIN_NCHANNELS': str(min(2, channels))}
    env.update(rccl_debug_file_env('nerfpp_bench'))
    return env


def _channels_arg():
    for i, a in enumerate(sys.argv):
        if a == '--rccl_channels' and i + 1 < len(sys.argv):
            return int(sys.argv[i + 1])
        if a.startswith('--rccl_channels='):
            return int(a.split('=', 1)[1])
    return -1


def spawn_ranks(n):
    """--gpus N without a launcher: start N copies of this script, one rank per GPU (the reference does the
    same with torch.multiprocessing.spawn, ddp_train_nerf.py:742-745).  Rank 0's stdout is ours."""
    import torch
    have = torch.cuda.device_count()
    if have < n and not os.environ.get('NERFPP_SHARE_GPU'):
        raise SystemExit('bench.py --gpus %d: only %d GPU(s) visible on this box -- refusing to report a smaller '
                         'job as N=%d' % (n, have, n))
    port = _free_port()
    procs = []
    for r in range(n):
        env = dict(os.environ, RANK=str(r), LOCAL_RANK=str(r), WORLD_SIZE=str(n), MASTER_ADDR='127.0.0.1',
                   MASTER_PORT=str(port), HSA_ENABLE_IPC_MODE_LEGACY=os.environ.get('HSA_ENABLE_IPC_MODE_LEGACY', '0'))
        for k, v in rccl_env_defaults(_channels_arg()).items():
            env.setdefault(k, v)
        procs.append(subprocess.Popen([sys.executable, os.path.abspath(__file__)] + sys.argv[1:], env=env,
                                      stdout=None if r == 0 else subprocess.DEVNULL))
    # poll: as soon as one rank exits non-zero the others are terminated (a dead rank would otherwise leave the rest
    # blocked in an RCCL collective until its timeout, and the bench would hang instead of failing loudly)
    rcs = [None] * n
    deadline = time.time() + float(os.environ.get('NERFPP_BENCH_TIMEOUT_S', '1800'))
    while any(rc is None for rc in rcs):
        for i, p in enumerate(procs):
            if rcs[i] is None:
                rcs[i] = p.poll()
        failed = [i for i, rc in enumerate(rcs) if rc not in (None, 0)]
        if failed or time.time() > deadline:
            for i, p in enumerate(procs):
                if rcs[i] is None:
                    p.terminate()
            for i, p in enumerate(procs):
                if rcs[i] is None:
                    try:
                        rcs[i] = p.wait(timeout=10)
                    except subprocess.TimeoutExpired:
                        p.kill()
                        rcs[i] = p.wait()
            raise SystemExit('bench.py --gpus %d: %s; rank exit codes %r' %
                             (n, 'rank(s) %r failed' % failed if failed else 'timed out', rcs))
        time.sleep(0.2)


def run_mode(args, precision, rank, world, device, batches, comm=None, outputs=None):
    """outputs: a dict that, when given, receives numpy copies of what the last timed step computed (taken after the timed
    region): `last_step_scalars` [levels, 4] = train_step's per-level [loss, rgb_loss, depth_loss, n_valid], and
    `params_level<m>` = level m's flat float32 parameters after that step's Adam update"""
    import torch
    from outdoor_nerf_depth_amd.trainer import NerfppTrainer, ALGO_MACS
    from outdoor_nerf_depth_amd.synthetic import SyntheticKitti

    scale = float(SyntheticKitti().depth_scale)
    tr = NerfppTrainer(device, precision=precision, use_depth=True, depth_loss_type=args.depth_loss_type,
                       lambda_depth=args.lambda_depth, depth_scale=scale, world_size=world, seed=(rank + 1) * 777, comm=comm)
    K, W = args.steps, args.warmup
    # live kernel taps: HIP events recorded by the library around the level-1 kernel groups (both nets), on the
    # launch stream, inside the timed region.  An event record costs ~6 us of queue time, so only every TAP-th
    # timed step carries them (>= 3 tapped steps) and level 0 is not tapped.  A tapped step runs level 0's backward inline
    # instead of under level 1's forward (NerfppTrainer.concurrent_backward: ~1 % of a step), so a tap times its group alone.
    mk = lambda: torch.cuda.Event(enable_timing=True)
    TAP = max(1, min(4, K // 3))
    tapped = [i for i in range(K) if i % TAP == 0]
    events = {}
    for i in tapped:
        ev = {'fwd': (mk(), mk()), 'bwd': (mk(), mk(), mk(), mk())}
        for e in ev['fwd'] + ev['bwd']:
            e.record()                           # materialise the hipEvent_t handles
        events[i] = [None, ev]
    # Engine set-up (untimed, reported as config.setup_steps): code objects loaded, workspaces allocated and touched, and
    # the GPU back at its steady clock -- after any idle an MI355X needs ~20 ms of this load (8 steps) to ramp
    # (profiles/r03_step_curve.json); the W warm-up steps below then start from the state a training run is in
    for i in range(SETUP_STEPS):
        tr.train_step(batches[i % len(batches)])
    for i in range(W):
        tr.train_step(batches[i])
    tr.flush()
    torch.cuda.synchronize()
    if world > 1:
        import torch.distributed as dist
        dist.barrier()
    torch.cuda.synchronize()
    if world > 1:
        tr.wait_taps = []                        # exposed (un-hidden) part of the side-stream update incl. the all-reduce
        tr.comm_taps = []                        # (level, begin, end) events around every gradient all-reduce, on its stream
    t0 = time.perf_counter()
    last = None
    for i in range(K):
        last = tr.train_step(batches[W + i], events=events.get(i))
    tr.flush()                                   # the last step's level-1 all-reduce + Adam belong to the timed region
    torch.cuda.synchronize()
    own = time.perf_counter() - t0               # this rank's own clock, before waiting for the others
    if world > 1:
        dist.barrier()
    torch.cuda.synchronize()
    elapsed = time.perf_counter() - t0
    per_rank, exposed, allreduce_ms = None, None, None
    if world > 1:
        t = torch.tensor([elapsed], device=device, dtype=torch.float64)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        elapsed = float(t.item())
        # diagnosis of a scaling run: every rank's own ms per step, the update time its main stream had to wait for, and the
        # duration of its gradient all-reduces (median over the timed steps) per cascade level, as its GPU saw them
        ar = [[a_.elapsed_time(b_) for m_, a_, b_ in tr.comm_taps if m_ == lvl] for lvl in range(2)]
        mine = torch.tensor([1e3 * own / K, sum(a.elapsed_time(b) for a, b in tr.wait_taps) / K] +
                            [float(np.median(x)) if x else -1.0 for x in ar], device=device, dtype=torch.float64)
        allr = [torch.zeros_like(mine) for _ in range(world)]
        dist.all_gather(allr, mine)
        per_rank = [round(float(x[0]), 4) for x in allr]
        exposed = [round(float(x[1]), 4) for x in allr]
        allreduce_ms = {'level0': [round(float(x[2]), 4) for x in allr], 'level1': [round(float(x[3]), 4) for x in allr]}
    tr.check_cameras()
    loss = [float(s[0]) for s in last]
    if outputs is not None:
        outputs['last_step_scalars'] = torch.stack([s.float() for s in last]).cpu().numpy()
        for m, e in enumerate(tr.engines):
            outputs['params_level%d' % m] = e.params.float().cpu().numpy()
    assert all(np.isfinite(loss)), 'non-finite loss %r' % (loss,)

    # live per-kernel-group timing (ms) at level 1: MLP forward (fg + bg launches), dX chain (fg + bg), dW GEMMs
    n, S1 = args.n_rand, 192
    rows = n * S1
    med = lambda xs: float(np.median(xs))
    fwd_ms = med([events[i][1]['fwd'][0].elapsed_time(events[i][1]['fwd'][1]) for i in tapped])
    bwd_ms = med([events[i][1]['bwd'][0].elapsed_time(events[i][1]['bwd'][1]) for i in tapped])
    dw_ms = med([events[i][1]['bwd'][2].elapsed_time(events[i][1]['bwd'][3]) for i in tapped])
    P = 2 if precision == 2 else 1            # precision of the backward kernels / saved planes the dW GEMM reads
    fwd_macs = ALGO_MACS['fwd'][0] + ALGO_MACS['fwd'][1]
    kernels = {
        'mlp_fwd_L1': dict(ms=fwd_ms, flop=2.0 * fwd_macs * rows),
        'mlp_bwd_L1': dict(ms=bwd_ms, flop=2.0 * (ALGO_MACS['dx'][0] + ALGO_MACS['dx'][1]) * rows),
        'dw_L1': dict(ms=dw_ms, flop=2.0 * fwd_macs * rows, bytes=float(DW_BYTES_PER_ROW * 2 if P == 2 else DW_BYTES_PER_ROW_BF16) * rows),
    }
    for k in kernels.values():
        k['tflops'] = k['flop'] / (k['ms'] * 1e-3) / 1e12
        if 'bytes' in k:
            k['gbs'] = k['bytes'] / (k['ms'] * 1e-3) / 1e9
    # share of a step: every group also runs once at level 0 on a third of the rows
    share = {k: v['ms'] * (1 + 64.0 / 192) for k, v in kernels.items()}
    # deterministic choice: groups within 2 % of the largest share count as tied and the tie goes to a fixed order
    # (forward, dX chain, weight gradients), so the reported kernel does not flip on timing noise; all tied groups are named
    order = ('mlp_fwd_L1', 'mlp_bwd_L1', 'dw_L1')
    top = max(share.values())
    tied = [k for k in order if share[k] >= 0.98 * top]
    dominant = tied[0]
    return dict(elapsed=elapsed, ms_per_step=1e3 * elapsed / K, value=n * K * world / elapsed, loss=loss,
                per_rank_ms_per_step=per_rank, exposed_update_ms_per_step=exposed, allreduce_ms=allreduce_ms,
                value_per_gpu=n * K / elapsed, kernels=kernels, dominant=dominant, co_dominant=tied, share_ms=share,
                pmc_ok=(n == 1024 and precision == 1 and PMC_TRAFFIC is not None))


def roofline(r):
    """the path is MFMA-bound provided activations stay on chip; `achieved` = algorithmic dense-layer
    FLOP of the dominant kernel group (largest share of the step) / its duration, measured live with HIP events
    recorded by the library on the launch stream inside the timed region; `whole_step` = 1.797 GFLOP per
    ray-step x rays/s.  The weight-gradient GEMM streams its operands from HBM (split-K over the samples), so
    its HBM view is kept as a sub-object, with the measured traffic against SURVEY 8(d)'s algorithmic bytes."""
    dom = r['kernels'][r['dominant']]
    tfl = r['value_per_gpu'] * FLOP_PER_RAY_STEP / 1e12
    allk = {k: {kk: round(vv, 4) for kk, vv in v.items() if kk in ('ms', 'tflops', 'gbs')} for k, v in r['kernels'].items()}
    for k in allk:
        allk[k]['frac_of_bf16_mfma_peak'] = round(allk[k]['tflops'] / PEAK_BF16_TFLOPS, 4)
    traffic = PMC_TRAFFIC.get(r['dominant']) if r['pmc_ok'] else None
    dw = r['kernels']['dw_L1']
    step_traffic = sum(PMC_TRAFFIC[k] for k in ('dw_L1', 'mlp_fwd_L1', 'mlp_bwd_L1')) * (1 + 64.0 / 192) if r['pmc_ok'] else None
    # the path's bound is the bf16 MFMA peak for EVERY kernel group, the weight-gradient GEMMs included --
    # that they stream their operands from HBM is this design's choice, not the algorithm's, so the headline is always
    # algorithmic FLOP of the dominant group / its time against 2.5 PFLOP/s; the HBM view of dW stays a sub-object
    head = {'bound': 'mfma', 'achieved': dom['tflops'], 'peak': PEAK_BF16_TFLOPS, 'unit': 'TFLOP/s',
            'frac': dom['tflops'] / PEAK_BF16_TFLOPS}
    # `achieved` counts the REFERENCE's dense MACs; the kernels execute fewer (the folded remap layer): the executed
    # rate is what the matrix pipe actually sustained
    ex = EXEC_OVER_ALGO[{'mlp_fwd_L1': 'mlp_fwd', 'mlp_bwd_L1': 'mlp_bwd', 'dw_L1': 'dw'}[r['dominant']]]
    head.update({'achieved_executed': dom['tflops'] * ex, 'frac_executed': dom['tflops'] * ex / PEAK_BF16_TFLOPS,
                 'kernel': r['dominant'], 'co_dominant_within_2pct': r['co_dominant'], 'traffic': traffic,
                 'launch_ms': dom['ms'], 'traffic_source': PMC_TRAFFIC['source'] if traffic else (PMC_STALE or None)})
    return {**head,
            'whole_step': {'tflops': tfl, 'frac_of_bf16_mfma_peak': tfl / PEAK_BF16_TFLOPS,
                           'hbm_traffic_bytes_per_step': step_traffic,
                           'traffic_over_survey_algorithmic_bytes':
                               (step_traffic / (SURVEY_ALGO_BYTES_PER_RAY * 1024) if step_traffic else None)},
            'all_kernels': allk, 'share_ms_per_step': {k: round(v, 4) for k, v in r['share_ms'].items()},
            # FLOP above are the REFERENCE's dense-layer counts.  The kernels execute fewer: the remap layer
            # (no activation, nerf_network.py:131) is folded into the colour head (csrc/nerfpp_common.h, forward stages)
            'executed_over_algorithmic_macs': {k: round(v, 4) for k, v in EXEC_OVER_ALGO.items()},
            'hbm_view_of_dw': {'bound': 'hbm', 'achieved': dw['gbs'], 'peak': PEAK_HBM_GBS, 'unit': 'GB/s',
                               'frac': dw['gbs'] / PEAK_HBM_GBS, 'operand_bytes_per_row': DW_BYTES_PER_ROW_BF16,
                               'traffic': PMC_TRAFFIC['dw_L1'] if r['pmc_ok'] else None}}


def cpu_baseline(args):
    """oracle/nerfpp_torch_cpu.py -- the path restated as torch-CPU ops + autograd + Adam (validated against the
    pinned numpy oracle in tests/test_oracle_golden.py) -- on the host cores, SURVEY 8(d) protocol: N_rand 1024,
    both levels fwd+bwd+Adam, float32, all host threads, 2 warm-up + 5 timed steps, median."""
    import torch
    from oracle import nerfpp_oracle as O
    from oracle import nerfpp_torch_cpu as TC
    from outdoor_nerf_depth_amd.synthetic import SyntheticKitti
    n = args.cpu_rays
    tc = TC.TorchCpuTrainer(O.init_params_like_reference(2), use_depth=True, depth_loss_type=args.depth_loss_type,
                            lambda_depth=args.lambda_depth)
    scene = SyntheticKitti(depth_sup_type=args.depth_sup_type)
    rng = np.random.RandomState(777)
    times = []
    n_warm, n_timed = 2, 5                        # median of >= 5 steps after 2 warm-ups -- always run in full
    for step in range(n_warm + n_timed):
        b = scene.random_batch(n, rng)
        uni = O.step_uniforms(777, step + 1, n, 64, 128)
        t0 = time.perf_counter()
        tc.train_step(b, uni)
        times.append(time.perf_counter() - t0)
    timed = times[n_warm:]
    t = float(np.median(timed))
    model = 'unknown'
    try:
        for line in open('/proc/cpuinfo'):
            if line.startswith('model name'):
                model = line.split(':', 1)[1].strip()
                break
    except OSError:
        pass
    print('cpu_baseline: %s, nproc=%d, torch threads=%d, s/step %s' %
          (model, os.cpu_count(), torch.get_num_threads(), ['%.2f' % x for x in times]), file=sys.stderr, flush=True)
    return dict(value=n / t, unit='rays/s', cores=torch.get_num_threads(), kind='port', cpu_model=model,
                host_logical_cpus=os.cpu_count(), s_per_step=t, s_per_step_all=[round(x, 3) for x in timed],
                sample='N_rand=%d rays/step, %d warm-up + %d timed steps (median), both levels fwd+bwd+Adam, float32 '
                       'PyTorch-CPU restatement (oracle/nerfpp_torch_cpu.py), torch threads = %d'
                       % (n, n_warm, len(timed), torch.get_num_threads()))


def vendor_gemm(device):
    """What a sustained MFMA-dense kernel gets from THIS socket: torch.mm (hipBLASLt) on bf16 8192^3, 60 launches after 20
    warm-up launches (~70 ms: the clock has settled under the power cap by then).  Context for `roofline.peak`, which is the
    nominal 2.5 PFLOP/s at 2400 MHz; profiles/r06_power_trace.md.  None on any failure."""
    try:
        import torch
        if torch.device(device).type != 'cuda':
            return None
        n = 8192
        x = torch.randn(n, n, device=device, dtype=torch.bfloat16)
        y = torch.randn(n, n, device=device, dtype=torch.bfloat16)
        for _ in range(20):
            torch.mm(x, y)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(60):
            torch.mm(x, y)
        e1.record()
        torch.cuda.synchronize()
        ms = e0.elapsed_time(e1) / 60
        tf = 2.0 * n ** 3 / (ms * 1e-3) / 1e12
        return {'what': 'torch.mm bf16 8192 x 8192 x 8192 (hipBLASLt) on this GPU, 60 launches back to back', 'ms': ms,
                'tflops': tf, 'frac_of_peak': tf / PEAK_BF16_TFLOPS}
    except Exception as e:              # context only: never costs the line
        return {'error': repr(e)}


def render_leg(args, device, precision, label):
    """SURVEY 8 f-2, the inference half of the metric: `render_single_image` (ddp_train_nerf.py:133-249) on one
    375x1242 frame -- deterministic sampling, both cascade levels (64 + 128 samples), fg + bg nets, chunked -- timed as the
    reference runs it (host loop, H2D of the frame's rays, D2H of every output map included), plus the time inside the MLP
    kernels alone from HIP events the library records around them on the launch stream (north_star's ">= 40 % bf16-MFMA
    utilisation in the MLP kernel" is THIS number: the same kernels as training without the saved-tensor stores)."""
    import torch
    from outdoor_nerf_depth_amd.data_loader_split import synthetic_ray_samplers
    from outdoor_nerf_depth_amd.ddp_train_nerf import render_single_image
    from outdoor_nerf_depth_amd.trainer import NerfppTrainer, ALGO_MACS
    sampler = synthetic_ray_samplers('test', 1, 'gt', 20, 375, 1242)[0]
    tr = NerfppTrainer(device, precision=precision, use_depth=False)
    render_single_image(0, 1, tr, sampler, args.render_chunk, keep_dists=False)      # warm-up
    torch.cuda.synchronize()
    taps = []
    t0 = time.perf_counter()
    for _ in range(args.render_frames):
        out = render_single_image(0, 1, tr, sampler, args.render_chunk, keep_dists=False, mlp_events=taps)
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) / args.render_frames
    assert bool(torch.isfinite(out[-1]['rgb']).all()), 'non-finite rendered frame'
    n = sampler.H * sampler.W
    macs = ALGO_MACS['fwd'][0] + ALGO_MACS['fwd'][1]
    lv = {}
    for m in (0, 1):
        ms = sum(b.elapsed_time(e) for (mm, _, b, e) in taps if mm == m) / args.render_frames
        rows = sum(r for (mm, r, _, _) in taps if mm == m) / args.render_frames
        tf = 2.0 * macs * rows / (ms * 1e-3) / 1e12
        lv['mlp_fwd_infer_L%d' % m] = {'ms_per_frame': round(ms, 3), 'rows': int(rows), 'tflops': round(tf, 1),
                                       'frac_of_bf16_mfma_peak': round(tf / PEAK_BF16_TFLOPS, 4)}
    mlp_ms = sum(v['ms_per_frame'] for v in lv.values())
    mlp_tf = n * FLOP_PER_RAY_RENDER / (mlp_ms * 1e-3) / 1e12
    tf = n * FLOP_PER_RAY_RENDER / dt / 1e12
    return {'dtype': label, 'frame': '%dx%d' % (sampler.H, sampler.W), 'chunk': args.render_chunk,
            'frames_timed': args.render_frames, 's_per_frame': dt, 'rays_per_s': n / dt, 'algorithmic_tflops': tf,
            'frac_of_bf16_mfma_peak': tf / PEAK_BF16_TFLOPS,
            'mlp_kernels': {'ms_per_frame': round(mlp_ms, 3), 'tflops': round(mlp_tf, 1),
                            'frac_of_bf16_mfma_peak': round(mlp_tf / PEAK_BF16_TFLOPS, 4), **lv},
            'note': 's_per_frame is the whole render_single_image call (host loop, H2D of rays, D2H of 7 output maps per '
                    'level); mlp_kernels is HIP-event time inside the MLP launches only (executed MFMA work is 3x the '
                    'algorithmic figure in split-bf16)'}


class PowerSampler(object):
    """Socket power and shader clock (amdgpu hwmon files of the PCI device HIP device 0 sits on) sampled every 50 ms by a thread
    while a leg runs: the MLP kernels hold the socket at its power cap with the clock throttled (profiles/r06_power_trace.md), and a
    box with a different cap or clock shows up here.  Never raises: `summary()` is None where the files are not readable."""

    def __init__(self):
        import threading
        self.files, self.rows, self.on, self.thread = {}, [], False, None
        try:
            import ctypes
            import glob
            hip = ctypes.CDLL('libamdhip64.so')
            buf = ctypes.create_string_buffer(64)
            if hip.hipDeviceGetPCIBusId(buf, 64, 0) != 0:
                return
            self.pci = buf.value.decode().lower()
            for d in sorted(glob.glob('/sys/bus/pci/devices/%s/hwmon/hwmon*' % self.pci)):
                for key, name in (('power_uw', 'power1_input'), ('power_uw', 'power1_average'), ('cap_uw', 'power1_cap'), ('sclk_hz', 'freq1_input')):
                    f = os.path.join(d, name)
                    if key not in self.files and os.path.exists(f):
                        self.files[key] = f
            if 'power_uw' in self.files:
                self.thread = threading.Thread(target=self._run, daemon=True)
        except Exception:
            self.files, self.thread = {}, None

    def _run(self):
        while self.on:
            row = {}
            for k, f in self.files.items():
                try:
                    with open(f) as fh:
                        row[k] = int(fh.read())
                except Exception:
                    pass
            self.rows.append((time.perf_counter(), row))
            time.sleep(0.05)

    def __enter__(self):
        if self.thread is not None:
            self.on = True
            self.thread.start()
        return self

    def __exit__(self, *exc):
        self.on = False
        if self.thread is not None:
            self.thread.join(timeout=2.0)
        return False

    def summary(self, t_from, t_to):
        """mean over the samples taken in [t_from, t_to] (time.perf_counter())"""
        rows = [r for t, r in self.rows if t_from <= t <= t_to]
        if not rows:
            return None
        out = {'samples': len(rows), 'pci': getattr(self, 'pci', None)}
        for k, name, div in (('power_uw', 'socket_w', 1e6), ('cap_uw', 'cap_w', 1e6), ('sclk_hz', 'sclk_mhz', 1e6)):
            v = [r[k] for r in rows if k in r]
            if v:
                out[name] = round(float(np.mean(v)) / div, 1)
                if k != 'cap_uw':
                    out[name + '_max'] = round(float(np.max(v)) / div, 1)
        return out


def cli_loop(args, kernel_only_ms):
    """the drop-in loop itself -- `ddp_train_nerf()` of outdoor_nerf_depth_amd/ddp_train_nerf.py
    (reference: ddp_train_nerf.py:417-431 per-step frame choice + random_sample + H2D, here device_sampler.py +
    nerfpp_gather_rays; log line every i_print = 100 steps) on the KITTI-shaped scene (375x1242 frames), bf16, gt / mse / 0.1
    -- once with the device sampler (default) and once with the reference's host sampler (--host_sampling).  ms per step =
    the loop's own `iter_time` (wall time between log lines / steps; the log line reads the scalars, i.e. synchronises),
    averaged over the log lines after step 200; `kernel_only_ms` = the headline's ms_per_step (pre-staged device batches)."""
    import logging
    import re
    import shutil
    import tempfile
    from outdoor_nerf_depth_amd import ddp_train_nerf as C

    class Cap(logging.Handler):
        def __init__(self):
            logging.Handler.__init__(self)
            self.rows, self.at = [], {}

        def emit(self, record):
            m = re.search(r'step: (\d+) .* iter_time: ([0-9.eE+-]+)', record.getMessage())
            if m:
                self.rows.append((int(m.group(1)), float(m.group(2))))
                self.at[int(m.group(1))] = time.perf_counter()

    import torch
    out = {'steps': args.cli_steps, 'i_print': 100,
           'scene': 'synthetic KITTI-shaped, %d frames of 375x1242 (BASELINE config 2: 295 incl. the held-out tenth), N_rand %d' % (args.cli_frames, args.n_rand),
           'kernel_only_ms_per_step': kernel_only_ms,
           'note': 'the step slows by 2-3 % over the first 1000 steps of a run (the clock follows the operand statistics of the '
                   'training network), so the loop is compared with the kernel-only step measured on ITS OWN trainer right '
                   'after the last loop step (pre-staged batches, 200 steps): overhead_pct; overhead_vs_fresh_pct is against '
                   "the headline's fresh-network window"}
    same_state = {}

    def on_finish(trainer, samplers):
        # the kernel-only step on the state the loop ended in: pre-staged device batches, no sampling, no log line
        from outdoor_nerf_depth_amd.trainer import batch_to_device
        if hasattr(samplers, 'random_sample'):
            staged = [samplers.random_sample(args.n_rand) for _ in range(32)]
        else:
            staged = [batch_to_device(samplers[i % len(samplers)].random_sample(args.n_rand), trainer.device) for i in range(32)]
        for i in range(20):
            trainer.train_step(staged[i % 32])
        trainer.flush()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for i in range(200):
            trainer.train_step(staged[i % 32])
        trainer.flush()
        torch.cuda.synchronize()
        same_state['ms'] = 1e3 * (time.perf_counter() - t0) / 200
    # (the loop in the CLI's DEFAULT precision too -- split-bf16 since round 5, 0.4x the bf16 rate: what a user who passes no
    # --precision gets)
    for name, extra in (('device_sampler', []), ('host_sampler', ['--host_sampling']), ('device_sampler_default_precision', ['--precision', 'split'])):
        tmp = tempfile.mkdtemp(prefix='nerfpp_cli_')
        cap = Cap()
        power = None
        C.setup_logger()
        lg = logging.getLogger(C.__package__ or 'outdoor_nerf_depth_amd')
        lg.addHandler(cap)
        level = lg.level
        try:
            a = C.config_parser().parse_args(
                ['--expname', 'bench', '--basedir', tmp, '--synthetic', '--synthetic_frames', str(args.cli_frames), '--world_size', '1',
                 '--cascade_samples', '64,128', '--N_rand_override', str(args.n_rand), '--N_iters', str(args.cli_steps),
                 '--i_print', '100', '--i_weights', '100000000', '--i_test', '100000000'] + ([] if '--precision' in extra else ['--precision', 'bf16']) + ['--use_depth',
                 '--depth_sup_type', args.depth_sup_type, '--depth_loss_type', args.depth_loss_type,
                 '--lambda_depth', str(args.lambda_depth)] + extra)
            C.validate_args(a)
            a.world_size = 1
            a.on_finish = on_finish
            same_state.clear()
            with PowerSampler() as ps:
                C.ddp_train_nerf(0, a)
            marks = sorted(st for st in cap.at if st >= 300)            # the log lines of steps 300 ... last: the steps `late` averages
            power = ps.summary(cap.at[marks[0]], cap.at[marks[-1]]) if len(marks) >= 2 else None
        finally:
            lg.removeHandler(cap)
            lg.setLevel(level)
            shutil.rmtree(tmp, ignore_errors=True)
        late = [t for (st, t) in cap.rows if st > 200 and st % 100 == 0]
        if not late:
            out[name] = None
            continue
        ms = 1e3 * float(np.mean(late[-4:]))          # the last 400 steps: the state the same-state reference is taken in
        ref = same_state.get('ms')
        out[name] = {'ms_per_step': ms, 'rays_per_s': args.n_rand / (ms * 1e-3), 'log_lines_averaged': len(late[-4:]),
                     'ms_per_step_by_log_line': [round(1e3 * t, 4) for t in late],
                     'kernel_only_same_state_ms': ref,
                     'overhead_pct': None if ref is None else 100.0 * (ms / ref - 1.0),
                     'overhead_vs_fresh_pct': None if 'default_precision' in name else 100.0 * (ms / kernel_only_ms - 1.0),
                     'power': power}
    return out


def second_transport(args, L, rank, world, device, batches, out):
    """--grad_comm both: the timed bf16 steps once more with the gradient all-reduce going through the library's own RCCL entry
    point (nerfpp_allreduce_mean on a communicator of its own).  A failure or a hang here must not cost the scaling run its
    torch.distributed number: errors are reported in config.grad_comm_rccl_abi, and a watchdog on EVERY rank ends the process
    (rank 0 after printing the line it already has) if the phase has not finished in NERFPP_BENCH_ABI_TIMEOUT_S (default 180 s)."""
    import threading

    def bail():
        if out is not None:
            out['config']['grad_comm_rccl_abi'] = {'error': 'timed out (watchdog): the rccl_abi transport did not finish'}
            print(json.dumps(out), flush=True)
        os._exit(0)
    dog = threading.Timer(float(os.environ.get('NERFPP_BENCH_ABI_TIMEOUT_S', '180')), bail)
    dog.daemon = True
    dog.start()
    result = None
    comm = None
    try:
        from outdoor_nerf_depth_amd.dist_utils import RcclComm
        comm = RcclComm(rank, world)
        r = run_mode(args, L.PREC_BF16, rank, world, device, batches, comm=comm)
        result = {'value': r['value'], 'ms_per_step': r['ms_per_step'], 'per_rank_ms_per_step': r['per_rank_ms_per_step'],
                  'exposed_update_ms_per_step': r['exposed_update_ms_per_step'], 'allreduce_ms': r['allreduce_ms']}
    except Exception as e:                           # noqa: BLE001 (reported in the JSON line)
        result = {'error': '%s: %s' % (type(e).__name__, e)}
    finally:
        if comm is not None:
            try:
                comm.destroy()
            except Exception:                        # noqa: BLE001
                pass
        dog.cancel()
    if out is not None:
        out['config']['grad_comm_rccl_abi'] = result


def _channels_in_effect():
    from outdoor_nerf_depth_amd.dist_utils import rccl_channels_in_effect
    return rccl_channels_in_effect()


def main():
    args = parse()
    env_world = os.environ.get('WORLD_SIZE')
    if env_world is None and args.gpus > 1:
        spawn_ranks(args.gpus)
        return
    import torch
    rank = int(os.environ.get('RANK', '0'))
    world = int(env_world or '1')
    local = int(os.environ.get('LOCAL_RANK', '0'))
    if world != args.gpus:
        raise SystemExit('bench.py: --gpus %d but WORLD_SIZE=%d' % (args.gpus, world))
    assert torch.cuda.is_available(), 'bench.py needs a GPU: the NeRF++ hot path has no CPU fallback'
    # test hooks: NERFPP_SHARE_GPU=1 puts every rank on cuda:0 and NERFPP_DIST_BACKEND=gloo replaces RCCL,
    # so the N > 1 code path can be smoke-tested on a 1-GPU box (numbers from such a run mean nothing)
    share = bool(os.environ.get('NERFPP_SHARE_GPU'))
    if share:
        local = 0
    elif local >= torch.cuda.device_count():
        raise SystemExit('bench.py: rank %d wants cuda:%d but only %d GPU(s) are visible' %
                         (rank, local, torch.cuda.device_count()))
    backend = os.environ.get('NERFPP_DIST_BACKEND', 'nccl')
    device = torch.device('cuda', local)
    torch.cuda.set_device(device)
    if world > 1:
        import torch.distributed as dist
        os.environ.setdefault('MASTER_ADDR', '127.0.0.1')
        for k, v in rccl_env_defaults(args.rccl_channels).items():          # (under torchrun: before the communicator exists)
            os.environ.setdefault(k, v)
        if backend == 'nccl':
            dist.init_process_group('nccl', rank=rank, world_size=world, device_id=device)
        else:
            dist.init_process_group(backend, rank=rank, world_size=world)
        assert dist.get_world_size() == args.gpus

    from outdoor_nerf_depth_amd.synthetic import SyntheticKitti
    from outdoor_nerf_depth_amd.trainer import batch_to_device
    from outdoor_nerf_depth_amd import _lib as L
    scene = SyntheticKitti(depth_sup_type=args.depth_sup_type)
    rng = np.random.RandomState((rank + 1) * 777)                 # ddp_train_nerf.py:406
    torch.manual_seed((rank + 1) * 777)                           # :408
    batches = [batch_to_device(scene.random_batch(args.n_rand, rng), device)
               for _ in range(args.steps + args.warmup)]

    res = {}
    dump = {} if args.dump_outputs else None            # filled by the headline run: bf16 when it runs, else split
    if world > 1 and args.precision == 'both':
        args.precision = 'bf16'                  # the scaling runs measure the headline precision only
    abi_second = False                       # --grad_comm both: the library's own RCCL entry point as a SECOND run, last of all
    if args.precision in ('both', 'bf16'):
        want = args.grad_comm if (world > 1 and backend == 'nccl') else 'torch'
        if want == 'rccl_abi':
            from outdoor_nerf_depth_amd.dist_utils import RcclComm
            comm = RcclComm(rank, world)
            res['bf16'] = run_mode(args, L.PREC_BF16, rank, world, device, batches, comm=comm, outputs=dump)
            comm.destroy()
        else:
            res['bf16'] = run_mode(args, L.PREC_BF16, rank, world, device, batches, outputs=dump)
            # (test hook: NERFPP_BENCH_FORCE_ABI_SECOND=1 runs the second-transport phase over gloo on a shared GPU too -- RCCL
            # refuses two ranks on one device, so what that exercises is the phase's failure and watchdog paths)
            abi_second = args.full and (want == 'both' or (world > 1 and bool(os.environ.get('NERFPP_BENCH_FORCE_ABI_SECOND'))))
    if args.precision == 'split' or (args.precision == 'both' and args.full):
        res['split'] = run_mode(args, L.PREC_SPLIT_BF16, rank, world, device, batches,
                                outputs=None if 'bf16' in res else dump)
    m360 = None
    if world > 1 and args.full and args.mip360_rays > 0:
        # BASELINE configs[4] is an 8-GPU configuration: the MipNeRF-360 step data-parallel over the same ranks
        # (per-rank rays, gradients averaged over RCCL); every rank takes part, rank 0 reports
        from outdoor_nerf_depth_amd import mip360
        m360 = mip360.benchmark_step(device, args.mip360_rays, steps=5, warmup=2, seed=rank, world_size=world)
    if rank != 0:
        if world > 1:
            if abi_second:
                second_transport(args, L, rank, world, device, batches, None)
            dist.destroy_process_group()
        return
    if dump is not None:
        os.makedirs(args.dump_outputs, exist_ok=True)
        for k, v in dump.items():
            np.save(os.path.join(args.dump_outputs, k + '.npy'), v)
    main_key = 'bf16' if 'bf16' in res else 'split'
    r = res[main_key]
    out = {
        'metric': 'train rays/sec, KITTI 375x1242, 64+128 samples/ray',
        'value': r['value'], 'unit': 'rays/s', 'n_gpus': world, 'steps': args.steps, 'warmup': args.warmup,
        'ms_per_step': r['ms_per_step'], 'higher_is_better': True, 'scaling': 'weak', 'vs_baseline': None,
        'dtype': 'bf16 MFMA operands, f32 accumulate / f32 master weights' if main_key == 'bf16'
                 else 'split-bf16 (hi+lo, 3 MFMA passes), f32 accumulate',
        'data': 'synthetic',
        'config': {'workload': 'NeRF++ KITTI seq00-shaped (295 fr, 375x1242), depth_sup_type=%s, '
                               'depth_loss_type=%s, lambda_depth=%g, N_rand=%d rays/GPU/step, cascade 64+128, '
                               'both levels fwd+bwd+Adam' % (args.depth_sup_type, args.depth_loss_type,
                                                             args.lambda_depth, args.n_rand),
                   'n_rand_per_gpu': args.n_rand, 'parallelism': 'dp%d (ray batches, RCCL grad all-reduce)' % world,
                   'setup_steps': SETUP_STEPS,
                   'dist_backend': (('%s, %s' % (backend, ' '.join('%s=%s' % (k, os.environ.get(k)) for k in ('NCCL_MAX_NCHANNELS', 'NCCL_MIN_NCHANNELS'))))
                                    if world > 1 else None),
                   # N > 1 diagnostics: each rank's own clock over the timed steps (ms per step, before the closing
                   # barrier) and the time per step its main stream waited for the side-stream parameter update (slab
                   # sum -> all-reduce -> Adam -> re-pack) that the next level's forward did not hide
                   'per_rank_ms_per_step': r['per_rank_ms_per_step'],
                   'exposed_update_ms_per_step': r['exposed_update_ms_per_step'],
                   # ... the duration of the 4.81 MB gradient all-reduce of each cascade level on every rank (ms, median over the
                   # timed steps; HIP events on the stream it is issued on), the transport it went through, and the channel counts
                   # RCCL's own INIT log reports for the communicators of rank 0 (null: gloo, or NCCL_DEBUG set by the caller)
                   'grad_comm': (None if world == 1 else 'rccl_abi' if (args.grad_comm == 'rccl_abi' and backend == 'nccl') else 'torch'),
                   'allreduce_ms': r['allreduce_ms'],
                   'rccl_channels_in_effect': _channels_in_effect() if world > 1 else None,
                   'grad_comm_rccl_abi': None},        # (--grad_comm both: filled in by second_transport() below)
        'roofline': roofline(r),
        'final_loss': r['loss'],
        'gates': {
            'value (bf16)': 'tests/test_gpu_parity.py bf16 gates: outputs / gradients within 2x the measured bf16 error '
                            'of profiles/r02_bf16_error_report.json and within bf16-grade bounds of the oracle run with '
                            'bf16-rounded GEMM operands; NOT the 1e-4 gate; PSNR: profiles/r01_n_* (paired gap '
                            '-0.10 +- 0.53 dB, synthetic scene)',
            'parity_forward_mode': 'rendered RGB / depth / loss within 1e-4 relative of the float32 reference '
                                   '(same forward kernels as parity_mode); gradients bf16-grade',
            'parity_mode': '1e-4 relative on RGB / depth / weights / loss, integer bins bit-exact, gradients within '
                           '5e-2 RMS of the float64 reference (tests/test_gpu_parity.py)',
        },
    }
    if not args.full:
        print(json.dumps(out), flush=True)
        if world > 1:
            dist.destroy_process_group()
        return
    # --full: the legs below run after the headline run and only add to the line; the headline's own fields stay as they are
    if world == 1:
        out['roofline']['vendor_gemm_same_socket'] = vendor_gemm(device)
    if world == 1 and args.precision == 'both':
        # split-bf16 forward (rendered RGB / depth / loss within 1e-4 of float32) + bf16 backward over its hi planes
        h = run_mode(args, L.PREC_SPLIT_FWD, rank, world, device, batches)
        out['parity_forward_mode'] = {'dtype': 'split-bf16 forward (outputs and loss at 1e-4), bf16 backward / weight gradients',
                                      'value': h['value'], 'ms_per_step': h['ms_per_step']}
        h3 = run_mode(args, L.PREC_FP16_FWD, rank, world, device, batches)
        out['fp16_forward_mode'] = {'dtype': 'fp16x2w forward (weights hi + lo in fp16, activations rounded once, 2 MFMA passes), bf16 backward / '
                                             'weight gradients; outputs within 1e-4 of float32 at initialisation, 3-4e-4 on trained weights '
                                             '(tests/test_gpu_round5.py): an intermediate precision, NOT a carrier of the 1e-4 clause',
                                    'value': h3['value'], 'ms_per_step': h3['ms_per_step']}
    if 'split' in res and main_key != 'split':
        s = res['split']
        out['parity_mode'] = {'dtype': 'split-bf16 (hi+lo, 3 MFMA passes): the precision the 1e-4 parity tests use',
                              'value': s['value'], 'ms_per_step': s['ms_per_step'],
                              'roofline': roofline(s)}
    if world == 1 and args.large_batch > 0 and main_key == 'bf16':
        # "report at N_rand=1024 (reference value) and at the largest N_rand that fits, labelled"
        import copy
        a2 = copy.copy(args)
        a2.n_rand, a2.steps, a2.warmup = args.large_batch, 5, 2
        b2 = [batch_to_device(scene.random_batch(a2.n_rand, rng), device) for _ in range(a2.steps + a2.warmup)]
        r2 = run_mode(a2, L.PREC_BF16, rank, world, device, b2)
        out['large_batch'] = {'n_rand_per_gpu': a2.n_rand, 'value': r2['value'], 'unit': 'rays/s',
                              'ms_per_step': r2['ms_per_step'], 'steps': a2.steps,
                              'note': 'same workload at a larger ray batch than the 1024 of the reference (labelled, not the headline)'}
    if world == 1 and args.mip360_rays > 0:
        # BASELINE configs[4], labelled extra: the MipNeRF-360 step on its own library (libmip360_hip.so)
        from outdoor_nerf_depth_amd import mip360
        out["config5_mip360"] = mip360.benchmark_step(device, args.mip360_rays, steps=10, warmup=3)
    elif m360 is not None:
        out['config5_mip360'] = m360
    if world == 1 and args.render_frames > 0:
        out['render'] = {'metric': 'render rays/sec, one 375x1242 frame, 64+128 samples/ray, deterministic sampling '
                                   '(render_single_image, ddp_train_nerf.py:133-249)',
                         'bf16': render_leg(args, device, L.PREC_BF16, 'bf16 MFMA operands, f32 accumulate')}
        if args.precision == 'both':
            out['render']['split_bf16'] = render_leg(args, device, L.PREC_SPLIT_BF16, 'split-bf16 (hi+lo, 3 MFMA passes): 1e-4 parity mode')
    if world == 1 and args.cli_steps >= 300 and main_key == 'bf16':
        out['cli_loop'] = cli_loop(args, r['ms_per_step'])
        d = out['cli_loop'].get('device_sampler')
        if d:
            # what a user of the drop-in loop gets: per-step frame choice, on-device pixel draw and ray
            # gather, log lines -- on a network that has trained for cli_steps steps, not the headline's fresh-network window
            out['end_to_end'] = {'value': d['rays_per_s'], 'unit': 'rays/s', 'ms_per_step': d['ms_per_step'],
                                 'what': 'outdoor_nerf_depth_amd.ddp_train_nerf.ddp_train_nerf(), bf16, %d frames, device sampler, '
                                         'mean over the last 400 of %d steps' % (args.cli_frames, args.cli_steps)}
            out['trained_state_ms'] = d['kernel_only_same_state_ms']
            # (also inside `config`, one of the objects the driver's record echoes as a whole: VERDICT r05 item 8)
            out['config']['end_to_end'] = dict(out['end_to_end'])
            if d.get('power'):
                # socket power / shader clock while that loop ran (hwmon): the kernels hold the socket at its cap, the clock gives way
                out['power'] = dict(d['power'], during='the end_to_end loop (bf16), between its log lines of step 300 and of the last step',
                                    default_precision_loop=(out['cli_loop'].get('device_sampler_default_precision') or {}).get('power'))
                out['config']['power'] = {k: out['power'].get(k) for k in ('socket_w', 'cap_w', 'sclk_mhz')}
        d2 = out['cli_loop'].get('device_sampler_default_precision')
        if d2:
            out['end_to_end_default_precision'] = {'value': d2['rays_per_s'], 'unit': 'rays/s', 'ms_per_step': d2['ms_per_step'],
                                                   'what': 'the same loop with the CLI default --precision split (split-bf16 everywhere: '
                                                           'outputs, loss and gradients at float32 grade)'}
            out['config']['end_to_end_default_precision'] = dict(out['end_to_end_default_precision'])
    if world == 1 and not args.no_cpu_baseline:
        out['cpu_baseline'] = cpu_baseline(args)
    if world > 1 and abi_second:
        # everything the line needs is in `out`; the second transport has never run on more than one GPU (no box in six rounds),
        # so it runs LAST and under a watchdog: should it hang, every rank abandons it and rank 0 still prints the line
        second_transport(args, L, rank, world, device, batches, out)
    print(json.dumps(out), flush=True)
    if world > 1:
        dist.destroy_process_group()


if __name__ == '__main__':
    main()

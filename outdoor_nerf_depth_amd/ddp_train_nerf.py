#!/usr/bin/env python
"""Drop-in entry point for nerf-methods/nerfplusplus/ddp_train_nerf.py on MI355X.

    python -m outdoor_nerf_depth_amd.ddp_train_nerf --config configs/kitti.txt \
        --use_depth --depth_sup_type gt --depth_loss_type mse --lambda_depth 0.1 --trainskip 4 ...

Same flags and defaults as the reference's `config_parser` (:657-727), same outputs under
{basedir}/{expname}/ (args.txt, config.txt, model_{step:06d}.pth with the reference's state-dict
keys, render_test_{step:06d}/ + psnr_/rmse_/absrel_*.txt), same log scalars
(`level_m/{rgb_loss,pnsr,loss_depth}`, `iter_time`, `resolution`).  The per-step work runs on the
HIP library (trainer.py); one process per GPU, RCCL all-reduce of the flat gradients.

Extra flags: --sample_every (the README's name for --trainskip), --precision {split,fp16_fwd,split_fwd,bf16},
--synthetic (KITTI-shaped procedural scene instead of --datadir), --N_rand_override.
With --depth_metrics every test render also gets depth_{name}_{step:06d}.txt: the whole KITTI depth-metric set (n_valid, rmse,
absrel, sqrel, absdiff, rmse_log, a1, a2, a3) of the frames that have ground-truth depth, in one device call (depth_metrics.py).
"""
import argparse
import logging
import os
import sys
import time
from collections import OrderedDict

import numpy as np

from . import depth_losses as DL
from . import depth_prior_stages as PS
from . import eval_outputs as EO
from .depth_metrics import DEPTH_METRICS_HELP
from .eval_outputs import load_lpips_weights

logger = logging.getLogger(__package__ or 'outdoor_nerf_depth_amd')
TINY_NUMBER = 1e-6
mse2psnr = lambda x: -10. * np.log(x + TINY_NUMBER) / np.log(10.)           # utils.py:31
to8b = lambda x: (255 * np.clip(x, 0, 1)).astype(np.uint8)


def setup_logger():
    lg = logging.getLogger(__package__ or 'outdoor_nerf_depth_amd')
    lg.setLevel(logging.INFO)
    if not lg.handlers:
        ch = logging.StreamHandler()
        ch.setFormatter(logging.Formatter('%(asctime)s [%(levelname)s] %(name)s: %(message)s'))
        lg.addHandler(ch)


class ConfigFileParser(argparse.ArgumentParser):
    """argparse + the config file syntax of configargparse's default parser (--config; the command line
    wins): one `key = value`, `key: value` or `key value` per line, `#` / `;` comments, a bare `key` or
    `key = true` for store_true flags.  Unknown keys are an error, like upstream."""

    @staticmethod
    def _split(line):
        for sep in ('=', ':'):
            if sep in line:
                k, v = line.split(sep, 1)
                if ' ' not in k.strip():
                    return k.strip(), v.strip()
        parts = line.split(None, 1)
        return parts[0], (parts[1].strip() if len(parts) > 1 else None)

    def parse_args(self, args=None, namespace=None):
        args = list(sys.argv[1:] if args is None else args)
        cfg = None
        for i, a in enumerate(args):
            if a == '--config' and i + 1 < len(args):
                cfg = args[i + 1]
            elif a.startswith('--config='):
                cfg = a.split('=', 1)[1]
        file_args = []
        if cfg and cfg != 'None':
            known = {}
            for a in self._actions:
                for opt in a.option_strings:
                    known[opt.lstrip('-')] = a
            for ln, raw in enumerate(open(cfg), 1):
                line = raw.strip()
                if not line or line[0] in '#;' or line.startswith('---'):
                    continue
                line = line.split(' #', 1)[0].strip()
                k, v = self._split(line)
                k = k.lstrip('-')
                if k == 'config':
                    continue
                if k not in known:
                    self.error('%s:%d: unrecognized config key %r' % (cfg, ln, k))
                if v is not None and len(v) >= 2 and v[0] == v[-1] and v[0] in '"\'':
                    v = v[1:-1]
                act = known[k]
                if isinstance(act, argparse._StoreTrueAction):
                    if v is None or v.lower() in ('true', '1', 'yes', 'on'):
                        file_args.append('--' + k)
                    elif v.lower() not in ('false', '0', 'no', 'off'):
                        self.error('%s:%d: flag %r takes true/false, got %r' % (cfg, ln, k, v))
                elif v is None:
                    self.error('%s:%d: key %r needs a value' % (cfg, ln, k))
                elif v != 'None':
                    file_args += ['--' + k, v]
        return super().parse_args(file_args + args, namespace)


def config_parser():
    """Flag for flag the reference's parser (ddp_train_nerf.py:657-727)."""
    p = ConfigFileParser()
    p.add_argument('--config', type=str, default=None, help='config file path')
    p.add_argument('--expname', type=str, help='experiment name')
    p.add_argument('--basedir', type=str, default='./logs/', help='where to store ckpts and logs')
    p.add_argument('--datadir', type=str, default=None, help='input data directory')
    p.add_argument('--scene', type=str, default=None, help='scene name')
    p.add_argument('--testskip', type=int, default=8)
    p.add_argument('--trainskip', '--sample_every', dest='trainskip', type=int, default=1,
                   help='will load 1/N images from train sets for sparse inputs')
    p.add_argument('--netdepth', type=int, default=8)
    p.add_argument('--netwidth', type=int, default=256)
    p.add_argument('--use_viewdirs', action='store_true')
    p.add_argument('--no_reload', action='store_true')
    p.add_argument('--ckpt_path', type=str, default=None)
    p.add_argument('--N_rand', type=int, default=32 * 32 * 2)
    p.add_argument('--chunk_size', type=int, default=1024 * 8)
    p.add_argument('--N_iters', type=int, default=250001)
    p.add_argument('--render_splits', type=str, default='test')
    p.add_argument('--cascade_level', type=int, default=2)
    p.add_argument('--cascade_samples', type=str, default='64,64')
    p.add_argument('--world_size', type=int, default=-1)
    p.add_argument('--optim_autoexpo', action='store_true')
    p.add_argument('--lambda_autoexpo', type=float, default=1.)
    p.add_argument('--lrate', type=float, default=5e-4)
    p.add_argument('--lrate_decay_factor', type=float, default=0.1)      # parsed, never read (as upstream)
    p.add_argument('--lrate_decay_steps', type=int, default=5000)        # parsed, never read
    p.add_argument('--det', action='store_true')                         # parsed, never read
    p.add_argument('--max_freq_log2', type=int, default=10)
    p.add_argument('--max_freq_log2_viewdirs', type=int, default=4)
    p.add_argument('--load_min_depth', action='store_true')
    p.add_argument('--i_print', type=int, default=100)
    p.add_argument('--i_img', type=int, default=500)                     # parsed, never read
    p.add_argument('--i_weights', type=int, default=10000)
    p.add_argument('--use_depth', action='store_true')
    p.add_argument('--lambda_depth', type=float, default=1.0)
    p.add_argument('--depth_loss_type', choices=['mse', 'kl', 'los', 'l1', 'nll', 'ssi', 'gnll'], default='mse',
                   help="mse / l1 / kl as the reference; ssi (an addition of this implementation): the scale-and-shift-invariant loss "
                        'for relative-depth priors such as --depth_sup_type mono_crop -- per batch (one frame per rank) the scale and '
                        'shift that best map the rendered depth onto the prior are fitted, and what is left is penalised; gnll (an '
                        'addition too): the Gaussian negative log-likelihood for priors with a per-pixel standard deviation, read from '
                        "{split}/depth[_<sup_type>]_std/ (encoded like the prior) or --depth_gnll_std -- a ray is penalised only while "
                        'its rendering lies outside what the prior expects')
    p.add_argument('--depth_sup_type', type=str, default='gt')
    p.add_argument('--depth_sigma', type=float, default=0.01)
    p.add_argument('--port', type=int, default=12345)
    # --- additions of this implementation
    p.add_argument('--depth_ssi_min_rays', type=int, default=8,
                   help='--depth_loss_type ssi: a batch with fewer supervised rays than this is not fitted and earns no depth loss')
    p.add_argument('--depth_gnll_std', type=float, default=0.0,
                   help='--depth_loss_type gnll: the standard deviation of the prior in metres at every pixel, used when the scene has '
                        'no depth[_<sup_type>]_std/ folder; 0 (default) = the folder is required')
    p.add_argument('--lambda_distortion', type=float, default=0.0,
                   help="weight of a distortion loss (MipNeRF-360's, on the sample intervals normalised to [min_depth, far]) on the "
                        'foreground weights of every cascade level: it pulls the weight along a ray together, against floaters where '
                        'no depth prior speaks.  0 (default) = off')
    p.add_argument('--lambda_opacity', type=float, default=0.0,
                   help='weight of the entropy -o log o of the foreground opacity o = sum of the foreground weights, on every cascade '
                        'level: it pushes a ray to be foreground or background rather than a blend.  0 (default) = off')
    p.add_argument('--depth_guide_samples', type=int, default=0,
                   help='this many of the new foreground samples of the second cascade level are drawn from a Gaussian around the depth '
                        "prior, truncated at three standard deviations, instead of from the first level's weights (Roessle et al., Dense "
                        'Depth Priors for NeRF), whatever the depth loss is; a ray without a prior, and every ray of a render, draws them '
                        'around the depth and spread the first level rendered.  The standard deviation is read like gnll\'s, from '
                        '{split}/depth[_<sup_type>]_std/ or a depth-prior stage, else --depth_guide_std.  Pass the same value to '
                        'ddp_test_nerf.  0 (default) = off')
    p.add_argument('--depth_guide_std', type=float, default=0.0,
                   help='--depth_guide_samples: the standard deviation of the prior in metres at every pixel, used when the training '
                        'frames carry no map; it must then be positive')
    p.add_argument('--depth_guide_min_std', type=float, default=0.0,
                   help='--depth_guide_samples: a floor in metres under the standard deviation of the Gaussian')
    p.add_argument('--lambda_los', type=float, default=0.0,
                   help="weight of Urban Radiance Fields' line-of-sight term on the foreground weights of every cascade level, beside "
                        'the depth loss (needs --use_depth and a metric prior, so not --depth_loss_type ssi): on a ray with a prior it '
                        'empties the space in front of the band prior +- sigma and pulls the weight inside the band to a narrow Gaussian '
                        'around the prior, against floaters that an expected-depth loss cannot see.  sigma comes from --los_sigma or '
                        '--los_sigma_std_mult.  The term is a mean over all rays of a batch, so a sparse prior wants a large weight (10 .. '
                        '100 on the synthetic scene, whose prior covers 5 %% of the pixels).  0 (default) = off')
    p.add_argument('--los_sigma', type=float, default=0.0,
                   help='--lambda_los: the half-width of the band around the prior in metres, at every pixel; about one sample interval '
                        'at the prior is a good start.  Needed unless --los_sigma_std_mult is positive')
    p.add_argument('--los_sigma_std_mult', type=float, default=0.0,
                   help="--lambda_los: positive = the half-width is this many standard deviations of the prior, read like gnll's from "
                        '{split}/depth[_<sup_type>]_std/ or a depth-prior stage; the run exits if the training frames carry none.  '
                        '0 (default) = --los_sigma')
    p.add_argument('--los_min_sigma', type=float, default=0.0,
                   help='--lambda_los: a floor in metres under the half-width of the band')
    p.add_argument('--los_sigma_decay', type=float, default=1.0,
                   help="--lambda_los: URF's annealing of the band: the half-width is multiplied by this factor ** (min(step, "
                        '--los_sigma_decay_steps) / --los_sigma_decay_steps), so it reaches the factor after that many steps and stays')
    p.add_argument('--los_sigma_decay_steps', type=int, default=0,
                   help='--lambda_los: the steps over which --los_sigma_decay is reached; 0 (default) = no annealing')
    PS.add_flags(p)                              # (host side only: a stage's binding and library are loaded by a run that asks for it)
    p.add_argument('--precision', choices=['bf16', 'split', 'split_fwd', 'fp16_fwd'], default='split',
                   help='MLP arithmetic.  split (default): split-bf16 (3 MFMA passes) in forward, backward and weight gradients -- '
                        'rendered RGB / depth / loss within 1e-4 of the float32 reference, gradients at float32 grade.  split_fwd: '
                        'that forward with the single-pass bf16 backward (1.6x the throughput).  fp16_fwd: forward with fp16 '
                        'operands, weights hi + lo (2 passes: 1e-4 at initialisation, 3-4e-4 on trained weights), bf16 backward '
                        '(2.3x).  bf16: single-pass bf16 MFMA everywhere (fastest; outputs at bf16 grade, 1e-2).  With a bf16 backward a '
                        "training run leaves the reference's trajectory like the reference's own float64 run leaves its float32 "
                        'run: rgb-only within 0.01 dB at step 200, with a depth term +-0.2 ... 0.9 dB at step 200 in either '
                        'direction and no resolvable gap (|median| < 0.1 dB over seeds) at 1000 steps: DESIGN.md section 5')
    p.add_argument('--grad_comm', choices=['torch', 'rccl_abi'], default='torch',
                   help="gradient all-reduce: torch.distributed (backend nccl = RCCL), or the library's own RCCL entry point "
                        '(nerfpp_allreduce_mean; the communicator id travels over the torch process group)')
    p.add_argument('--rccl_channels', type=int, default=-1,
                   help='cap on the RCCL channels of the gradient all-reduce (NCCL_MAX_NCHANNELS; every channel holds a CU that an '
                        'MLP tile cannot use).  -1 (default): 4 when all ranks run on one node, RCCL\'s own choice across nodes; '
                        "0: never touch RCCL's environment; N > 0: N, also across nodes.  NCCL_* variables set by the caller always win; "
                        'the values in effect are logged on every rank')
    p.add_argument('--synthetic', action='store_true', help='KITTI-shaped procedural scene, no datadir')
    p.add_argument('--synthetic_hw', type=str, default=None, help="'H,W' of the synthetic frames (default 375,1242)")
    p.add_argument('--synthetic_frames', type=int, default=295)
    p.add_argument('--N_rand_override', type=int, default=None,
                   help='the reference overrides N_rand to 1024 on >14 GB GPUs; this overrides that')
    p.add_argument('--i_test', type=int, default=50000, help='test-set render period (hard-coded 50000 upstream)')
    p.add_argument('--device_sampling', action='store_true',
                   help='(default) keep the training frames in HBM and draw ray batches on the device: no host '
                        'np.random.choice over H*W (4 ms per step at 375x1242), no per-step H2D copies')
    p.add_argument('--image_metrics', action='store_true',
                   help="also score every test render like the reference's utils/eval.py scores the written PNGs: SSIM "
                        '(scikit-image defaults, 7 x 7 uniform window) and PSNR on the 8-bit images, computed on the device from the '
                        'bytes that are written; adds ssim_{step}.txt and psnr8_{step}.txt beside psnr_{step}.txt')
    p.add_argument('--lpips_weights', type=str, default=None, help=LPIPS_WEIGHTS_HELP % 'lpips_{step}.txt')
    p.add_argument('--depth_vis', action='store_true',
                   help="also write every test render's foreground and background depth as pictures, as the reference's "
                        'ddp_test_nerf.py does (colorize_np: jet, min-max over the frame), coloured on the device: '
                        'fg_depth_{idx:06d}.png, bg_depth_{idx:06d}.png.  They carry no colour bar; depth_range_{step:06d}.txt '
                        "lists 'fg_vmin fg_vmax bg_vmin bg_vmax' per image instead")
    p.add_argument('--depth_metrics', action='store_true',
                   help=DEPTH_METRICS_HELP % 'depth_{name}_{step:06d}.txt for the nine names, beside rmse_{step}.txt')
    p.add_argument('--host_sampling', action='store_true',
                   help="the reference's host-side RaySamplerSingleImage.random_sample per step (numpy RNG stream "
                        'of the reference; bounds the step at ~4 ms)')
    return p


LPIPS_WEIGHTS_HELP = ("also score every test render with LPIPS (v0.1, VGG-16) on the device, as the reference's utils/eval.py "
                      'does on the CPU: A[,B] = one or two files (.npz or torch state dicts) that together hold '
                      "torchvision's VGG-16 `features.*` tensors and the lpips package's `lin{0..4}.model.1.weight`; this package "
                      'ships no weights.  Adds %s beside the other metric files')


def validate_args(args):
    if args.netdepth != 8 or args.netwidth != 256:
        raise SystemExit('only netdepth=8 / netwidth=256 (the reference configs) are implemented in HIP')
    if args.max_freq_log2 != 10 or args.max_freq_log2_viewdirs != 4:
        raise SystemExit('only max_freq_log2=10 / max_freq_log2_viewdirs=4 are implemented in HIP')
    if args.use_depth and args.depth_loss_type in DL.DEAD:
        raise SystemExit("depth_loss_type '%s' is dead code in the reference (depth_loss.py:46-76)" %
                         args.depth_loss_type)
    if args.cascade_level != 2:
        raise SystemExit('cascade_level must be 2')
    for name in ('lambda_distortion', 'lambda_opacity'):
        if not (np.isfinite(getattr(args, name)) and getattr(args, name) >= 0):
            raise SystemExit('--%s %r: expected a finite value that is not negative' % (name, getattr(args, name)))
    if args.depth_guide_samples != 0:            # (off: depth_guide.py is not imported)
        from . import depth_guide as DG
        try:
            cascade = [int(x.strip()) for x in args.cascade_samples.split(',')]
            DG.check_samples(args.depth_guide_samples, cascade[1] if len(cascade) > 1 else 0)
            DG.check_std(args.depth_guide_std, have_map=True)
            DG.check_min_std(args.depth_guide_min_std)
        except ValueError as e:
            raise SystemExit('--depth_guide_samples: %s' % e)
    if args.lambda_los != 0:                     # (off: ray_los.py is not imported)
        from . import ray_los as RL
        try:
            RL.check_combination(RL.check_lambda(args.lambda_los), False, args.use_depth, args.depth_loss_type)
            RL.check_sigma_source(args.los_sigma, args.los_sigma_std_mult)
            RL.check_min_sigma(args.los_min_sigma)
            RL.check_decay(args.los_sigma_decay, args.los_sigma_decay_steps)
        except ValueError as e:
            raise SystemExit('--lambda_los: %s' % e)
    PS.check_args(args)


# ------------------------------------------------------------------------------------------------
def render_single_image(rank, world_size, trainer, ray_sampler, chunk_size, keep_dists=True, mlp_events=None):
    """ddp_train_nerf.py:133-249: deterministic sampling, no perturbation, chunked, sharded over ranks
    (ragged last shard instead of raising when H*W % world_size != 0).  Returns, per level, every key of
    `ret` except the two weight tensors, in the reference's order (:210-218) -- including `fg_dists`
    [H, W, S] (0.36 GB per 375x1242 frame at S = 192; keep_dists=False drops it for timing runs).
    mlp_events: optional list; (level, rows, begin, end) HIP-event taps around the MLP kernels (fg + bg) of every
    chunk are appended to it (bench.py's inference leg reads them after a synchronise)."""
    import torch
    from . import ops
    from .dist_utils import shard_sizes, gather_ragged
    trainer.flush()
    b = ray_sampler.get_all()
    n = b['ray_d'].shape[0]
    sizes = shard_sizes(n, world_size)
    lo = sum(sizes[:rank])
    dev = trainer.device
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a[lo:lo + sizes[rank]])).to(dev)
    ray_o, ray_d, min_depth = T(b['ray_o']), T(b['ray_d']), T(b['min_depth'])
    S0 = trainer.cascade_samples[0]
    keys = ('rgb', 'fg_dists', 'fg_rgb', 'fg_depth', 'bg_rgb', 'bg_depth', 'bg_lambda', 'depth')
    if not keep_dists:
        keys = tuple(k for k in keys if k != 'fg_dists')
    out = [OrderedDict((k, []) for k in keys) for _ in range(2)]
    for s in range(0, sizes[rank], chunk_size):
        o, d, md = ray_o[s:s + chunk_size], ray_d[s:s + chunk_size], min_depth[s:s + chunk_size]
        far, fg_z, bg_z = ops.sample_coarse(o, d, md, S0, perturb=False, check=(s == 0))
        ret = None
        for m, eng in enumerate(trainer.engines):
            if m > 0:
                fg_z, bg_z, _ = trainer.fine_samples(fg_z, bg_z, ret, md, far, det=True)
            ev = None
            if mlp_events is not None:
                ev = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
                ev[0].record(); ev[1].record()            # materialise the hipEvent_t handles
                mlp_events.append((m, int(o.shape[0]) * int(fg_z.shape[1]), ev[0], ev[1]))
            ret = eng.forward(o, d, far, fg_z, bg_z, training=False, events=ev)
            for k in keys:
                out[m][k].append(ret[k])
    merged = []
    for m in range(2):
        lvl = OrderedDict()
        for k in keys:
            t = gather_ragged(torch.cat(out[m][k], 0), sizes, rank, world_size)
            if rank == 0:
                lvl[k] = t.cpu().reshape((ray_sampler.H, ray_sampler.W, -1)).squeeze()
        merged.append(lvl)
    return merged if rank == 0 else None


def save_checkpoint(path, trainer, global_step):
    """{net_m: state_dict (DDP-prefixed keys), optim_m: Adam state_dict}   ddp_train_nerf.py:642-652"""
    import torch
    from .model import state_dict_from_flat, adam_state_dict
    trainer.flush()
    # never write (and later auto-reload) a checkpoint of a poisoned run.  Under data parallelism the bad-ray count is summed
    # over ranks, so a check on rank 0 alone would raise here while the other ranks block in the next step's gradient
    # all-reduce: there the training loop runs check_cameras() on EVERY rank right before this call
    if trainer.world_size == 1:
        trainer.check_cameras()
    to_save = OrderedDict()
    for m, eng in enumerate(trainer.engines):
        to_save['net_%d' % m] = OrderedDict((k, v.clone().cpu()) for k, v in
                                            state_dict_from_flat(eng.params).items())
        to_save['optim_%d' % m] = adam_state_dict(trainer.exp_avg[m].cpu(), trainer.exp_avg_sq[m].cpu(),
                                                  trainer.step_count, trainer.lrate)
        if trainer.autoexpo is not None:          # autoexpo_params follow nerf_net in parameters() order
            ae = trainer.autoexpo[m]
            for k, v in ae.state_dict_entries():
                to_save['net_%d' % m][k] = v.cpu()
            opt = to_save['optim_%d' % m]
            base = len(opt['param_groups'][0]['params'])
            for i, st in enumerate(ae.adam_entries()):
                opt['param_groups'][0]['params'].append(base + i)
                if st is not None:
                    opt['state'][base + i] = st
    torch.save(to_save, path)


def load_checkpoint(path, trainer):
    import torch
    from .model import load_state_dict_into_flat, load_adam_state_dict
    ck = torch.load(path, map_location='cpu', weights_only=False)
    for m, eng in enumerate(trainer.engines):
        load_state_dict_into_flat(eng.params, ck['net_%d' % m])
        if 'optim_%d' % m in ck:
            trainer.step_count = load_adam_state_dict(trainer.exp_avg[m], trainer.exp_avg_sq[m], ck['optim_%d' % m])
        eng.repack()
        if trainer.autoexpo is not None:
            ae = trainer.autoexpo[m]
            ae.load_state_dict_entries(ck['net_%d' % m])
            if 'optim_%d' % m in ck:
                from .model import level_param_specs
                base = len(level_param_specs())
                ae.load_adam_entries([ck['optim_%d' % m]['state'].get(base + i) for i in range(len(ae.names))])


def find_latest_checkpoint(args):
    """ddp_train_nerf.py:329-352: explicit --ckpt_path, else the newest model_*.pth by trailing integer."""
    def path2iter(path):
        tmp = os.path.basename(path)[:-4]
        return int(tmp[tmp.rfind('_') + 1:])
    if args.ckpt_path is not None and os.path.isfile(args.ckpt_path):
        ckpts = [args.ckpt_path]
    else:
        d = os.path.join(args.basedir, args.expname)
        ckpts = [os.path.join(d, f) for f in sorted(os.listdir(d)) if f.endswith('.pth')] if os.path.isdir(d) else []
    ckpts = sorted(ckpts, key=path2iter)
    if ckpts and not args.no_reload:
        return ckpts[-1], path2iter(ckpts[-1])
    return None, -1


def minmax8(x):
    """min-max normalised uint8 map (ddp_train_nerf.py:562-564, :593-596).  A constant map is 0 / 0 upstream (NaN cast to
    uint8); here it is written as zeros."""
    x = np.asarray(x, np.float32)
    lo, hi = float(x.min()), float(x.max())
    if not hi > lo:
        return np.zeros(x.shape, np.uint8)
    return (np.clip((x - lo) / (hi - lo), 0., 1.) * 255.).astype(np.uint8)


def write_eval_images(out_dir, idx, ret, sampler, image_pairs=None, depth_frames=None, depth_pairs=None):
    """The per-image artefacts of the in-loop evaluation (ddp_train_nerf.py:549-600): {idx}.png, fg_ / bg_ composites,
    error_rgb_ (mean absolute colour error, min-max normalised), depth_ (uint16 = metres x 256) and absrel_ (absolute depth
    error on the valid ground-truth pixels, min-max normalised).  Returns (psnr | None, rmse | None, absrel | None).
    image_pairs (--image_metrics, --lpips_weights): a list that receives (ground-truth bytes, the bytes written to {idx}.png)
    of every frame that has a ground-truth image, for render_split's image scores.
    depth_frames (--depth_vis): a list that receives (idx, fg_depth, bg_depth) as float32 [H, W] arrays, for write_depth_pictures.
    depth_pairs (--depth_metrics): a list that receives (rendered depth, ground-truth depth, depth scale) of every frame that has
    ground-truth depth, as float32 [H, W] arrays in scene units, for render_split's depth scores."""
    from PIL import Image
    fname = '{:06d}.png'.format(idx)
    im = ret[-1]['rgb'].numpy()
    psnr = rmse = absrel = None
    if sampler.get_img() is not None:
        gt_im = sampler.get_img()
        psnr = float(mse2psnr(np.mean((gt_im - im) * (gt_im - im))))
        Image.fromarray(minmax8(np.abs(im - gt_im).mean(-1))).save(os.path.join(out_dir, 'error_rgb_' + fname))
    if sampler.get_gt_depth_img() is not None:
        pred = ret[-1]['depth'].numpy()
        rmse, absrel, err = EO.depth_errors(pred, sampler.get_gt_depth_img(), sampler.get_depth_scale())   # ddp_train_nerf.py:566-600
        Image.fromarray(EO.depth_u16(pred, sampler.get_depth_scale())).save(os.path.join(out_dir, 'depth_' + fname))
        Image.fromarray(minmax8(err)).save(os.path.join(out_dir, 'absrel_' + fname))
        if depth_pairs is not None:
            depth_pairs.append((np.asarray(pred, np.float32), np.asarray(sampler.get_gt_depth_img(), np.float32),
                                float(sampler.get_depth_scale())))
    im8 = to8b(im)
    Image.fromarray(im8).save(os.path.join(out_dir, fname))
    if image_pairs is not None and sampler.get_img() is not None:
        from .image_metrics import to_bytes_nearest
        image_pairs.append((to_bytes_nearest(sampler.get_img()), im8))
    Image.fromarray(to8b(ret[-1]['fg_rgb'].numpy())).save(os.path.join(out_dir, 'fg_' + fname))
    Image.fromarray(to8b(ret[-1]['bg_rgb'].numpy())).save(os.path.join(out_dir, 'bg_' + fname))
    if depth_frames is not None:
        depth_frames.append((idx, ret[-1]['fg_depth'].numpy().astype(np.float32), ret[-1]['bg_depth'].numpy().astype(np.float32)))
    return psnr, rmse, absrel


def write_depth_pictures(out_dir, step, depth_frames, device):
    """--depth_vis: fg_depth_{idx:06d}.png / bg_depth_{idx:06d}.png of a rendered split (the reference's ddp_test_nerf.py:129-137:
    colorize_np, jet, min-max over the frame) in one device call per frame size (depth_vis.py), and depth_range_{step:06d}.txt
    with 'fg_vmin fg_vmax bg_vmin bg_vmax' per image in place of the reference's colour bar."""
    if not depth_frames:
        return
    from PIL import Image
    from . import depth_vis as DV
    maps = [f[1] for f in depth_frames] + [f[2] for f in depth_frames]         # the fg frames, then the bg frames: one call per size
    rows = EO.FrameBatches(lambda x: DV.minmax_colorize_async(x), (maps,), device=device).get()
    ranges = []
    for (idx, _, _), fg, bg in zip(depth_frames, rows, rows[len(depth_frames):]):
        fname = '{:06d}.png'.format(idx)
        Image.fromarray(fg['image']).save(os.path.join(out_dir, 'fg_depth_' + fname))
        Image.fromarray(bg['image']).save(os.path.join(out_dir, 'bg_depth_' + fname))
        ranges.append((fg['minmax'][0], fg['minmax'][1] + np.float32(TINY_NUMBER), bg['minmax'][0], bg['minmax'][1] + np.float32(TINY_NUMBER)))
    with open(os.path.join(out_dir, 'depth_range_%06d.txt' % step), 'w') as f:
        f.write('\n'.join(' '.join(repr(float(v)) for v in row) for row in ranges))


def wants_image_pairs(args):
    return bool(getattr(args, 'image_metrics', False) or getattr(args, 'lpips_weights', None))


def render_split(rank, world, trainer, samplers, args, out_dir, step, device, lpips_weights):
    """Render every frame of a split and write its files under out_dir, which rank 0 has made (ddp_train_nerf.py:539-640, ddp_test_nerf.py:66-160): the
    images of write_eval_images, {name}_{step:06d}.txt (per image, then the mean) for psnr, rmse and absrel and, by flag, for
    depth_{name} (--depth_metrics: the frames that have ground-truth depth, one device call per frame size and depth scale), ssim and
    psnr8 (--image_metrics) and lpips (--lpips_weights: the frames that have a ground-truth image, one device call each), and the
    pictures of --depth_vis.  Every rank renders every frame; rank 0 writes and returns the (name, mean) pairs of the files it wrote,
    in that order."""
    scores = OrderedDict((name, []) for name in ('psnr', 'rmse', 'absrel'))
    image_pairs = [] if wants_image_pairs(args) else None
    depth_frames = [] if getattr(args, 'depth_vis', False) else None
    depth_pairs = [] if getattr(args, 'depth_metrics', False) else None
    for idx, sampler in enumerate(samplers):
        ret = render_single_image(rank, world, trainer, sampler, args.chunk_size, keep_dists=False)   # fg_dists is never read below
        if rank != 0:
            continue
        for name, v in zip(scores, write_eval_images(out_dir, idx, ret, sampler, image_pairs, depth_frames, depth_pairs)):
            if v is not None:
                scores[name].append(v)
    if rank != 0:
        return []
    write_depth_pictures(out_dir, step, depth_frames, device)
    if depth_pairs:
        preds, gts, scales = zip(*depth_pairs)
        scores.update(('depth_' + name, vals) for name, vals in EO.depth_scores(preds, gts, scales, device).items())
    if image_pairs:
        gts, preds = zip(*image_pairs)
        if getattr(args, 'image_metrics', False):
            scores.update(EO.image_scores(gts, preds, device))
        if lpips_weights is not None:
            scores.update(EO.lpips_scores(gts, preds, lpips_weights, device))
    return [(name, EO.write_scores(os.path.join(out_dir, '%s_%06d.txt' % (name, step)), vals)[-1]) for name, vals in scores.items() if vals]


def ddp_train_nerf(rank, args):
    import torch
    from .trainer import NerfppTrainer, batch_to_device
    from .data_loader_split import load_data_split, synthetic_ray_samplers
    from . import _lib as L
    setup_logger()
    lpips_weights = load_lpips_weights(args) if rank == 0 else None
    world = args.world_size
    torch.cuda.set_device(rank)
    device = torch.device('cuda', rank)
    if world > 1:
        import torch.distributed as dist
        os.environ.setdefault('MASTER_ADDR', '127.0.0.1')
        os.environ['MASTER_PORT'] = str(args.port)
        from .dist_utils import apply_rccl_env_defaults
        # few channels: a CU RCCL holds is a CU a tile cannot use (dist_utils.py); process-global, so only on one node by default
        eff = apply_rccl_env_defaults(world, None if args.rccl_channels < 0 else args.rccl_channels)
        logger.info('rank %d RCCL environment: %s' % (rank, ' '.join('%s=%s' % kv for kv in sorted(eff.items())) or "RCCL's defaults"))
        dist.init_process_group('nccl', rank=rank, world_size=world, device_id=device)   # RCCL (gloo upstream, :298)

    # batch sizes by GPU memory                                      ddp_train_nerf.py:364-373
    if torch.cuda.get_device_properties(rank).total_memory / 1e9 > 14:
        args.N_rand, args.chunk_size = 1024, 8192
    else:
        args.N_rand, args.chunk_size = 512, 4096
    if args.N_rand_override:
        args.N_rand = args.N_rand_override
        args.chunk_size = max(args.chunk_size, 8 * args.N_rand_override)

    exp_dir = os.path.join(args.basedir, args.expname)
    if rank == 0:                                                   # :376-386
        os.makedirs(exp_dir, exist_ok=True)
        with open(os.path.join(exp_dir, 'args.txt'), 'w') as f:
            for arg in sorted(vars(args)):
                f.write('{} = {}\n'.format(arg, getattr(args, arg)))
        if args.config is not None:
            with open(os.path.join(exp_dir, 'config.txt'), 'w') as f:
                f.write(open(args.config, 'r').read())
    if world > 1:
        dist.barrier()

    # the prior's standard deviation travels with the training frames only of a run whose depth loss reads it
    std_kw = {'depth_std': args.depth_gnll_std} if (args.use_depth and DL.needs(args.depth_loss_type, 'depth_std')) else {}
    los_needs_std = args.lambda_los > 0 and args.los_sigma_std_mult > 0
    guide_std_optional = not std_kw and (args.depth_guide_samples > 0 or los_needs_std)
    if guide_std_optional:                        # ... or whose fine sampling or line-of-sight band does: the folder, then a stage's;
        std_kw = {'depth_std': 0.0}               # optional while loading: each consumer looks at what arrived, below
    if args.synthetic:
        hw = [int(x) for x in args.synthetic_hw.split(',')] if args.synthetic_hw else [None, None]
        ray_samplers = synthetic_ray_samplers('train', args.trainskip, args.depth_sup_type,
                                              args.synthetic_frames, hw[0], hw[1], **std_kw)
        val_ray_samplers = synthetic_ray_samplers('test', args.testskip, args.depth_sup_type,
                                                  args.synthetic_frames, hw[0], hw[1])
    else:
        if std_kw and (guide_std_optional or PS.std_source(*PS.check_args(args)) is not None):
            std_kw['depth_std_optional'] = True  # the standard deviation: the folder, then the constant, then a stage's
        ray_samplers = load_data_split(args.datadir, args.scene, split='train', skip=args.trainskip,
                                       try_load_min_depth=args.load_min_depth, depth_sup_type=args.depth_sup_type, **std_kw)
        val_ray_samplers = load_data_split(args.datadir, args.scene, split='test', skip=args.testskip,
                                           try_load_min_depth=args.load_min_depth, depth_sup_type=args.depth_sup_type)
    depth_scale = ray_samplers[0].get_depth_scale() or 1.0
    def load_anchors(sup_type):                   # the training frames under the type of an alignment's anchor that is read, not computed
        if args.synthetic:
            return synthetic_ray_samplers('train', args.trainskip, sup_type, args.synthetic_frames, hw[0], hw[1])
        return load_data_split(args.datadir, args.scene, split='train', skip=args.trainskip, try_load_min_depth=False, depth_sup_type=sup_type)
    # the stages that compute or repair the training prior, once, each logging its totals as it ends
    PS.run_samplers(args, ray_samplers, device, depth_scale, bool(std_kw), load_anchors, logger.info if rank == 0 else None)
    los_kw = {}
    if args.lambda_los > 0:
        if los_needs_std and not all(rs.depth_std is not None for rs in ray_samplers):
            raise SystemExit('--los_sigma_std_mult %g: the training frames carry no standard deviation of the prior (no train/depth%s_std/ '
                             'folder, no stage that estimates one): write the maps there, or pass --los_sigma, metres, positive'
                             % (args.los_sigma_std_mult, '_' + args.depth_sup_type if args.depth_sup_type != 'gt' else ''))
        los_kw = dict(lambda_los=args.lambda_los, los_sigma=args.los_sigma if args.los_sigma > 0 else None,
                      los_sigma_std_mult=args.los_sigma_std_mult, los_min_sigma=args.los_min_sigma,
                      los_sigma_decay=args.los_sigma_decay, los_sigma_decay_steps=args.los_sigma_decay_steps)
    guide_kw = {}
    if args.depth_guide_samples > 0:
        # every frame carries a map (the folder's, a constant's or a stage's): it is read.  Otherwise the trainer falls back to the constant
        have_map = all(rs.depth_std is not None for rs in ray_samplers)
        if not have_map:
            if not args.depth_guide_std > 0:
                raise SystemExit('--depth_guide_samples %d: the training frames carry no standard deviation of the prior (no '
                                 'depth[_<sup_type>]_std/ folder, no stage that estimates one): pass --depth_guide_std, metres, positive'
                                 % args.depth_guide_samples)
            for rs in ray_samplers:               # (the line-of-sight band has not come this far without a map on every frame)
                rs.depth_std = None
        guide_kw = dict(depth_guide_samples=args.depth_guide_samples, depth_guide_std=None if have_map else args.depth_guide_std,
                        depth_guide_min_std=args.depth_guide_min_std)
    img_names = None
    if args.optim_autoexpo:                       # :394-399 (written before the nets need it, unlike upstream)
        img_names = [rs.img_path or 'synthetic/train/rgb/%06d.png' % i for i, rs in enumerate(ray_samplers)]
        if rank == 0:
            import json
            with open(os.path.join(exp_dir, 'train_images.json'), 'w') as f:
                json.dump(img_names, f, indent=2)
    device_samplers = None
    if not args.host_sampling:
        from .device_sampler import DeviceRaySamplers
        if len(set((rs.H, rs.W) for rs in ray_samplers)) == 1:
            device_samplers = DeviceRaySamplers(ray_samplers, device, seed=(rank + 1) * 777)
        else:
            logger.info('frames of different sizes: falling back to host-side ray sampling')

    cascade = tuple(int(x.strip()) for x in args.cascade_samples.split(','))
    comm = None
    if args.grad_comm == 'rccl_abi':
        from .dist_utils import RcclComm
        comm = RcclComm(rank, world)
    trainer = NerfppTrainer(device, precision={'bf16': L.PREC_BF16, 'split': L.PREC_SPLIT_BF16, 'split_fwd': L.PREC_SPLIT_FWD,
                                               'fp16_fwd': L.PREC_FP16_FWD}[args.precision],
                            cascade_samples=cascade, lrate=args.lrate, use_depth=args.use_depth,
                            depth_loss_type=args.depth_loss_type, lambda_depth=args.lambda_depth,
                            depth_sigma=args.depth_sigma, depth_scale=depth_scale, world_size=world,
                            optim_autoexpo=args.optim_autoexpo, img_names=img_names,
                            lambda_autoexpo=args.lambda_autoexpo, seed=(rank + 1) * 777, comm=comm,    # :406-408
                            depth_ssi_min_rays=args.depth_ssi_min_rays, lambda_distortion=args.lambda_distortion,
                            lambda_opacity=args.lambda_opacity, **guide_kw, **los_kw)
    if rank == 0:
        # (the default is the slowest mode -- say so at start-up, with the alternatives and what they cost / keep)
        logger.info('precision = %s%s.  Relative throughput on one MI355X (bench.py, round 6): bf16 1.0, fp16_fwd 0.81, split_fwd 0.67, '
                    'split 0.40; split / split_fwd keep rendered RGB, depth and loss within 1e-4 of the float32 reference (split also the '
                    'gradients), bf16 is at bf16 grade (1e-2) -- see --help' % (args.precision, ' (the default)' if args.precision == 'split' else ''))
    ckpt, start = find_latest_checkpoint(args)
    if ckpt is not None:
        logger.info('Reloading from: {}'.format(ckpt))
        load_checkpoint(ckpt, trainer)

    np.random.seed((rank + 1) * 777)                                # :406
    torch.manual_seed((rank + 1) * 777)                             # :408
    writer = None
    if rank == 0:
        try:
            from tensorboardX import SummaryWriter
            writer = SummaryWriter(os.path.join(args.basedir, 'summaries', args.expname))
        except ImportError:
            logger.info('tensorboardX not installed: scalars go to the console only')

    for global_step in range(start + 1, start + 1 + args.N_iters):
        if global_step == start + 1:
            t_log, n_log = time.time(), 0
        n_log += 1
        if device_samplers is not None:
            ray_batch = device_samplers.random_sample(args.N_rand)   # two small kernels on the training stream: +0.8 % of a step
            # (drawing the next batch on a side stream instead measured +1.0 %: profiles/r04_cli_loop.md)
        else:
            i = np.random.randint(low=0, high=len(ray_samplers))
            ray_batch = batch_to_device(ray_samplers[i].random_sample(args.N_rand, center_crop=False), device)
            if img_names is not None:
                ray_batch['img_name'] = img_names[i]
        scalars = trainer.train_step(ray_batch)
        log_now = rank == 0 and (global_step % args.i_print == 0 or global_step < 10)
        if global_step % args.i_print == 0 or global_step < 10:
            trainer.check_cameras()               # every rank: the reference raises per step (:62-63)
        if log_now:
            scalars_to_log = OrderedDict([('resolution', ray_samplers[0].resolution_level)])
            for m, sc in enumerate(scalars):
                sc = sc.cpu().numpy()
                if not np.isfinite(sc[:2]).all():
                    raise FloatingPointError('non-finite loss at step %d, level %d: loss=%r rgb_loss=%r (check the '
                                             'scene normalisation / input data)' % (global_step, m, sc[0], sc[1]))
                if args.use_depth:
                    scalars_to_log['level_{}/loss_depth'.format(m)] = float(sc[2])
                if trainer.last_autoexpo[m] is not None:
                    scalars_to_log['level_{}/autoexpo_scale'.format(m)] = float(trainer.last_autoexpo[m][0])
                    scalars_to_log['level_{}/autoexpo_shift'.format(m)] = float(trainer.last_autoexpo[m][1])
                scalars_to_log['level_{}/rgb_loss'.format(m)] = float(sc[1])
                scalars_to_log['level_{}/pnsr'.format(m)] = float(mse2psnr(float(sc[1])))
                if trainer.last_ray_reg is not None:          # a regulariser is on: its values and the share of rays with far > min_depth
                    values, stats = trainer.last_ray_reg[m]
                    scalars_to_log['level_{}/distortion'.format(m)] = float(values[0])
                    scalars_to_log['level_{}/opacity'.format(m)] = float(values[1])
                    scalars_to_log['level_{}/ray_reg_valid'.format(m)] = float(stats[0]) / int(ray_batch['ray_o'].shape[0])
                if trainer.last_ray_los is not None:          # the line-of-sight term is on: its value and, per supervised ray,
                    values, stats = trainer.last_ray_los[m]   # the mass in front of the band
                    stats = stats.cpu().numpy()
                    scalars_to_log['level_{}/los'.format(m)] = float(values[0])
                    scalars_to_log['level_{}/los_front'.format(m)] = float(stats[1]) / max(float(stats[0]), 1.0)
                if trainer.last_depth_guide is not None and trainer.last_depth_guide[m] is not None:
                    # depth-guided sampling is on: the share of the batch's rays whose guided samples lie around the prior
                    scalars_to_log['level_{}/guided'.format(m)] = float((trainer.last_depth_guide[m] == 0).float().mean())
            # the steps are queued asynchronously; reading the scalars above synchronised, so the wall time
            # since the previous log line over the steps it covers is the true time per iteration
            scalars_to_log['iter_time'] = (time.time() - t_log) / max(n_log, 1)
            t_log, n_log = time.time(), 0
            logstr = '{} step: {} '.format(args.expname, global_step)
            for k, v in scalars_to_log.items():
                logstr += ' {}: {:.6f}'.format(k, v)
                if writer is not None:
                    writer.add_scalar(k, v, global_step)
            # 'gnll': the share of the batch's supervised rays the gate let through (last level)
            logstr += DL.depth_log_tail(trainer.loss_type, DL.kept_stats(trainer, trainer.loss_type))
            logger.info(logstr)

        if (global_step % args.i_test == 0) and global_step != 0:   # :539-640
            out_dir = os.path.join(exp_dir, 'render_{}_{:06d}'.format('test', global_step))
            if rank == 0:
                os.makedirs(out_dir, exist_ok=True)
            trainer.check_cameras()
            for name, mean in render_split(rank, world, trainer, val_ray_samplers, args, out_dir, global_step, device, lpips_weights):
                if writer is not None:
                    writer.add_scalar('test_' + name, mean, global_step)
                logger.info('test_%s: %s' % (name, mean))

        if global_step % args.i_weights == 0 and global_step > 0:   # :642-652
            trainer.check_cameras()               # every rank, so that all raise together: never write (and later auto-reload) a checkpoint of a poisoned run
        if rank == 0 and (global_step % args.i_weights == 0 and global_step > 0):
            save_checkpoint(os.path.join(exp_dir, 'model_{:06d}.pth'.format(global_step)), trainer, global_step)

    trainer.flush()                               # the last step's level-1 update is applied lazily under DP
    trainer.check_cameras()
    on_finish = getattr(args, 'on_finish', None)  # (bench.py: times the kernel-only step on the SAME trained state)
    if on_finish is not None:
        on_finish(trainer, device_samplers if device_samplers is not None else ray_samplers)
    if comm is not None:
        torch.cuda.synchronize()
        comm.destroy()                            # the library's own communicator, before the process group that carried its id
    if world > 1:
        dist.destroy_process_group()


def train(argv=None):
    import torch
    parser = config_parser()
    args = parser.parse_args(argv)
    validate_args(args)
    if os.path.exists(os.path.join(args.basedir, args.expname)):     # :733-735
        print('already trained, exiting...')
        sys.exit(0)
    if args.world_size == -1:
        args.world_size = torch.cuda.device_count()
    if args.world_size <= 1:
        args.world_size = 1
        ddp_train_nerf(0, args)
    else:
        torch.multiprocessing.spawn(ddp_train_nerf, args=(args,), nprocs=args.world_size, join=True)


if __name__ == '__main__':
    setup_logger()
    train()

"""Per-rank optimisation step of the NeRF++ path on the HIP library.

Mirrors the per-cascade-level loop of nerf-methods/nerfplusplus/ddp_train_nerf.py:432-498:
level 0 draws stratified depths, level 1 re-samples from level 0's (detached) weights; each level
has its own net, its own Adam state and its own gradient all-reduce (DDP averages gradients,
:323); the depth term is added when --use_depth (:486-493).
"""
import contextlib

import numpy as np
import torch

from . import _lib as L
from . import depth_losses as DL
from . import ops
from .model import init_level_params

# (what the reference computes.  The MLP kernels execute 65 536 fewer per net in the forward and in the dX chain: the remap layer
# is folded into the colour head, csrc/nerfpp_common.h.)
ALGO_MACS = {            # dense MACs per sample (SURVEY.md 8a / BASELINE.md section 2)
    'fwd': (593408, 604160),         # fg, bg forward (= weight-gradient MACs)
    'dx': (557696, 557696),          # backward dX chain (no dX for L0, raw-input part of L5, dirs)
}


class NerfppTrainer(object):
    def __init__(self, device, precision=L.PREC_SPLIT_BF16, cascade_samples=(64, 128), lrate=5e-4,
                 use_depth=True, depth_loss_type='mse', lambda_depth=0.1, depth_sigma=0.01, depth_scale=1.0,
                 world_size=1, level_params=None, overlap_allreduce=True, optim_autoexpo=False, img_names=None,
                 lambda_autoexpo=1.0, seed=777, torch_rng=False, fuse_loss=False, comm=None, depth_ssi_min_rays=8,
                 lambda_distortion=0.0, lambda_opacity=0.0, depth_guide_samples=0, depth_guide_std=None, depth_guide_min_std=0.0,
                 lambda_los=0.0, los_sigma=None, los_sigma_std_mult=0.0, los_min_sigma=0.0, los_sigma_decay=1.0,
                 los_sigma_decay_steps=0):
        """seed: key of the in-kernel sampling RNG (the CLI passes (rank+1)*777 like ddp_train_nerf.py:406-408);
        torch_rng=True draws the four uniform tensors with torch.rand in the reference's call order instead
        (4 extra launches per step).  comm: optional dist_utils.RcclComm -- the gradient average then goes through the
        library's own RCCL entry point (nerfpp_allreduce_mean) instead of torch.distributed.all_reduce.
        depth_loss_type: a row of depth_losses.LOSSES.  'ssi' and 'gnll' are not in the reference; they run as after-calls behind the
        rgb-only loss head: 'ssi' on every level's depth, one fit per batch (a batch is one frame), skipped for a
        batch with fewer than depth_ssi_min_rays supervised rays; 'gnll' on the level's depth and its foreground weights, with the
        batch's depth_std.
        lambda_distortion, lambda_opacity: weights of the two regularisers on every level's foreground weights (ray_reg.py, DESIGN
        9.11): a distortion loss on the sample intervals normalised to [min_depth, far] and the entropy of the foreground opacity.
        0 = off; with both off the module is not imported and a step makes the calls it made without them.
        depth_guide_samples: G of the cascade_samples[1] new foreground depths of every level m > 0 are drawn from a Gaussian around
        the batch's depth prior, truncated at three standard deviations, instead of from the previous level's weights
        (depth_guide.py), whatever the depth loss is; a ray without a prior, and every ray of a batch without
        depth_sup, takes them around the depth and spread the previous level rendered.  0 <= G < cascade_samples[1], else
        ValueError.  The standard deviation is the batch's depth_std, or depth_guide_std (metres, times depth_scale) where the
        batch has none: None (default) says that every batch with a prior carries depth_std, a number must be positive.
        depth_guide_min_std (metres, times depth_scale): a floor under either.  0 = off: nothing of depth_guide.py is imported,
        loaded or launched, and a step and a render make exactly the calls they made without it.
        lambda_los: weight of Urban Radiance Fields' line-of-sight term on every level's foreground weights (ray_los.py, DESIGN
        9.13), beside the depth loss: on a ray with a prior it empties the intervals in front of the band prior +- sigma and pulls
        the weight of the intervals that touch the band to the mass of N(prior, (sigma / 3)^2) in them.  sigma per ray and step:
        los_sigma (metres, times depth_scale), or los_sigma_std_mult times the batch's depth_std where the multiplier is positive;
        floored at los_min_sigma (metres, times depth_scale); times los_sigma_decay ** (min(step_count, los_sigma_decay_steps) /
        los_sigma_decay_steps), URF's annealing of the band (0 steps = none; step_count survives a resume).  Needs use_depth and a
        metric prior (not 'ssi'), not fuse_loss: ValueError.  0 = off: nothing of ray_los.py is imported, loaded or launched, and a
        step makes exactly the calls it made without it."""
        self.device = torch.device(device)
        self.depth_guide = None           # the binding, imported when depth_guide_samples is on
        self.depth_guide_samples, self.depth_guide_std, self.depth_guide_min_std = 0, None, 0.0
        if depth_guide_samples != 0:
            from . import depth_guide
            cascade_samples = tuple(cascade_samples)
            self.depth_guide_samples = depth_guide.check_samples(depth_guide_samples, cascade_samples[1] if len(cascade_samples) > 1 else 0)
            std = depth_guide.check_std(depth_guide_std, have_map=depth_guide_std is None)
            self.depth_guide_std = None if std is None else std * depth_scale
            self.depth_guide_min_std = depth_guide.check_min_std(depth_guide_min_std) * depth_scale
            self.depth_guide = depth_guide
        # depth_guide_samples on: [levels] the `mode` tensor [n] int32 of the last step's depth_guide call (None for level 0): 0 = around
        # the prior, 1 = around the previous level's depth, 2 = stratified -- read it where the caller synchronises anyway
        self.last_depth_guide = None
        for name, v in (('lambda_distortion', lambda_distortion), ('lambda_opacity', lambda_opacity)):
            if not (np.isfinite(v) and v >= 0):
                raise ValueError('%s = %r: expected a finite value that is not negative' % (name, v))
        self.lambda_distortion, self.lambda_opacity = float(lambda_distortion), float(lambda_opacity)
        self.ray_reg = None               # the binding, imported when a lambda is on
        if self.lambda_distortion > 0 or self.lambda_opacity > 0:
            if fuse_loss:
                raise ValueError('fuse_loss and lambda_distortion / lambda_opacity cannot be combined: the fused backward forms the '
                                 'loss gradient itself and ignores g_fg_weights')
            from . import ray_reg
            self.ray_reg = ray_reg
        # a lambda on: [levels] (values [2] = (distortion, opacity), stats [1] = (rays with far > min_depth)) of the last step, device
        # tensors -- read them where the caller synchronises anyway
        self.last_ray_reg = None
        self.ray_los = None               # the binding, imported when lambda_los is on
        self.lambda_los = float(lambda_los)
        if not (np.isfinite(self.lambda_los) and self.lambda_los >= 0):
            raise ValueError('lambda_los = %r: expected a finite value that is not negative' % (lambda_los,))
        if self.lambda_los > 0:
            from . import ray_los
            ray_los.check_combination(self.lambda_los, fuse_loss, use_depth, depth_loss_type)
            sigma, self.los_sigma_std_mult = ray_los.check_sigma_source(los_sigma, los_sigma_std_mult)
            self.los_sigma = None if sigma is None else sigma * depth_scale
            self.los_min_sigma = ray_los.check_min_sigma(los_min_sigma) * depth_scale
            self.los_sigma_decay, self.los_sigma_decay_steps = ray_los.check_decay(los_sigma_decay, los_sigma_decay_steps)
            self.ray_los = ray_los
        # lambda_los on: [levels] (values [1] = (the term), stats [2] = (supervised rays, their summed mass in front of the band)) of
        # the last step, device tensors -- read them where the caller synchronises anyway; and the step's sigma [n]
        self.last_ray_los = None
        self.last_los_sigma = None
        self.comm = comm
        self.precision = precision
        self.cascade_samples = tuple(cascade_samples)
        self.lrate = lrate
        self.loss_type = depth_loss_type if use_depth else 'rgbonly'
        if self.loss_type not in DL.names('nerfpp'):
            raise ValueError("depth_loss_type %r: only mse / l1 / kl exist in the reference "
                             "('los' and 'nll' are dead code there); ssi is this implementation's, and so is gnll" % depth_loss_type)
        row = DL.LOSSES[self.loss_type]
        self.ssi_min_rays = int(depth_ssi_min_rays)
        if 'min_rays' in row.extra and self.ssi_min_rays < 1:
            raise ValueError("depth_loss_type %r: depth_ssi_min_rays = %r, expected at least 1" % (self.loss_type, depth_ssi_min_rays))
        self.last_gnll_stats = None       # 'gnll': [levels][1, 3] = (supervised, gated, clamped rays) of the last step
        for flag, name in ((fuse_loss, 'fuse_loss'), (optim_autoexpo, 'optim_autoexpo')):
            if flag and name in row.refuses:
                raise ValueError("depth_loss_type %r and %s cannot be combined: %s" % (self.loss_type, name, DL.REFUSAL[name]))
        self.lambda_depth = lambda_depth
        self.kl_sigma = depth_sigma * depth_scale           # ddp_train_nerf.py:489
        self.world_size = world_size
        if level_params is None:
            level_params = init_level_params(len(self.cascade_samples))   # manual_seed(777), :308
        self.engines = [ops.LevelEngine(p.to(self.device), precision) for p in level_params]
        self.exp_avg = [torch.zeros_like(e.params) for e in self.engines]
        self.exp_avg_sq = [torch.zeros_like(e.params) for e in self.engines]
        # [LEVEL_PARAMS gradient | bad-camera flag | pad]: the flag rides the gradient all-reduce (a SUM over ranks) and is
        # the device-side predicate of the Adam step, so that NO rank applies an update computed from rays that left the
        # unit sphere (the reference raises before the step, ddp_train_nerf.py:62-63; here the count is read later)
        self.grads = [torch.zeros(L.LEVEL_PARAMS + 4, device=self.device) for _ in self.engines]
        self.step_count = 0
        self.seed, self.torch_rng = int(seed), bool(torch_rng)
        # loss-head gradient inside the compositing backward (nerfpp_backward_args.fused_loss; not with auto-exposure).
        # Bit-identical to the two-call path; measured in one process (tools/ab_step.py, profiles/r03_ab_*): 2.717 ms per
        # step fused vs 2.704 separate -- the loss launch it takes off the critical path (~9 us) is paid back by the recount
        # in every compositing workgroup and the extra stream events, so the default stays the separate launch.
        self.fuse_loss = bool(fuse_loss)
        self.rng_step = 0                 # counter of the in-kernel RNG (not reset by checkpoint reloads of step_count)
        # rays whose closest point to the origin lies outside the unit sphere, summed over all steps since
        # the last check_cameras() (the reference raises on the spot, ddp_train_nerf.py:62-63; here the
        # counter is read wherever the caller synchronises anyway)
        self.bad_cameras = torch.zeros(1, dtype=torch.int32, device=self.device)
        # per-image auto-exposure parameters, one set per level's net (ddp_model.py:161-192)
        self.autoexpo = None
        if optim_autoexpo:
            if not img_names:
                raise ValueError('optim_autoexpo needs the training image names (ddp_model.py:168)')
            from .autoexpo import AutoExposure
            self.img_names = list(img_names)
            self.autoexpo = [AutoExposure(img_names, self.device, lrate, lambda_autoexpo, world_size)
                             for _ in self.engines]
        self._ae_grad = [None] * len(self.engines)
        self.last_autoexpo = [None] * len(self.engines)
        # The parameter update of a level (split-K slab sum -> [RCCL all-reduce] -> Adam -> re-pack of the bf16 weight
        # streams: four to six short launches that leave most CUs idle) runs on a side stream under the NEXT level's
        # sampling + forward; the main stream waits for it right before the level's streams are used again, i.e. at
        # the same level of the next step.  overlap_allreduce=False keeps everything on the caller's stream.
        self.update_stream = torch.cuda.Stream(device=self.device) if overlap_allreduce else None
        self.level_streams = [torch.cuda.Stream(device=self.device) for _ in range(len(self.cascade_samples))] if overlap_allreduce else None
        self.concurrent_backward = True     # level 0's backward on its own stream under level 1's forward (False: inline)
        self._pending = {}                # level -> event recorded after its update on the side stream
        # diagnostic (bench.py, N > 1): when a list, every _update_end appends a (before, after) timing-event pair around
        # the main stream's wait for the side-stream update -- the part of [slab sum, all-reduce, Adam, re-pack] that the
        # next level's sampling + forward did NOT hide
        self.wait_taps = None
        # diagnostic (bench.py, N > 1): when a list, every gradient all-reduce appends (level, begin, end) timing events recorded
        # around it on the stream it is issued on -- the duration of the collective as the GPU saw it (queueing behind the slab
        # sum included in `begin`'s position, not in the interval)
        self.comm_taps = None

    # -- parameter update ----------------------------------------------------------------------------
    def _update(self, m, step):
        """reduce the weight-gradient slabs, average over ranks (DDP semantics: grads were pre-scaled by
        1/world_size in the reduction, so a SUM all-reduce yields the mean, ddp_train_nerf.py:323), Adam, re-pack."""
        eng = self.engines[m]
        eng.reduce_grads()
        # the slab sum wrote float(bad_cameras) -- cumulative since the last check_cameras() -- behind the gradients
        # (nerfpp_backward_args.bad_count; until round 6 a torch copy_ launch per level and step)
        flag = self.grads[m][L.LEVEL_PARAMS:L.LEVEL_PARAMS + 1]
        if self.world_size > 1 or self.comm is not None:
            import torch.distributed as dist
            if self.autoexpo is not None:
                # [n_img, 3]: grads | used flag; a few hundred bytes.  EVERY rank issues this collective every
                # step: a rank whose image has no auto-exposure entry (ddp_model.py:186 falls back to the plain
                # rgb loss) contributes zeros, otherwise the ranks' collective sequences would diverge
                if self._ae_grad[m] is None:
                    self._ae_grad[m] = torch.zeros(len(self.autoexpo[m].names), 3, device=self.device)
                if self.comm is not None:
                    self.comm.allreduce_mean(self._ae_grad[m].view(-1), prescaled=True)
                else:
                    dist.all_reduce(self._ae_grad[m])
            tap = None
            if self.comm_taps is not None:
                tap = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
                tap[0].record()
            if self.comm is not None:
                self.comm.allreduce_mean(self.grads[m], prescaled=True)      # grads carry 1 / world_size already (grad_scale)
            else:
                dist.all_reduce(self.grads[m])
            if tap is not None:
                tap[1].record()
                self.comm_taps.append((m, tap[0], tap[1]))
        ops.adam_step(eng.params, self.grads[m][:L.LEVEL_PARAMS], self.exp_avg[m], self.exp_avg_sq[m], step, lr=self.lrate,
                      skip=flag)
        eng.repack()
        if self._ae_grad[m] is not None:
            self.autoexpo[m].apply(self._ae_grad[m][:, :2], self._ae_grad[m][:, 2] > 0)
            self._ae_grad[m] = None

    @staticmethod
    def _after_here(stream):
        """Order `stream` after what is queued on the current one.  Returns the context in which launches go to `stream`."""
        ev = torch.cuda.Event()
        ev.record()
        stream.wait_event(ev)
        return torch.cuda.stream(stream)

    def _update_begin(self, m):
        if self.update_stream is None:
            self._update(m, self.step_count)
            return
        side = self._after_here(self.update_stream)
        if self._ae_grad[m] is not None:
            self._ae_grad[m].record_stream(self.update_stream)
        with side:
            self._update(m, self.step_count)
            done = torch.cuda.Event()
            done.record()
        self._pending[m] = done

    def _update_end(self, m):
        done = self._pending.pop(m, None)
        if done is not None:
            if self.wait_taps is not None:
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                torch.cuda.current_stream().wait_event(done)
                b.record()
                self.wait_taps.append((a, b))
            else:
                torch.cuda.current_stream().wait_event(done)

    def flush(self):
        """Order the caller's stream after the parameter updates still running on the side stream.  Call before
        reading parameters or using the engines directly: checkpoints, rendering, the end of a timed region."""
        for m in list(self._pending):
            self._update_end(m)

    def check_cameras(self):
        """Raise the reference's exception (ddp_train_nerf.py:62-63) if any ray of any step since the last
        call left the unit sphere -- on ANY rank: the count rides the gradient all-reduce, so every rank raises
        together instead of one raising and the others blocking in the next collective.  From the first bad step
        until this call the Adam updates are dropped on the device (adam_step(skip=...)), i.e. the parameters are
        what they were when the reference would have raised.  Synchronises (a few bytes D2H): call it where the loop
        syncs anyway -- the log line, checkpoints, evaluation, the end of training."""
        bad = int(self.bad_cameras.item())
        if self.world_size > 1 and self.step_count > 0:
            self.flush()
            bad += int(sum(float(g[L.LEVEL_PARAMS].item()) for g in self.grads))
        if bad != 0:
            self.bad_cameras.zero_()
            for g in self.grads:
                g[L.LEVEL_PARAMS:].zero_()
            raise Exception(ops.CAMERA_ERROR)

    # -- the parts of a level ------------------------------------------------------------------------
    def fine_samples(self, fg_z, bg_z, ret, min_depth, far, batch=None, uniforms=None, rng=None, det=False):
        """The depths of a level m > 0 from the previous level's depths and `ret`: (fg_z, bg_z, mode); mode: depth_guide's [n] int32
        tensor, None with depth_guide_samples off.  det: the deterministic forms a render takes, which read no prior (`batch` is not
        looked at); else rng = (seed, step) draws the uniforms in the kernels; else they are `uniforms`', torch.rand where it has none."""
        prev = (fg_z, ret['fg_weights'], bg_z, ret['bg_weights'], self.cascade_samples[1])
        u = uniforms or {}
        if self.depth_guide is None:
            return ops.sample_fine_pair(*prev, det=det, u_fg=u.get('u_fg'), u_bg=u.get('u_bg'), rng=rng) + (None,)
        if det:
            # as training sampled, in deterministic form and without a prior: around the previous level's depth and spread
            kw = dict(det=True)
        else:
            # G of the S1 new foreground depths around the prior (whatever the depth loss is), the others and the background
            # from the existing fine sampling; positions carry no gradient, so nothing below sees more than other depths
            prior, prior_std = batch.get('depth_sup'), batch.get('depth_std')
            if prior is not None and prior_std is None and self.depth_guide_std is None:
                raise ValueError('depth_guide_samples: the batch has a depth prior without depth_std, and no depth_guide_std was given')
            kw = dict(prior=None if prior is None else prior.contiguous().float(),
                      prior_std=None if prior_std is None else prior_std.contiguous().float(), std_const=self.depth_guide_std or 0.0,
                      u_fg=u.get('u_fg'), u_bg=u.get('u_bg'), v_fg=u.get('v_fg'), rng=rng)
        return self.depth_guide.fine_level(*prev, self.depth_guide_samples, min_depth.contiguous().float(), far,
                                           min_std=self.depth_guide_min_std, **kw)

    def los_band(self, batch):
        """This step's half-width [n] of the line-of-sight band, in scene units, formed on the device: the constant or the multiple of
        the batch's depth_std, floored, annealed by step_count"""
        for key in ('depth_sup',) + (('depth_std',) if self.los_sigma_std_mult > 0 else ()):
            if batch.get(key) is None:
                raise L.NerfppError("lambda_los: the batch has no %s" % key)
        if self.los_sigma_std_mult > 0:
            sigma = batch['depth_std'].contiguous().float() * self.los_sigma_std_mult
        else:
            sigma = torch.full_like(batch['depth_sup'], self.los_sigma, dtype=torch.float32)
        if self.los_min_sigma > 0:
            sigma = sigma.clamp_min(self.los_min_sigma)
        factor = self.ray_los.decay_factor(self.los_sigma_decay, self.los_sigma_decay_steps, self.step_count)
        return sigma * factor if factor != 1.0 else sigma

    def _loss_head(self, m, ret, batch, depth_sup, fg_z, far, ae, ae_idx):
        """Level m's (scalars, g_rgb, g_depth, g_w): the loss head of the depth loss, then auto-exposure, then the regularisers and
        the line-of-sight term."""
        row = DL.LOSSES[self.loss_type]
        rgb_gt = ae.target(ae_idx, batch['rgb']) if ae is not None else batch['rgb']
        if row.nerfpp == DL.AFTER:
            for key in ('depth_sup', 'depth_std'):
                if (key == 'depth_sup' or key in row.inputs) and batch.get(key) is None:
                    raise L.NerfppError("depth_loss_type %r: the batch has no %s" % (self.loss_type, key))
            sc, g_rgb, g_depth, g_w = ops.loss_and_grads(ret, rgb_gt, None, 'rgbonly', self.lambda_depth)
            if 'weights' in row.reads:        # a loss with a gradient to the weights starts from zeros
                g_w = torch.zeros_like(ret['fg_weights'])
            # onto the zeros of g_depth (and g_w); loss += lambda * value, depth_loss = value, n_valid = supervised rays, on the
            # device.  One group per batch, the mean over the supervised rays; a variance is that of the foreground samples, so the
            # mask takes p < fg_far as kl's does
            _, stats = DL.after(self.loss_type, dict(weights=[ret['fg_weights']], x=[fg_z], pred=[ret['depth']]), depth_sup,
                                [self.lambda_depth], dict(weights=[g_w], pred=[g_depth]),
                                dict(total=sc[0:1], last=sc[2:3], n_sup=sc[3:4]),
                                dict(min_rays=self.ssi_min_rays, norm='supervised', prior_std=batch.get('depth_std'), limit=far))
            if row.stats is not None and hasattr(self, row.stats):      # (this trainer keeps last_gnll_stats only)
                setattr(self, row.stats, (getattr(self, row.stats) if m > 0 else []) + [stats])
        else:
            sc, g_rgb, g_depth, g_w = ops.loss_and_grads(ret, rgb_gt, depth_sup, self.loss_type,
                                                         self.lambda_depth, self.kl_sigma, fg_z, far)
        if ae is not None:                    # ddp_train_nerf.py:472-479
            g_ae = ae.finish(ae_idx, ret['rgb'], batch['rgb'], sc, g_rgb, self.lambda_depth)
            rows = torch.zeros(len(ae.names), 3, device=self.device)
            rows[ae_idx, :2] = g_ae
            rows[ae_idx, 2] = 1.0
            self._ae_grad[m] = rows
            self.last_autoexpo[m] = ae.scale_shift(ae_idx)
        if self.ray_reg is not None:
            # onto g_w (zeros where the loss head has no gradient to the weights); loss += lambda * value on the device.  After
            # auto-exposure, which sees the scalars it saw without the regularisers
            if g_w is None:
                g_w = torch.zeros_like(ret['fg_weights'])
            reg = self.ray_reg.ray_reg(ret['fg_weights'], fg_z, batch['min_depth'].contiguous().float(), far, self.lambda_distortion,
                                       self.lambda_opacity, g_weights=g_w, fold_total=sc[0:1])
            self.last_ray_reg = (self.last_ray_reg if m > 0 else []) + [reg]
        if self.ray_los is not None:
            # beside the depth loss, onto g_w in the same way; one band per step, shared by the levels
            if m == 0:
                self.last_los_sigma = self.los_band(batch)
            if g_w is None:
                g_w = torch.zeros_like(ret['fg_weights'])
            los = self.ray_los.ray_los(ret['fg_weights'], fg_z, far, batch['depth_sup'].contiguous().float(), self.last_los_sigma,
                                       self.lambda_los, g_weights=g_w, fold_total=sc[0:1])
            self.last_ray_los = (self.last_ray_los if m > 0 else []) + [los]
        return sc, g_rgb, g_depth, g_w

    def _fused_scalars(self, ret, batch, depth_sup, fg_z, far):
        """The logged scalars of a level whose loss gradient the compositing backward forms (fuse_loss)"""
        return ops.loss_and_grads(ret, batch['rgb'], depth_sup, self.loss_type, self.lambda_depth, self.kl_sigma, fg_z, far)[0]

    def _backward(self, m, eng, g, ev=None, fused_loss=None):
        """Level m's backward on the current stream.  g = (g_rgb, g_depth, g_w), or three None with fused_loss."""
        eng.backward(*g, grad_scale=1.0 / self.world_size, out=self.grads[m][:L.LEVEL_PARAMS + 1], bad_count=self.bad_cameras,
                     events=ev['bwd'] if ev else None, defer_reduce=True, fused_loss=fused_loss)

    # -- one optimisation step ----------------------------------------------------------------------
    def train_step(self, batch, uniforms=None, events=None):
        """batch: dict of device tensors ray_o, ray_d, rgb, min_depth, [depth_sup], [depth_std].
        uniforms: optional dict t_fg, t_bg [N,S0], u_fg, u_bg [N,S1] (replay); else torch.rand in the
        reference's call order; with depth_guide_samples = G > 0 the replay's u_fg is [N,S1-G] and v_fg [N,G] joins them, drawn in
        the order u_fg, u_bg, v_fg.  events: optional per-level dict of torch.cuda.Event taps.
        Returns per-level scalar tensors [loss, rgb_loss, depth_loss, n_valid] (device, no sync)."""
        self.step_count += 1
        ray_o, ray_d = batch['ray_o'], batch['ray_d']
        u = uniforms or {}
        self.rng_step += 1
        rng = None if (uniforms is not None or self.torch_rng) else (self.seed, self.rng_step)
        # (without rng, sample_coarse draws the jitter it is not given with torch.rand, fg first, as sample_fine_pair does)
        far, fg_z, bg_z = ops.sample_coarse(ray_o, ray_d, batch['min_depth'], self.cascade_samples[0], u.get('t_fg'), u.get('t_bg'),
                                            check=False, rng=rng, bad=self.bad_cameras)
        depth_sup = batch.get('depth_sup') if self.loss_type != 'rgbonly' else None
        scalars, ret, ae_idx = [], None, None
        if self.autoexpo is not None:
            name = batch.get('img_name')
            if name is None and 'frame' in batch:
                name = self.img_names[int(batch['frame'])]
            ae_idx = self.autoexpo[0].lookup(name)
        for m, eng in enumerate(self.engines):
            self._update_end(m)                   # this level's update from the previous step
            if m > 0:
                fg_z, bg_z, mode = self.fine_samples(fg_z, bg_z, ret, batch['min_depth'], far, batch, uniforms, rng)
                if self.depth_guide is not None:
                    self.last_depth_guide = (self.last_depth_guide if m > 1 else [None]) + [mode]
            ev = events[m] if events is not None else None
            ret = eng.forward(ray_o, ray_d, far, fg_z, bg_z, training=True,
                              events=ev['fwd'] if ev else None)
            ae = self.autoexpo[m] if ae_idx is not None else None
            side = contextlib.nullcontext()       # the backward and the update go to the caller's stream, or to the level's own
            fused = loss_done = None
            if ae is None and self.fuse_loss:
                # The loss head's gradient is formed inside the compositing backward (nerfpp_backward_args.fused_loss);
                # the loss launch itself only yields the logged scalars, so it runs on the side stream next to the
                # backward kernels instead of between forward and backward on the critical path.
                g = (None, None, None)
                fused = dict(loss_type=self.loss_type, lambda_depth=self.lambda_depth, kl_sigma=self.kl_sigma,
                             ret=ret, rgb_gt=batch['rgb'], depth_sup=depth_sup)
                if self.update_stream is not None:
                    with self._after_here(self.update_stream):
                        sc = self._fused_scalars(ret, batch, depth_sup, fg_z, far)
                        loss_done = torch.cuda.Event()
                        loss_done.record()
            else:
                sc, *g = self._loss_head(m, ret, batch, depth_sup, fg_z, far, ae, ae_idx)
                if self.concurrent_backward and m + 1 < len(self.engines) and ae is None and events is None and self.update_stream is not None:
                    # Level 1 needs level 0's FORWARD only (its weights, detached: ddp_train_nerf.py:452-457): level 0's backward, weight
                    # gradients and update run on their own stream under level 1's sampling and forward (HBM-bound weight gradients
                    # next to the forward kernels).  Measured: -1.1 % per step; the last level's backward under the NEXT step's
                    # level 0 as well: no further gain (+-0.5 %); level 0's loss head + compositing backward moved to that stream too (25 us off
                    # the path to level 1's forward): 2.331 vs 2.328 ms in one process (round 4) -- the step is bound by the sum of
                    # the work, not by this chain.  _update_end(m) / flush() order later readers.  A step that carries
                    # event taps runs inline, so that a tap times its kernel group alone on the GPU.
                    stream = self.level_streams[m]
                    side = self._after_here(stream)
                    for t in g + [ray_o, ray_d, far, fg_z, bg_z, batch['rgb'], depth_sup] + list(ret.values()):
                        if torch.is_tensor(t):
                            t.record_stream(stream)               # (allocated on this stream, read on the level's)
            with side:
                self._backward(m, eng, g, ev, fused)
                if loss_done is not None:
                    torch.cuda.current_stream().wait_event(loss_done)     # long finished: orders readers of `sc` / frees of `ret`
                elif fused is not None:
                    sc = self._fused_scalars(ret, batch, depth_sup, fg_z, far)
                scalars.append(sc)
                self._update_begin(m)
        return scalars


def batch_to_device(b, device):
    out = {}
    for k, v in b.items():
        if isinstance(v, np.ndarray):
            out[k] = torch.from_numpy(np.ascontiguousarray(v)).to(device)
    return out

#!/usr/bin/env python
"""Measured errors of the HIP path in both precisions against the reference's golden vectors:

  * forward: max relative error of rgb / depth / fg_weights against tests/golden/forward.npz (float32 reference),
  * gradients: per-tensor relative L2 error and max |diff| / RMS against the FLOAT64 run of the reference
    (tests/golden/grads_*.npz; the float32 reference is itself ~1e-1 RMS away from it).

    python tools/grad_error_report.py [--json profiles/r02_bf16_error_report.json] [modes ...]

`measure()` is also what tests/test_gpu_round2.py calls to hold the bf16 kernels to 2x the recorded values.

--at-scale: the HIP backward of all four precisions against the float64 autograd reference of tests/grad_reference64.py, with the
same upstream gradients (the loss head on the kernel's own forward, modes rgbonly / mse / kl), at the training shapes (level 0 at
1024 rays x 64, level 1 at 1024 x 192 with fine depths) and the ragged shapes of tests/test_gpu_parity.py; per parameter tensor
the relative L2 error and max |err| / RMS, the worst over modes and seeds:

    python tools/grad_error_report.py --at-scale [--seeds 0,1,2] [--json profiles/r07_grad_error_at_scale.json]

`measure_at_scale()` is what tests/test_gpu_gradients_at_scale.py holds to 2x the recorded values.
"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
GOLDEN = os.path.join(ROOT, 'tests', 'golden')


def measure(modes=('rgbonly', 'mse', 'l1', 'kl')):
    import torch
    from oracle import nerfpp_oracle as O                     # test infrastructure: parameter init + names only
    from outdoor_nerf_depth_amd import ops
    dev = torch.device('cuda:0')
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    levels = O.init_params_like_reference(2)
    flat = lambda lv: np.concatenate([lv[k].reshape(-1) for k in O.param_order()]).astype(np.float32)
    shapes = {}
    for net, in_ch in (('fg_net', 63), ('bg_net', 84)):
        for k, s in O.mlp_param_shapes(in_ch, 27).items():
            shapes['%s.%s' % (net, k)] = s
    out = {'bf16': {}, 'split': {}}
    names = {1: 'bf16', 2: 'split'}
    gf = np.load(os.path.join(GOLDEN, 'forward.npz'))
    for prec in (2, 1):
        for m, (fz, bz) in enumerate((('fg_z0', 'bg_z0'), ('fg_z1', 'bg_z1'))):
            eng = ops.LevelEngine(T(flat(levels[m])), precision=prec)
            ret = eng.forward(T(gf['ray_o']), T(gf['ray_d']), T(gf['fg_far']), T(gf[fz]), T(gf[bz]))
            for k in ('rgb', 'depth', 'fg_weights', 'bg_lambda'):
                ref = gf['L%d.%s' % (m, k)]
                got = ret[k].cpu().numpy()
                out[names[prec]]['fwd.L%d.%s.max_abs_over_max' % (m, k)] = float(np.abs(got - ref).max() / (np.abs(ref).max() + 1e-30))
    for mode in modes:
        g = np.load(os.path.join(GOLDEN, 'grads_%s.npz' % mode))
        for m in (0, 1):
            for prec in (2, 1):
                eng = ops.LevelEngine(T(flat(levels[m])), precision=prec)
                fz, bz = g['L%d.fg_z' % m], g['L%d.bg_z' % m]
                ret = eng.forward(T(g['ray_o']), T(g['ray_d']), T(g['fg_far']), T(fz), T(bz), training=True)
                sc, g_rgb, g_depth, g_w = ops.loss_and_grads(ret, T(g['rgb_gt']), T(g['depth_sup']), mode,
                                                             float(g['lambda_depth']), kl_sigma=float(g['depth_sigma_scaled']),
                                                             fg_z_vals=T(fz), fg_far_depth=T(g['fg_far']))
                gr = eng.backward(g_rgb, g_depth, g_w).cpu().numpy()
                off = 0
                worst_l2, worst_max = 0.0, 0.0
                for k in O.param_order():
                    n = int(np.prod(shapes[k]))
                    mine = gr[off:off + n][g['L%d.%s.idx' % (m, k)]]
                    ref = g['L%d.%s.g64' % (m, k)]
                    rms = g['L%d.%s.norm64' % (m, k)] / np.sqrt(n) + 1e-12
                    if n > 3:                                  # 1- and 3-element tensors are single cancelling sums
                        worst_l2 = max(worst_l2, float(np.linalg.norm(mine - ref) / (np.linalg.norm(ref) + 1e-30)))
                    worst_max = max(worst_max, float(np.abs(mine - ref).max() / rms))
                    off += n
                out[names[prec]]['grad.%s.L%d.worst_rel_l2' % (mode, m)] = worst_l2
                out[names[prec]]['grad.%s.L%d.worst_max_over_rms' % (mode, m)] = worst_max
                out[names[prec]]['loss.%s.L%d.rel' % (mode, m)] = float(abs(float(sc[0]) - float(g['L%d.loss' % m])) /
                                                                       abs(float(g['L%d.loss' % m])))
    return out


AT_SCALE_PRECISIONS = (('split', 2), ('split_fwd', 12), ('fp16_fwd', 3), ('bf16', 1))     # _lib.PREC_* values
# name -> (level, n_rays, n_samples): the two cascade levels at the training shape, then the ragged sizes of
# tests/test_gpu_parity.py::test_training_ragged_sizes_match_oracle (level-0 parameters, coarse depths)
AT_SCALE_SHAPES = (('L0_1024x64', 0, 1024, 64), ('L1_1024x192', 1, 1024, 192), ('r7x192', 0, 7, 192), ('r33x33', 0, 33, 33),
                   ('r5x64', 0, 5, 64), ('r270x64', 0, 270, 64))
AT_SCALE_MODES = ('rgbonly', 'mse', 'kl')


def scale_case(level, n, S, seed=0):
    """Inputs of one level's training step on the device: dict(params (numpy, by name), batch (numpy), far, fg_z, bg_z (device)).
    n = 1024 / 2048 and S = 64 / 192: the _full_size_case of tests/test_gpu_round2.py (coarse depths from replayed uniforms, fine
    depths from a split-bf16 level-0 forward and sample_fine_pair); any other shape: oracle coarse depths, perturbed."""
    import torch
    from oracle import nerfpp_oracle as O
    from outdoor_nerf_depth_amd import ops
    from outdoor_nerf_depth_amd.synthetic import SyntheticKitti
    dev = torch.device('cuda:0')
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    levels = O.init_params_like_reference(2)
    flat = lambda lv: np.concatenate([lv[k].reshape(-1) for k in O.param_order()]).astype(np.float32)
    if (level == 1 and S == 192) or (level == 0 and S == 64 and n >= 1024):
        b = SyntheticKitti(depth_sup_type='mono_crop').random_batch(n, np.random.RandomState(11 + seed))
        b['depth_sup'][::7] = 0.0
        uni = O.step_uniforms(777 + seed, 1, n, 64, 128)
        far, fg, bg = ops.sample_coarse(T(b['ray_o']), T(b['ray_d']), T(b['min_depth']), 64, t_rand_fg=T(uni['t_fg']),
                                        t_rand_bg=T(uni['t_bg']))
        if level == 1:
            e0 = ops.LevelEngine(T(flat(levels[0])), precision=2)
            r0 = e0.forward(T(b['ray_o']), T(b['ray_d']), far, fg, bg)
            fg, bg = ops.sample_fine_pair(fg, r0['fg_weights'], bg, r0['bg_weights'], 128, u_fg=T(uni['u_fg']),
                                          u_bg=T(uni['u_bg']))
            del e0, r0
    else:
        b = SyntheticKitti(depth_sup_type='mono_crop').random_batch(n, np.random.RandomState(7 * n + S + 1000 * seed))
        b['depth_sup'][: max(1, n // 3)] = np.float32(0.05)
        rs = np.random.RandomState(S + 1000 * seed)
        far_o = O.intersect_sphere(b['ray_o'], b['ray_d'])
        fg_o, bg_o = O.coarse_depths(b['min_depth'], far_o, S)
        far, fg = T(far_o), T(O.perturb_samples(fg_o, rs.rand(n, S).astype(np.float32)))
        bg = T(O.perturb_samples(bg_o, rs.rand(n, S).astype(np.float32)))
    return dict(params=levels[level], flat=flat(levels[level]), batch=b, far=far, fg_z=fg, bg_z=bg)


def upstream(ops, ret, case, mode):
    """(g_rgb, g_depth, g_w) of the loss head on a forward's outputs (g_w: kl only)"""
    import torch
    dev = ret['rgb'].device
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    b = case['batch']
    _, g_rgb, g_depth, g_w = ops.loss_and_grads(ret, T(b['rgb']), T(b['depth_sup']), mode, 0.1, kl_sigma=0.01,
                                                fg_z_vals=case['fg_z'], fg_far_depth=case['far'])
    return g_rgb, g_depth, g_w


def measure_at_scale(seeds=(0, 1, 2), precisions=AT_SCALE_PRECISIONS, shapes=AT_SCALE_SHAPES, modes=AT_SCALE_MODES):
    """{prec: {shape: {tensor: [rel_l2, max_over_rms]}}}, worst over `modes` and `seeds`; prec 'torch_f32': the float32 torch
    autograd of the same restatement (tests/grad_reference64.py), i.e. what plain float32 arithmetic of the gradient reaches."""
    import torch
    from outdoor_nerf_depth_amd import ops
    from tests import grad_reference64 as R
    dev = torch.device('cuda:0')
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    out = {p: {} for p, _ in precisions}
    for seed in seeds:
        for shape, level, n, S in shapes:
            case = scale_case(level, n, S, seed)
            b = case['batch']
            for pname, prec in precisions:
                eng = ops.LevelEngine(T(case['flat']), precision=prec)
                ret = eng.forward(T(b['ray_o']), T(b['ray_d']), case['far'], case['fg_z'], case['bg_z'], training=True)
                for mode in modes:
                    g_rgb, g_depth, g_w = upstream(ops, ret, case, mode)
                    got = R.flat_to_dict(eng.backward(g_rgb, g_depth, g_w).double().cpu().numpy())
                    ref = R.level_grads64(case['params'], T(b['ray_o']), T(b['ray_d']), case['far'], case['fg_z'], case['bg_z'],
                                          g_rgb, g_depth, g_w)
                    rec = out[pname].setdefault(shape, {})
                    for k, (rel, mx) in R.errors(got, ref).items():
                        old = rec.get(k, [0.0, 0.0])
                        rec[k] = [max(old[0], rel), max(old[1], mx)]
                del eng, ret
            # float32 autograd of the same gradient (upstream gradients of the split-bf16 forward): the conditioning floor
            eng = ops.LevelEngine(T(case['flat']), precision=2)
            ret = eng.forward(T(b['ray_o']), T(b['ray_d']), case['far'], case['fg_z'], case['bg_z'], training=True)
            for mode in modes:
                g = upstream(ops, ret, case, mode)
                args = (case['params'], T(b['ray_o']), T(b['ray_d']), case['far'], case['fg_z'], case['bg_z']) + g
                rec = out.setdefault('torch_f32', {}).setdefault(shape, {})
                for k, (rel, mx) in R.errors(R.level_grads64(*args, dtype=torch.float32), R.level_grads64(*args)).items():
                    old = rec.get(k, [0.0, 0.0])
                    rec[k] = [max(old[0], rel), max(old[1], mx)]
            del eng, ret, case
            torch.cuda.empty_cache()
    return out


def at_scale_main(args):
    import time
    from outdoor_nerf_depth_amd import _lib as L
    path = None
    if '--json' in args:
        path = args[args.index('--json') + 1]
    seeds = (0, 1, 2)
    if '--seeds' in args:
        seeds = tuple(int(v) for v in args[args.index('--seeds') + 1].split(','))
    t0 = time.time()
    res = measure_at_scale(seeds)
    wall = time.time() - t0
    for pname, shapes in res.items():
        for shape, tensors in shapes.items():
            rel = max(v[0] for v in tensors.values())
            rel_big = max(v[0] for k, v in tensors.items() if not k.endswith(('sigma_layers.0.bias', 'rgb_layers.2.bias')))
            mx = max(v[1] for v in tensors.values())
            print('%-10s %-12s worst rel-L2 %.3e (tensors > 3 elements %.3e)  worst max/RMS %.3e' % (pname, shape, rel, rel_big, mx))
    ws = {'%dx%d' % (n, S): {'prec%d' % p: int(L.lib().nerfpp_workspace_bytes(n, S, p, 1)) for p in (1, 2, 3)}
          for n, S in ((1024, 64), (1024, 192), (2048, 192))}
    print('training workspace bytes:', json.dumps(ws))
    print('wall %.1f s for seeds %s' % (wall, seeds))
    if path:
        res = dict(errors=res, seeds=list(seeds), modes=list(AT_SCALE_MODES), workspace_bytes=ws, wall_s=round(wall, 1),
                   _doc=('measured on MI355X by tools/grad_error_report.py --at-scale: per parameter tensor [relative L2 error, '
                         'max |err| / RMS] of the HIP backward against the float64 autograd reference (tests/grad_reference64.py) '
                         'with the same upstream gradients, worst over the modes and seeds; precisions by name '
                         '(split = PREC_SPLIT_BF16, split_fwd = PREC_SPLIT_FWD, fp16_fwd = PREC_FP16_FWD, bf16 = PREC_BF16; torch_f32 = the '
                         'float32 torch autograd of the same gradient)'))
        with open(path, 'w') as f:
            json.dump(res, f, indent=0, sort_keys=True)


if __name__ == '__main__' and '--at-scale' in sys.argv[1:]:
    at_scale_main(sys.argv[1:])
elif __name__ == '__main__':
    args = sys.argv[1:]
    path = None
    if '--json' in args:
        i = args.index('--json')
        path = args[i + 1]
        del args[i:i + 2]
    res = measure(tuple(args) or ('rgbonly', 'mse', 'l1', 'kl'))
    for prec in ('split', 'bf16'):
        print('== %s' % prec)
        for k, v in sorted(res[prec].items()):
            print('  %-44s %.3e' % (k, v))
    if path:
        res['_doc'] = ('measured on MI355X by tools/grad_error_report.py: forward max|diff|/max|ref| vs the float32 reference, '
                       'gradient worst-tensor relative L2 and max|diff|/RMS vs the float64 run of the reference')
        with open(path, 'w') as f:
            json.dump(res, f, indent=1, sort_keys=True)

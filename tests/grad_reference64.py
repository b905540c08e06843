"""Float64 reference for one cascade level's parameter gradients, shared by the CPU test that pins it
(tests/test_grad_reference64.py) and the GPU tests / measurement that hold the HIP backward to it
(tests/test_gpu_gradients_at_scale.py, tools/grad_error_report.py --at-scale).

    level_grads64(params, ray_o, ray_d, fg_far, fg_z, bg_z, g_rgb, g_depth, g_w)
        = d/d theta  sum(g_rgb * rgb + g_depth * depth + g_w * fg_weights)

with torch autograd in float64 through oracle/nerfpp_torch_cpu.nerf_forward (pinned to the numpy oracle), on the device of
`ray_o` (numpy inputs: the CPU), chunked over rays.  The gradient is a sum over rays, so the chunks' float64 gradients add up to
the whole batch's and 196 608 rows fit in a few GB.  The upstream gradients are constants here: the caller takes them from the
loss head of whichever forward it is checking, and hands the same values to the HIP backward.
"""
from collections import OrderedDict

import numpy as np
import torch

from oracle import nerfpp_oracle as O
from oracle import nerfpp_torch_cpu as TC

ROWS_PER_CHUNK = 16384          # ~1.5 GB of float64 activations + autograd state per chunk


def _t64(a, device, dtype=torch.float64):
    if isinstance(a, torch.Tensor):
        return a.detach().to(device=device, dtype=dtype)
    return torch.from_numpy(np.ascontiguousarray(a)).to(device=device, dtype=dtype)


def level_grads64(params, ray_o, ray_d, fg_far, fg_z, bg_z, g_rgb, g_depth, g_w=None, chunk_rays=None, dtype=torch.float64):
    """params: {name: array or tensor} of one level (names of O.param_order()); ray_o / ray_d [n,3], fg_far [n], fg_z / bg_z [n,S],
    g_rgb [n,3], g_depth [n], g_w [n,S] or None.  chunk_rays: rays per autograd pass (default: ROWS_PER_CHUNK rows).
    Returns an OrderedDict in O.param_order() of float64 tensors on the inputs' device.  dtype=torch.float32: the same autograd
    in float32 (accumulated in float64): how far plain float32 arithmetic of this gradient lands from float64."""
    device = ray_o.device if isinstance(ray_o, torch.Tensor) else torch.device('cpu')
    p = OrderedDict((k, _t64(params[k], device, dtype).requires_grad_(True)) for k in O.param_order())
    n, S = fg_z.shape
    if chunk_rays is None:
        chunk_rays = max(1, ROWS_PER_CHUNK // S)
    ins = [_t64(a, device, dtype) for a in (ray_o, ray_d, fg_far, fg_z, bg_z, g_rgb, g_depth)]
    gw = _t64(g_w, device, dtype) if g_w is not None else None
    acc = OrderedDict((k, torch.zeros_like(v, dtype=torch.float64, requires_grad=False)) for k, v in p.items())
    for r0 in range(0, n, chunk_rays):
        sl = slice(r0, min(n, r0 + chunk_rays))
        o, d, far, fz, bz, gr, gd = [a[sl] for a in ins]
        ret = TC.nerf_forward(p, o, d, far, fz, bz)
        s = (gr * ret['rgb']).sum() + (gd * ret['depth']).sum()
        if gw is not None:
            s = s + (gw[sl] * ret['fg_weights']).sum()
        for k, g in zip(p, torch.autograd.grad(s, list(p.values()))):
            acc[k] += g
    return acc


def flat_to_dict(vec):
    """Split a flat level gradient / parameter vector (NerfNet.parameters() order) into {name: array} of the reference shapes."""
    shapes = OrderedDict()
    for net, in_ch in (('fg_net', O.FG_IN), ('bg_net', O.BG_IN)):
        for k, s in O.mlp_param_shapes(in_ch, O.DIR_IN).items():
            shapes['%s.%s' % (net, k)] = s
    out, off = OrderedDict(), 0
    for k in O.param_order():
        m = int(np.prod(shapes[k]))
        out[k] = vec[off:off + m].reshape(shapes[k])
        off += m
    assert off == vec.shape[0] or off + 1 == vec.shape[0], (off, vec.shape)
    return out


def errors(got, ref):
    """{name: (rel-L2, max|err| / RMS)} of got against ref (float64; dicts of arrays or tensors)."""
    out = OrderedDict()
    for k in O.param_order():
        g = got[k].detach().double().cpu().numpy() if isinstance(got[k], torch.Tensor) else np.asarray(got[k], np.float64)
        r = ref[k].detach().double().cpu().numpy() if isinstance(ref[k], torch.Tensor) else np.asarray(ref[k], np.float64)
        g, r = g.reshape(-1), r.reshape(-1)
        rn = np.linalg.norm(r)
        rms = rn / np.sqrt(r.size)
        out[k] = (float(np.linalg.norm(g - r) / (rn + 1e-300)), float(np.abs(g - r).max() / (rms + 1e-300)))
    return out

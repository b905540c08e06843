"""Float64 restatements, per-element error bounds and input families for the non-MLP kernels of the NeRF++ path
(csrc/nerfpp_render.hip: composite_fwd_kernel, composite_bwd_kernel, loss_kernel, kl_terms_kernel, sphere_far /
intersect_sphere_kernel / sample_coarse_kernel; csrc/nerfpp_optim.hip: adam_kernel), for tests/test_nerfpp_render_reference.py (CPU)
and tests/test_gpu_nerfpp_render_edges.py (GPU).  Plain numpy; torch on the CPU only in composite_backward64 (float64 autograd).
Nothing here touches the code under test.

Every bound is absolute and is built from magnitudes of the inputs: a relative bound holds for no correct float32 implementation of
a quantity that cancels (1 - e, 1 - pn, the suffix-sum difference in d_a, m in Adam).  U = 2^-24 is the unit roundoff of float32,
gamma(k) = (1 + U)^k - 1 what k roundings in a row do to a product or to a sum of same-signed terms.  A fused multiply-add drops one
rounding of a count, so every bound admits a compiler that contracts a * b + c.  Division and square root are correctly rounded;
expf and logf on the device are admitted EXP_ULPS = LOG_ULPS = 2 ulp (4 U relative; numpy's are correctly rounded).  A result below
2^-126 may be flushed to 0 (FLUSH).  A sum of k terms may be taken in any fixed order: k roundings on any term.

Each bound function multiplies its derived bound by ONE leading constant C[name].  The constants were calibrated on the CPU against
float32 implementations of the reference's arithmetic (oracle.nerfpp_oracle.nerf_forward's compositing and composite_backward fed with
the same raw values, loss_and_grads, intersect_sphere; float32 torch.optim.Adam) -- never against the HIP kernels: F32_WORST[name] is the
worst |error| / bound of those implementations over all cases below with the constant at 1, and C[name] is the smallest power of two
that is at least 4 F32_WORST[name] (the 4 covers the device's 1-2 ulp expf / logf and a different but fixed summation order across 64
lanes).  tests/test_nerfpp_render_reference.py re-measures the ratios and asserts the rule.

Known distance of adam64 from torch.optim.Adam with exact double constants (documented, not a rounding error): the launcher hands the
kernel (float)(1 - beta1) = 0.1 (1 + 1.49e-8), (float)beta2 = 0.999 (1 + 1.29e-8), (float)(1 - beta2) = 0.001 (1 + 4.75e-8),
(float)eps = 1e-8 (1 - 6.1e-9), and (float)(lr / bias1), (float)sqrt(bias2), which depend on the step (at step 1: 1 - 2.24e-8 and
1 - 5.38e-8 of the double values).  Each is within U = 5.96e-8 of its double value, so m' - m and v' of one step are at most 1.5e-8 and
6.1e-8 (relative) from the exact-constant update and the step at most 1.4e-7 of its size: below the bounds of adam_bounds, which are
taken against adam64 with the launcher's constants.  adam_constants(exact=True) are the double constants; adam_constant_distance()
returns the largest of the figures and the CPU test asserts they stay below ADAM_CONSTANT_DISTANCE."""
import zlib

import numpy as np

U = 2.0 ** -24                      # unit roundoff of float32
FLUSH = 2.0 ** -126                 # smallest normal float32: what a flushed result can lose
DENORM = 2.0 ** -149                # smallest float32
TINY = float(np.float32(1e-6))      # utils.py:8 TINY_NUMBER as float32 holds it
HUGE = 1e10                         # utils.py:7 HUGE_NUMBER (exact in float32)
KL_EPS = float(np.float32(1e-5))
EXP_ULPS = 2
LOG_ULPS = 2
ADAM_CONSTANT_DISTANCE = 2.0 ** -24

# worst |error| / bound of the float32 implementations of the reference's arithmetic, constant at 1 (CPU calibration), and the
# constants that follow from them: smallest power of two >= 4 * worst
F32_WORST = {
    'fg_dists': 0.4696, 'fg_weights': 0.3705, 'bg_weights': 0.3705, 'bg_lambda': 0.1948, 'fg_rgb': 0.2195, 'bg_rgb': 0.2131,
    'rgb': 0.1872, 'fg_depth': 0.2912, 'bg_depth': 0.1888, 'depth': 0.1740, 'dout_rgb': 0.3906, 'dout_sigma': 0.1286,
    'loss': 0.4571, 'rgb_loss': 0.4571, 'depth_loss': 0.4615, 'g_rgb': 0.9485, 'g_depth': 0.9922, 'g_w': 0.5712,
    'adam_p': 1.0, 'adam_m': 0.5500, 'adam_v': 0.4899, 'sphere_far': 0.1977,
}


def pow2_at_least(x):
    """smallest power of two >= x (x > 0)"""
    return 2.0 ** int(np.ceil(np.log2(x)))


C = {k: pow2_at_least(4 * v) for k, v in F32_WORST.items()}


def f64(a):
    return np.asarray(a, np.float64)


def f32r(x):
    """a Python float as a kernel receives it: rounded to float32, held in a double"""
    return float(np.float32(x))


def gamma(k):
    return (1.0 + U) ** k - 1.0


def ratio(got, want, bound):
    """|got - want| / bound per element; an element that is not finite where the reference is, or off where the bound is 0,
    counts as inf (a NaN must not pass a comparison by being unordered)."""
    got, want, bound = f64(got), f64(want), f64(bound) + np.zeros_like(f64(want))
    with np.errstate(invalid='ignore'):
        err = np.abs(got - want)
    with np.errstate(divide='ignore', invalid='ignore'):
        r = np.where(err == 0, 0.0, err / bound)
    return np.where(np.isfinite(got) | ~np.isfinite(want), np.nan_to_num(r, nan=np.inf), np.inf)


def prod_bound(a, da, b, db, roundings=1):
    """|a' b' (1 + d) - a b| for |a' - a| <= da, |b' - b| <= db, |d| <= gamma(roundings)"""
    a, b = np.abs(a), np.abs(b)
    return da * (b + db) + a * db + gamma(roundings) * (a + da) * (b + db)


# ------------------------------------------------------------------------------------------------------------ compositing
RET_KEYS = ('rgb', 'depth', 'fg_weights', 'bg_weights', 'fg_dists', 'fg_rgb', 'fg_depth', 'bg_rgb', 'bg_depth', 'bg_lambda')
_IN_KEYS = ('raw_fg', 'raw_bg', 'depth_real_bg', 'ray_d', 'fg_far', 'fg_z', 'bg_z')


def _shape(case):
    n, S = np.shape(case['fg_z'])
    return n, S


def _volumes(case):
    """The per-sample quantities of both volumes in float64 on the float32 inputs (oracle.nerfpp_oracle.nerf_forward lines 436-478),
    background in the FLIPPED order the compositing runs in, each with the error a float32 evaluation may carry:
      dnorm = |ray_d|: 3 products, 2 sums, 1 square root: gamma(4) (the root halves the first five)
      dist: fg dnorm (z[i+1] - z[i]): the difference of two float32 numbers is rounded once, the product once: gamma(6) dist;
            bg z[s] - z[s-1]: gamma(1); the last one is 1e10, exact
      x = |sigma| dist: 1 more.  e = exp(-x): e (rel(x) x + 2 EXP_ULPS U) + DENORM  (x e^-x <= 1 / e, so this is at most a few U)
      alpha = 1 - e: d_e + U        q = (1 - alpha) + TINY: d_e + 3 U (alpha's rounding, 1 - alpha is exact below 1/2 and 1 U above, the sum)
        -- absolute: next to q = TINY three roundoffs of 1 are 18 % of q, which is what float32 does there (alpha rounds to 1)
      T[i] = prod_{j<i} q[j]: between prod (q - d_q) and prod (q + d_q), times (1 + U)^i for the products in any order, + S FLUSH
      w = alpha T: prod_bound"""
    n, S = _shape(case)
    raw_fg, raw_bg = f64(case['raw_fg']).reshape(n, S, 4), f64(case['raw_bg']).reshape(n, S, 4)[:, ::-1]
    zr = f64(case['depth_real_bg']).reshape(n, S)[:, ::-1]
    d = f64(case['ray_d'])
    dnorm = np.sqrt((d * d).sum(-1))[:, None]
    fg_z, bg_zf = f64(case['fg_z']), f64(case['bg_z'])[:, ::-1]
    vols = []
    for bg in (False, True):
        if bg:
            dist = np.concatenate([bg_zf[:, :-1] - bg_zf[:, 1:], np.full((n, 1), HUGE)], -1)
            d_dist = gamma(1) * np.abs(dist)
            d_dist[:, -1] = 0.0
            raw, zval = raw_bg, zr
        else:
            dist = dnorm * np.concatenate([fg_z[:, 1:] - fg_z[:, :-1], f64(case['fg_far'])[:, None] - fg_z[:, -1:]], -1)
            d_dist = gamma(6) * np.abs(dist) + FLUSH
            raw, zval = raw_fg, fg_z
        sraw = raw[..., 3]
        sigma = np.abs(sraw)
        x = sigma * dist
        rel_x = np.where(dist != 0, d_dist / np.where(dist != 0, np.abs(dist), 1.0), 0.0) + U
        with np.errstate(under='ignore'):
            e = np.exp(-x)
        d_e = np.where(x == 0, 0.0, e * (rel_x * np.abs(x) + 2 * EXP_ULPS * U) + DENORM)
        alpha = -np.expm1(-x)
        d_alpha = np.where(x == 0, 0.0, d_e + U)
        q = e + TINY
        d_q = d_e + 3 * U
        ones = np.ones((n, 1))
        T_all = np.cumprod(q, -1)
        T_hi = np.cumprod(q + d_q, -1) * (1 + U) ** np.arange(1, S + 1)
        T = np.concatenate([ones, T_all[:, :-1]], -1)
        d_T = np.concatenate([0 * ones, (T_hi - T_all)[:, :-1]], -1) + S * FLUSH
        d_T[:, 0] = 0.0
        w = alpha * T
        d_w = prod_bound(alpha, d_alpha, T, d_T) + FLUSH
        d_w = np.where(alpha == 0, 0.0, d_w)
        vols.append(dict(dist=dist, d_dist=d_dist, sraw=sraw, e=e, d_e=d_e, alpha=alpha, d_alpha=d_alpha, q=q, d_q=d_q, T=T, d_T=d_T,
                         w=w, d_w=d_w, c=raw[..., :3], zval=zval, lam=T_all[:, -1], d_lam=(T_hi - T_all)[:, -1] + S * FLUSH))
    return vols


def _wsum(v, vals):
    """sum_i w_i vals_i and its bound: every w's own error, 1 product and S sums in any order on magnitudes"""
    S = v['w'].shape[1]
    mag = (v['w'] + v['d_w']) * np.abs(vals)
    return (v['w'] * vals).sum(1), (v['d_w'] * np.abs(vals)).sum(1) + gamma(S + 1) * mag.sum(1) + FLUSH


def _composite_all(case):
    fg, bg = _volumes(case)
    out, bnd, aux = {}, {}, {}
    out['fg_dists'], bnd['fg_dists'] = fg['dist'], fg['d_dist']
    out['fg_weights'], bnd['fg_weights'] = fg['w'], fg['d_w']
    out['bg_weights'], bnd['bg_weights'] = bg['w'], bg['d_w']
    lam, d_lam = fg['lam'], fg['d_lam']
    out['bg_lambda'], bnd['bg_lambda'] = lam, d_lam
    f_rgb = [_wsum(fg, fg['c'][..., k]) for k in range(3)]
    b_rgb = [_wsum(bg, bg['c'][..., k]) for k in range(3)]
    f_dep, b_dep = _wsum(fg, fg['zval']), _wsum(bg, bg['zval'])
    out['fg_rgb'], bnd['fg_rgb'] = np.stack([t[0] for t in f_rgb], -1), np.stack([t[1] for t in f_rgb], -1)
    out['fg_depth'], bnd['fg_depth'] = f_dep
    braw, d_braw = np.stack([t[0] for t in b_rgb], -1), np.stack([t[1] for t in b_rgb], -1)
    out['bg_rgb'], bnd['bg_rgb'] = lam[:, None] * braw, prod_bound(lam[:, None], d_lam[:, None], braw, d_braw) + FLUSH
    out['bg_depth'], bnd['bg_depth'] = lam * b_dep[0], prod_bound(lam, d_lam, b_dep[0], b_dep[1]) + FLUSH
    for k, a, b in (('rgb', 'fg_rgb', 'bg_rgb'), ('depth', 'fg_depth', 'bg_depth')):
        out[k] = out[a] + out[b]
        bnd[k] = bnd[a] + bnd[b] + U * (np.abs(out[a]) + bnd[a] + np.abs(out[b]) + bnd[b])
    aux.update(fg=fg, bg=bg, bg_rgb_raw=(braw, d_braw), bg_depth_raw=b_dep)
    return out, bnd, aux


def composite64(raw_fg, raw_bg, depth_real_bg, ray_d, fg_far, fg_z, bg_z):
    """The ten outputs of the compositing in float64 on the float32 inputs; bg_weights in the flipped order the reference returns"""
    return _composite_all(dict(zip(_IN_KEYS, (raw_fg, raw_bg, depth_real_bg, ray_d, fg_far, fg_z, bg_z))))[0]


def composite_bounds(case):
    """{output: C[output] * its bound}, one bound function per output, all from _volumes"""
    return {k: C[k] * b for k, b in _composite_all(case)[1].items()}


def composite64_torch(case, torch):
    """composite64 restated on float64 torch tensors (for autograd): returns (rgb, depth, fg_weights) and the two raw leaves"""
    n, S = _shape(case)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(f64(a)))
    raw_fg, raw_bg = t(case['raw_fg']).reshape(n, S, 4).requires_grad_(), t(case['raw_bg']).reshape(n, S, 4).requires_grad_()
    d = t(case['ray_d'])
    dnorm = (d * d).sum(-1, keepdim=True).sqrt()
    fg_z, bg_z = t(case['fg_z']), t(case['bg_z'])
    ones = torch.ones(n, 1, dtype=torch.float64)

    def volume(raw, dist, zval):
        e = torch.exp(-raw[..., 3].abs() * dist)
        alpha = 1 - e
        T_all = torch.cumprod(e + TINY, -1)
        w = alpha * torch.cat([ones, T_all[:, :-1]], -1)
        return w, (w[..., None] * raw[..., :3]).sum(1), (w * zval).sum(1), T_all[:, -1]

    fg_dist = dnorm * torch.cat([fg_z[:, 1:] - fg_z[:, :-1], t(case['fg_far'])[:, None] - fg_z[:, -1:]], -1)
    w_fg, fg_rgb, fg_depth, lam = volume(raw_fg, fg_dist, fg_z)
    bg_zf = bg_z.flip(1)
    bg_dist = torch.cat([bg_zf[:, :-1] - bg_zf[:, 1:], HUGE * ones], -1)
    _, bg_rgb, bg_depth, _ = volume(raw_bg.flip(1), bg_dist, t(case['depth_real_bg']).reshape(n, S).flip(1))
    return fg_rgb + lam[:, None] * bg_rgb, fg_depth + lam * bg_depth, w_fg, raw_fg, raw_bg


def composite_backward64(case, g_rgb, g_depth, g_w=None):
    """d/d raw of sum(g_rgb rgb) + sum(g_depth depth) + sum(g_w fg_weights) by float64 autograd of composite64_torch, then through the
    sigmoid's derivative c (1 - c) for the colours (raw holds the colours after the sigmoid) and sign(sigma_raw), sign(0) = 0, for
    sigma (torch's abs has that subgradient).  Returns (dout_fg, dout_bg) [n*S, 4] in natural sample order."""
    import torch
    rgb, depth, w_fg, raw_fg, raw_bg = composite64_torch(case, torch)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(f64(a)))
    obj = (t(g_rgb) * rgb).sum() + (t(g_depth) * depth).sum()
    if g_w is not None:
        obj = obj + (t(g_w) * w_fg).sum()
    grads = torch.autograd.grad(obj, (raw_fg, raw_bg))
    outs = []
    for raw, g in zip((raw_fg, raw_bg), grads):
        raw, g = raw.detach().numpy(), g.numpy().copy()
        c = raw[..., :3]
        g[..., :3] *= c * (1 - c)
        g[..., 3] = np.where(raw[..., 3] == 0, 0.0, g[..., 3])
        outs.append(g.reshape(-1, 4))
    return outs[0], outs[1]


def _volume_backward_bound(v, gC, d_gC, gD, d_gD, g_w, X, d_X):
    """Bounds of one volume's (d rgb [.., 3], d sigma_raw): with gw_i = gC . c_i + gD z_i + g_w_i, term_i = gw_i w_i,
      d_a = gw T - (sum_{k>i} term_k + X) / q,   d sigma_raw = sign d_a dist e,   d rgb = w gC c (1 - c)
    (X = g_lam lam in the foreground, 0 in the background).  Every step carries its operands' bounds and its own roundings on
    magnitudes; the quotient by q uses q - d_q (d_q may be 18 % of q at q = TINY); 1 - c of a float32 c is rounded once."""
    S = v['w'].shape[1]
    c, z = v['c'], v['zval']
    A_gw = (np.abs(gC)[:, None, :] * np.abs(c)).sum(-1) + np.abs(gD)[:, None] * np.abs(z) + np.abs(g_w)
    gw = (gC[:, None, :] * c).sum(-1) + gD[:, None] * z + g_w
    d_gw = gamma(8) * A_gw + (d_gC[:, None, :] * np.abs(c)).sum(-1) * (1 + gamma(8)) + d_gD[:, None] * np.abs(z) * (1 + gamma(8)) + FLUSH
    term = gw * v['w']
    d_term = prod_bound(gw, d_gw, v['w'], v['d_w']) + FLUSH
    mag = np.abs(term) + d_term
    suf = lambda a: np.concatenate([np.cumsum(a[:, ::-1], -1)[:, ::-1][:, 1:], np.zeros((a.shape[0], 1))], -1)
    suffix, d_suffix = suf(term), suf(d_term) + gamma(S) * suf(mag)
    N = suffix + X[:, None]
    d_N = d_suffix + d_X[:, None] + U * (np.abs(suffix) + d_suffix + np.abs(X)[:, None] + d_X[:, None])
    q, d_q = v['q'], v['d_q']
    Y = N / q
    d_Y = (d_N * q + np.abs(N) * d_q) / (q * (q - d_q))
    d_Y = d_Y + U * (np.abs(Y) + d_Y)
    P = gw * v['T']
    d_P = prod_bound(gw, d_gw, v['T'], v['d_T']) + FLUSH
    d_a = P - Y
    d_da = d_P + d_Y + U * (np.abs(P) + d_P + np.abs(Y) + d_Y)
    de = v['dist'] * v['e']
    d_de = prod_bound(v['dist'], v['d_dist'], v['e'], v['d_e'])
    b_sigma = np.where(v['sraw'] == 0, 0.0, prod_bound(d_a, d_da, de, d_de) + FLUSH)
    wg = v['w'][..., None] * gC[:, None, :]
    d_wg = prod_bound(v['w'][..., None], v['d_w'][..., None], gC[:, None, :], d_gC[:, None, :])
    cc = c * (1 - c)
    b_rgb = prod_bound(wg, d_wg, cc, gamma(2) * np.abs(cc), 1) + FLUSH
    b_rgb = np.where((cc == 0) | (gC[:, None, :] == 0) & (d_gC[:, None, :] == 0), 0.0, b_rgb)
    return b_rgb, b_sigma


def composite_backward_bounds(case, g_rgb, g_depth, g_w=None):
    """(bound of dout_fg, bound of dout_bg) [n*S, 4], natural sample order: columns 0..2 times C['dout_rgb'], column 3 times
    C['dout_sigma'].  g_lam = g_rgb . bg_rgb_raw + g_depth bg_depth_raw from the forward's background sums and their bounds."""
    n, S = _shape(case)
    _, _, aux = _composite_all(case)
    fg, bg = aux['fg'], aux['bg']
    gC, gD = f64(g_rgb), f64(g_depth)
    g_w = np.zeros((n, S)) if g_w is None else f64(g_w)
    braw, d_braw = aux['bg_rgb_raw']
    bdep, d_bdep = aux['bg_depth_raw']
    g_lam = (gC * braw).sum(-1) + gD * bdep
    A = (np.abs(gC) * (np.abs(braw) + d_braw)).sum(-1) + np.abs(gD) * (np.abs(bdep) + d_bdep)
    d_glam = (np.abs(gC) * d_braw).sum(-1) + np.abs(gD) * d_bdep + gamma(5) * A + FLUSH
    lam, d_lam = fg['lam'], fg['d_lam']
    X, d_X = g_lam * lam, prod_bound(g_lam, d_glam, lam, d_lam) + FLUSH
    zero = np.zeros(n)
    f_rgb, f_sigma = _volume_backward_bound(fg, gC, 0 * gC, gD, zero, g_w, X, d_X)
    gCb, d_gCb = lam[:, None] * gC, prod_bound(lam[:, None], d_lam[:, None], gC, 0 * gC) + FLUSH * (gC != 0)
    gDb, d_gDb = lam * gD, prod_bound(lam, d_lam, gD, zero) + FLUSH * (gD != 0)
    b_rgb, b_sigma = _volume_backward_bound(bg, gCb, d_gCb, gDb, d_gDb, np.zeros((n, S)), zero, zero)
    out_fg = np.concatenate([C['dout_rgb'] * f_rgb, C['dout_sigma'] * f_sigma[..., None]], -1).reshape(-1, 4)
    out_bg = np.concatenate([C['dout_rgb'] * b_rgb, C['dout_sigma'] * b_sigma[..., None]], -1)[:, ::-1].reshape(-1, 4)
    return out_fg, out_bg


# ------------------------------------------------------------------------------------------------------------ loss head
def loss64(loss_type, lambda_depth, kl_sigma, rgb, rgb_gt, depth, depth_sup, fg_weights, fg_z, fg_dists, fg_far):
    """The loss head of ddp_train_nerf.py:481-493 in float64 on the float32 inputs, types 0 rgb only, 1 mse, 2 l1, 3 kl; lambda_depth
    and kl_sigma as the floats the kernel receives.  KL mask 0 < gt < fg_far, divided by S; the mse / l1 normaliser is the number of
    rays with gt > 0, and an empty mask there gives NaN scalars and zero gradients.
    Returns dict(loss, rgb_loss, depth_loss, n_valid, g_rgb, g_depth, g_w) and dict of bounds under the same keys."""
    rgb, gt_rgb = f64(rgb), f64(rgb_gt)
    n = rgb.shape[0]
    S = np.shape(fg_weights)[1]
    lam = f32r(lambda_depth)
    d = rgb - gt_rgb
    o, b = {}, {}
    o['rgb_loss'] = (d * d).sum() / (3.0 * n)
    b['rgb_loss'] = gamma(4) * o['rgb_loss'] + FLUSH            # d, d d, the cast of the double mean (sums in double)
    o['g_rgb'] = 2.0 * d / (3.0 * n)
    b['g_rgb'] = gamma(2) * np.abs(o['g_rgb']) + FLUSH          # d, the division (2 d is exact)
    o['g_depth'], b['g_depth'] = np.zeros(n), np.zeros(n)
    o['g_w'], b['g_w'] = np.zeros((n, S)), np.zeros((n, S))
    o['depth_loss'], b['depth_loss'], o['n_valid'] = 0.0, 0.0, 0.0
    if loss_type in (1, 2):
        gt, z = f64(depth_sup), f64(depth)
        m = gt > 0
        cnt = float(m.sum())
        o['n_valid'] = cnt
        r = np.where(m, z - gt, 0.0)
        if cnt == 0:
            o['depth_loss'] = np.nan
        elif loss_type == 1:
            o['depth_loss'] = (r * r).sum() / cnt
            b['depth_loss'] = gamma(4) * o['depth_loss'] + FLUSH
            o['g_depth'] = lam * 2.0 * r / cnt
            b['g_depth'] = gamma(3) * np.abs(o['g_depth']) + FLUSH * m      # d, the product, the division
        else:
            o['depth_loss'] = np.abs(r).sum() / cnt
            b['depth_loss'] = gamma(2) * o['depth_loss'] + FLUSH
            o['g_depth'] = lam * np.sign(r) / cnt
            b['g_depth'] = gamma(1) * np.abs(o['g_depth'])
    elif loss_type == 3:
        gt, far = f64(depth_sup), f64(fg_far)
        m = (gt > 0) & (gt < far)
        o['n_valid'] = float(m.sum())
        w, z, dists = f64(fg_weights) + KL_EPS, f64(fg_z), f64(fg_dists)
        sig = f32r(kl_sigma)
        arg = (z - gt[:, None]) ** 2 / (2.0 * sig)
        with np.errstate(under='ignore'):
            e = np.exp(-arg)
        lg = -np.log(w)
        # w + 1e-5: 1 rounding, so log moves by U and logf adds LOG_ULPS ulp of itself; arg: z - gt, its square, 1 / (2 sigma),
        # the product: gamma(6) arg; expf; the two products
        d_lg = 2 * U + 2 * LOG_ULPS * U * np.abs(lg)
        d_e = e * (gamma(6) * arg + 2 * EXP_ULPS * U) + DENORM
        term = lg * e * dists
        d_term = (prod_bound(lg, d_lg, e, d_e) * np.abs(dists) + gamma(1) * np.abs(term)) + FLUSH
        ray = np.where(m, term.sum(1), 0.0)
        d_ray = np.where(m, d_term.sum(1) + U * np.abs(term).sum(1), 0.0)                # the per-ray sum's cast to float
        o['depth_loss'] = ray.sum() / S
        b['depth_loss'] = d_ray.sum() / S + U * np.abs(ray).sum() / S + FLUSH
        g = -lam * e * dists / (w * S)
        o['g_w'] = np.where(m[:, None], g, 0.0)
        b['g_w'] = np.where(m[:, None], np.abs(lam) * d_e * np.abs(dists) / (w * S) * (1 + gamma(5)) + gamma(5) * np.abs(g) + FLUSH * (g != 0), 0.0)
    if loss_type == 0:
        o['loss'], b['loss'] = o['rgb_loss'], b['rgb_loss']
    else:
        o['loss'] = o['rgb_loss'] + lam * o['depth_loss']
        mag = abs(o['rgb_loss']) + abs(lam * o['depth_loss'])
        b['loss'] = b['rgb_loss'] + abs(lam) * b['depth_loss'] + gamma(2) * (mag + b['rgb_loss'] + abs(lam) * b['depth_loss']) + FLUSH
    b = {k: C[k] * v for k, v in b.items()}
    return o, b


# ------------------------------------------------------------------------------------------------------------ Adam
def adam_constants(step, lr=5e-4, b1=0.9, b2=0.999, eps=1e-8, exact=False):
    """exact=False: what the launcher hands adam_kernel -- 1 - beta in double, then rounded once; (float)beta2; step_size =
    (float)(lr / bias1); sqrt_bias2 = (float)sqrt(bias2); (float)eps.  exact=True: torch.optim.Adam's double constants."""
    bias1, bias2 = 1.0 - b1 ** step, 1.0 - b2 ** step
    r = (lambda x: x) if exact else f32r
    return dict(omb1=r(1.0 - b1), b2=r(b2), omb2=r(1.0 - b2), step_size=r(lr / bias1), sqrt_bias2=r(np.sqrt(bias2)), eps=r(eps))


def adam_constant_distance(step, **kw):
    """largest relative distance of a launcher constant from its double value"""
    a, b = adam_constants(step, exact=False, **kw), adam_constants(step, exact=True, **kw)
    return max(abs(a[k] - b[k]) / abs(b[k]) for k in a)


def adam64(p, g, m, v, step, lr=5e-4, b1=0.9, b2=0.999, eps=1e-8, exact=False):
    """torch.optim.Adam's single-tensor update in float64 on the float32 state: exp_avg.lerp_(grad, 1 - beta1),
    exp_avg_sq.mul_(beta2).addcmul_(grad, grad, value=1 - beta2), denom = sqrt(exp_avg_sq) / sqrt(bias2) + eps,
    param -= step_size exp_avg / denom.  Returns (p, m, v)."""
    c = adam_constants(step, lr, b1, b2, eps, exact)
    p, g, m, v = f64(p), f64(g), f64(m), f64(v)
    mi = m + (g - m) * c['omb1']
    vi = v * c['b2'] + c['omb2'] * g * g
    return p - c['step_size'] * (mi / (np.sqrt(vi) / c['sqrt_bias2'] + c['eps'])), mi, vi


def adam_first_step_m(g, b1=0.9):
    """exp_avg after a step from m == 0, exactly: 0 + (g - 0) omb1 is one product of two float32 numbers -- exact in double -- rounded
    once, so a float32 implementation has these bits wherever the result is in the normal range (second return value).  This pins
    omb1 = (float)(1 - beta1): 1.f - (float)beta1 is 2.2e-7 larger and changes the bits of nearly every element."""
    exact = (f64(g) * adam_constants(1, b1=b1)['omb1']).astype(np.float32)
    return exact, np.abs(exact) >= FLUSH


def ulp32(a):
    """spacing of float32 at |a| (2^-149 below the normal range)"""
    a = np.abs(a)
    _, e = np.frexp(a)
    return np.where(a < FLUSH, DENORM, np.ldexp(1.0, e - 24))


def adam_bounds(p, g, m, v, step, lr=5e-4, b1=0.9, b2=0.999, eps=1e-8):
    """How far a float32 adam_kernel may be from adam64.  Per element:
      m' = m + (g - m) omb1: the difference, the product, the sum -- each at most U of A_m = |m| + omb1 (|g| + |m|), the sum of the
        magnitudes (m and omb1 (g - m) cancel when g and m have opposite signs):                     d_m <= gamma(3) A_m + FLUSH
      v' = v b2 + (omb2 g) g: same-signed terms, at most 3 roundings in a row and the sum:            d_v <= gamma(4) v' + FLUSH
      s = sqrt(v') / sqrt_bias2: half of v's relative error, the root, the division;  den = s + eps: 1 more
      u = step_size (m' / den): m's and den's errors to first order with the remainder 1 / (1 - d_den / den), 2 roundings
      p - u: half a spacing at the result.
    Returns dict(p, m, v), each times its constant."""
    c = adam_constants(step, lr, b1, b2, eps)
    p64, mi, vi = adam64(p, g, m, v, step, lr, b1, b2, eps)
    g, m = f64(g), f64(m)
    A_m = np.abs(m) + c['omb1'] * (np.abs(g) + np.abs(m))
    d_m = gamma(3) * A_m + FLUSH
    d_v = gamma(4) * vi + FLUSH
    s = np.sqrt(vi) / c['sqrt_bias2']
    d_s = s * (gamma(4) / 2 + gamma(2)) + np.sqrt(FLUSH) / c['sqrt_bias2']
    den = s + c['eps']
    d_den = d_s + U * den
    u = c['step_size'] * mi / den
    d_u = (c['step_size'] * d_m / den + np.abs(u) * d_den / den) / (1 - d_den / den) + gamma(2) * np.abs(u) + FLUSH
    d_p = d_u + 0.5 * ulp32(np.abs(p64) + d_u)
    return dict(p=C['adam_p'] * d_p, m=C['adam_m'] * d_m, v=C['adam_v'] * d_v)


# ------------------------------------------------------------------------------------------------------------ sphere intersection
def sphere_far64(ray_o, ray_d):
    """intersect_sphere (ddp_train_nerf.py:51-66) in float64 on the float32 inputs.  Returns (far, pn): pn = |closest point|^2."""
    o, d = f64(ray_o), f64(ray_d)
    dd = (d * d).sum(-1)
    d1 = -(d * o).sum(-1) / dd
    p = o + d1[:, None] * d
    pn = (p * p).sum(-1)
    with np.errstate(invalid='ignore'):
        return d1 + np.sqrt(1.0 - pn) / np.sqrt(dd), pn


def sphere_far_bound(ray_o, ray_d):
    """d . o: gamma(3) of sum |d_k o_k| (it cancels); d1 = -(d . o) / dd: that over dd, and gamma(4) of itself (dd's 3, the division);
    p_k = o_k + d1 d_k: d1's error times |d_k|, 2 roundings on |o_k| + |d1 d_k|; pn = sum p_k^2: 2 |p_k| d_p_k + d_p_k^2 and gamma(3) pn;
    y = 1 - pn cancels next to the sphere: d_pn + U y; sqrt(y) moves by at most sqrt(y) - sqrt(y - d_y) (all of sqrt(y + d_y) when
    y < d_y), 1 rounding; 1 / sqrt(dd): gamma(4); the product and the last sum, 1 each.  Only for rays inside the sphere (pn < 1)."""
    o, d = f64(ray_o), f64(ray_d)
    dd = (d * d).sum(-1)
    do = (d * o).sum(-1)
    d1 = -do / dd
    d_d1 = gamma(3) * np.abs(d * o).sum(-1) / dd * (1 + gamma(4)) + gamma(4) * np.abs(d1) + FLUSH
    p = o + d1[:, None] * d
    d_p = d_d1[:, None] * np.abs(d) + gamma(2) * (np.abs(o) + np.abs(d1[:, None] * d)) + FLUSH
    pn = (p * p).sum(-1)
    d_pn = (2 * np.abs(p) * d_p + d_p * d_p).sum(-1) + gamma(3) * (pn + (2 * np.abs(p) * d_p + d_p * d_p).sum(-1))
    y = 1.0 - pn
    d_y = d_pn + U * np.abs(y)
    root = np.sqrt(np.maximum(y, 0))
    d_root = np.where(y > d_y, root - np.sqrt(np.maximum(y - d_y, 0)), np.sqrt(np.maximum(y, 0) + d_y)) + U * (root + np.sqrt(d_y))
    inv = 1 / np.sqrt(dd)
    d2 = root * inv
    d_d2 = prod_bound(root, d_root, inv, gamma(4) * inv) + FLUSH
    return C['sphere_far'] * (d_d1 + d_d2 + U * (np.abs(d1) + d_d1 + np.abs(d2) + d_d2))


# ------------------------------------------------------------------------------------------------------------ input families
COMPOSITE_S = (2, 3, 63, 64, 65, 128, 129, 192, 193, 255, 256)
COMPOSITE_N = (1, 3, 4, 5, 9)
COMPOSITE_FAMILIES = ('general', 'zero', 'saturating', 'zero_width', 'colour_ends', 'ray_scale', 'bg_tail')
SATURATING_X = (80.0, 87.5, 95.0, 104.0, 1e4)
SATURATING_COUNTS = (1, 8, 0)                     # samples per ray at that exponent; 0 = all
RAY_SCALES = (1e-3, 1.0, 1e3)
UPSTREAM = ('random', 'zero', 'depth_only', 'no_weights')
LOSS_N = (1, 2, 255, 256, 257, 1023, 1024, 1025, 2500)
LOSS_S = (2, 64, 65, 256)
LOSS_LAMBDAS = (0.0, 0.3, 1.0)
LOSS_MASKS = ('all', 'none', 'mixed')
KL_SIGMAS = (1e-4, 1e-2, 1.0)
FUSED_N = (1, 5, 257, 1025)
ADAM_N = (1, 255, 256, 257, 70001)
ADAM_STEPS = (1, 2, 10, 1000, 100000, 500000)
ADAM_GRADS = tuple(10.0 ** k for k in range(-20, 19)) + (3e-7,)
SPHERE_PN = (0.0, 0.5, 1 - 2.0 ** -10, 1 - 2.0 ** -20, 1 - 2.0 ** -23)
BAD_N = (1, 255, 256, 257, 1000)
COARSE_S = (2, 64, 256)

f32 = np.float32


def _seed(*parts):
    return zlib.crc32(repr(parts).encode())


def composite_case(family, S, n):
    """The float32 inputs of one compositing call as a dict (keys _IN_KEYS).
    general: sigma of both signs, colours in (0, 1), ascending fg_z with fg_far >= fg_z[-1], ascending bg_z in (0, 1);
    zero: sigma_raw exactly +0 or -0 on every other ray and on a third of the other samples;
    saturating: |sigma| dist in SATURATING_X on 1, 8 or all samples of a ray (the combination walks with the ray and with S);
    zero_width: tied fg_z, fg_far == fg_z[-1], tied bg_z;   colour_ends: half of the colours exactly 0 or 1;
    ray_scale: |ray_d| in RAY_SCALES;   bg_tail: the last background interval (1e10 wide) with sigma 0, 1e-12 and 1."""
    rs = np.random.RandomState(_seed(family, S, n))
    ray_d = rs.randn(n, 3)
    ray_d /= np.sqrt((ray_d ** 2).sum(-1, keepdims=True))
    ray_d *= np.asarray(RAY_SCALES)[np.arange(n) % 3][:, None] if family == 'ray_scale' else rs.uniform(0.5, 2.0, (n, 1))
    fg_z = np.sort(rs.uniform(0.01, 2.0, (n, S)), -1).astype(f32)
    bg_z = np.sort(rs.uniform(0.001, 0.999, (n, S)), -1).astype(f32)
    if family == 'zero_width':
        for k in range(0, S - 1, 3):
            fg_z[:, k + 1] = fg_z[:, k]
            bg_z[:, k + 1] = bg_z[:, k]
        fg_z[:, -1] = fg_z[:, -2] if n % 2 else fg_z[:, -1]
        fg_far = fg_z[:, -1].copy()
    else:
        fg_far = (fg_z[:, -1] + rs.uniform(0, 0.1, n).astype(f32)).astype(f32)
    scale = np.sqrt(S) * 10.0 ** rs.uniform(-1.5, 0.5, (2, n, 1))
    sigma = (rs.randn(2, n, S) * scale).astype(f32)
    colour = np.clip(rs.uniform(0, 1, (2, n, S, 3)), 1e-3, 1 - 1e-3).astype(f32)
    depth_real = (1.0 / (bg_z.astype(np.float64) + 1e-2) * rs.uniform(0.9, 1.1, (n, S))).astype(f32)
    ray_d = ray_d.astype(f32)
    if family == 'zero':
        sigma[:, ::2] = 0
        scattered = rs.rand(2, n, S) < 1.0 / 3
        sigma[scattered] = 0
        sigma[(rs.rand(2, n, S) < 0.5) & (sigma == 0)] = -0.0
    if family == 'colour_ends':
        ends = rs.rand(2, n, S, 3)
        colour[ends < 0.25] = 0
        colour[ends > 0.75] = 1
    if family == 'bg_tail':
        sigma[1, :, 0] = np.asarray([0.0, 1e-12, 1.0], f32)[np.arange(n) % 3]
    if family == 'saturating':
        dnorm = np.sqrt((ray_d.astype(np.float64) ** 2).sum(-1))[:, None]
        fg_dist = dnorm * np.concatenate([np.diff(fg_z.astype(np.float64), axis=-1), (fg_far.astype(np.float64) - fg_z[:, -1])[:, None]], -1)
        bg_dist = np.concatenate([np.full((n, 1), HUGE), np.diff(bg_z.astype(np.float64), axis=-1)], -1)     # natural order: sample 0 is the tail
        for r in range(n):
            combo = (r + S + n) % (len(SATURATING_X) * len(SATURATING_COUNTS))
            x, count = SATURATING_X[combo % len(SATURATING_X)], SATURATING_COUNTS[combo // len(SATURATING_X)]
            count = S if count == 0 else min(count, S)
            for vol, dist in ((0, fg_dist), (1, bg_dist)):
                idx = rs.choice(S, count, replace=False)
                sign = np.where(rs.rand(count) < 0.5, -1.0, 1.0)
                sigma[vol, r, idx] = (sign * x / np.maximum(dist[r, idx], 1e-30)).astype(f32)
    raw = np.concatenate([colour, sigma[..., None]], -1).astype(f32)
    return dict(raw_fg=raw[0].reshape(n * S, 4), raw_bg=raw[1].reshape(n * S, 4), depth_real_bg=depth_real.reshape(n * S),
                ray_d=ray_d, fg_far=fg_far, fg_z=fg_z, bg_z=bg_z)


def composite_cases(S):
    """every (family, n) pairing run at this S: the general family at every n, the others at two n each (walking with S, so that
    every family meets every n over COMPOSITE_S)"""
    k = COMPOSITE_S.index(S)
    out = [('general', n) for n in COMPOSITE_N]
    for j, fam in enumerate(COMPOSITE_FAMILIES[1:]):
        out += [(fam, COMPOSITE_N[(k + j) % 5]), (fam, COMPOSITE_N[(k + j + 2) % 5])]
    return out


def mirrored(case):
    """the same rays with -sigma_raw in both volumes"""
    out = dict(case)
    for k in ('raw_fg', 'raw_bg'):
        r = case[k].copy()
        r[:, 3] = -r[:, 3]
        out[k] = r
    return out


def upstream(kind, S, n):
    """(g_rgb [n,3], g_depth [n], g_fg_weights [n,S] or None) float32"""
    rs = np.random.RandomState(_seed('up', kind, S, n))
    g_rgb, g_depth, g_w = rs.randn(n, 3).astype(f32), (0.1 * rs.randn(n)).astype(f32), (0.01 * rs.randn(n, S)).astype(f32)
    if kind == 'zero':
        return 0 * g_rgb, 0 * g_depth, 0 * g_w
    if kind == 'depth_only':
        return 0 * g_rgb, g_depth, None
    if kind == 'no_weights':
        return g_rgb, g_depth, None
    return g_rgb, g_depth, g_w


def depth_sup_for(mask, fg_far, rs):
    """priors [n] float32 for fg_far.  'all': every ray has 0 < gt < fg_far; 'none': gt <= 0 (-0.0, +0.0 and negatives in turn);
    'mixed', by ray index modulo 9: 0-2 valid, 3 gt == fg_far, 4 gt == nextafter(fg_far, 0), 5 -0.0, 6 negative, 7 +0.0, 8 gt = 1.5 fg_far
    (beyond fg_far: valid for mse / l1, outside the KL mask)"""
    n = fg_far.shape[0]
    gt = rs.uniform(0.02, 1.0, n).astype(f32) * fg_far
    gt = np.minimum(gt, np.nextafter(fg_far, f32(0))).astype(f32)
    r = np.arange(n)
    if mask == 'none':
        gt = np.where(r % 3 == 0, f32(-0.0), np.where(r % 3 == 1, f32(0.0), -gt))
    elif mask == 'mixed':
        kind = r % 9
        gt = np.where(kind == 3, fg_far, gt)
        gt = np.where(kind == 4, np.nextafter(fg_far, f32(0)), gt)
        gt = np.where(kind == 5, f32(-0.0), gt)
        gt = np.where(kind == 6, -gt, gt)
        gt = np.where(kind == 7, f32(0.0), gt)
        gt = np.where(kind == 8, fg_far * f32(1.5), gt)
    return gt.astype(f32)


def loss_case(n, S, mask, edges=True):
    """ret-like float32 inputs of the loss head: rgb, rgb_gt [n,3], depth, depth_sup, fg_far [n], fg_weights, fg_z, fg_dists [n,S];
    mask as in depth_sup_for.  edges: every 5th ray has an rgb residual of exactly 0, every 7th (with a prior) depth == gt, every 4th
    ray w == 0 on half its samples, every 6th dists == 0 on half.  (kl_far_case: priors so far away that the exponential underflows.)"""
    rs = np.random.RandomState(_seed('loss', n, S, mask))
    rgb, rgb_gt = rs.rand(n, 3).astype(f32), rs.rand(n, 3).astype(f32)
    fg_z = np.sort(rs.uniform(0.01, 2.0, (n, S)), -1).astype(f32)
    fg_far = (fg_z[:, -1] + f32(0.05)).astype(f32)
    w = rs.rand(n, S) ** 4
    w = (w / w.sum(-1, keepdims=True) * rs.rand(n, 1)).astype(f32)
    dists = np.concatenate([np.diff(fg_z, axis=-1), (fg_far - fg_z[:, -1])[:, None]], -1).astype(f32)
    depth = (w * fg_z).sum(-1).astype(f32)
    gt = depth_sup_for(mask, fg_far, rs)
    r = np.arange(n)
    if edges:
        rgb[::5] = rgb_gt[::5]
        valid = gt > 0
        depth = np.where((r % 7 == 0) & valid, gt, depth).astype(f32)
        w[::4, ::2] = 0
        dists[::6, 1::2] = 0
    return dict(rgb=rgb, rgb_gt=rgb_gt, depth=depth, depth_sup=gt.astype(f32), fg_far=fg_far, fg_weights=w, fg_z=fg_z, fg_dists=dists)


def loss_cases():
    """[(n, S, mask, loss_type, lambda_depth, kl_sigma)]: every n x S x mask x type; lambda_depth and kl_sigma walk through their
    lists so that every type meets every value of both"""
    out, i = [], 0
    for n in LOSS_N:
        for S in LOSS_S:
            for mask in LOSS_MASKS:
                for t in range(4):
                    out.append((n, S, mask, t, LOSS_LAMBDAS[i % 3], KL_SIGMAS[(i // 3 + i // 12) % 3]))
                    i += 1
    return out


def kl_far_case(n, S, kl_sigma):
    """a KL batch whose priors sit so far from every sample that expf(-(z - gt)^2 / (2 sigma)) is exactly 0 in any float32
    evaluation ((z - gt)^2 / (2 sigma) >= 200 > 104): every term and every gradient is exactly 0, n_valid = n"""
    c = loss_case(n, S, 'all', edges=False)
    gap = np.sqrt(400.0 * kl_sigma)
    c['fg_z'] = (c['fg_z'] * f32(0.01)).astype(f32)                        # samples in (0, 0.02]
    c['depth_sup'] = np.full(n, 0.03 + gap, f32)
    c['fg_far'] = (c['depth_sup'] + f32(1.0)).astype(f32)
    return c


def adam_case(n, step, seed=0):
    """p, g, m, v (float32).  Element i has a gradient of magnitude ADAM_GRADS[(i + step + seed) % 40] |N(0, 1)| -- every decade from
    1e-20 to 1e18 and 3e-7, where sqrt(v_hat) is about eps -- and every 7th gradient is exactly 0.  Above step 1 the moments are those
    of a history whose gradients had the magnitude of g and, on every other element, the opposite sign; a tenth of the elements sit
    within 1e-3 of the complete cancellation m + (g - m) omb1 = 0, that is g = -9 m."""
    rs = np.random.RandomState(_seed('adam', n, step, seed))
    scale = np.asarray(ADAM_GRADS)[(np.arange(n) + step + seed) % len(ADAM_GRADS)]
    with np.errstate(over='ignore', under='ignore'):
        g = (rs.randn(n) * scale).astype(f32)
        g[::7] = 0
        p = (rs.randn(n) * 0.1).astype(f32)
        if step == 1:
            return p, g, np.zeros(n, f32), np.zeros(n, f32)
        sign = np.where(np.arange(n) % 2 == 0, -1.0, 1.0)
        m = sign * np.abs(rs.randn(n) * scale) * (1 - 0.9 ** (step - 1))
        near = rs.rand(n) < 0.1
        m = np.where(near, -f64(g) / 9 * (1 + 1e-3 * rs.randn(n)), m)
        v = np.minimum((rs.randn(n) * scale) ** 2 * (1 - 0.999 ** (step - 1)), 1e37)
        return p, g, m.astype(f32), v.astype(f32)


def adam_dyadic_case(n):
    """A step in which every operation is exact in float32: beta1 = 0.5, beta2 = 0.75, step 1 (bias1 = 0.5, sqrt(bias2) = 0.5),
    lr = 2^-10, g = +-2^-3 or 0, m = v = 0, eps = 2^-3: m' = g / 2, v' = g^2 / 4, denom = |g| + eps = 2^-2 (2^-3 where g = 0), update
    2^-9 m' / denom = +-2^-11; p a multiple of 2^-12 in [-1, 1].  Returns (p, g, m, v, kwargs)."""
    rs = np.random.RandomState(n)
    p = (rs.randint(-4096, 4097, n) / 4096.0).astype(f32)
    g = (rs.randint(-1, 2, n) * 0.125).astype(f32)
    return p, g, np.zeros(n, f32), np.zeros(n, f32), dict(step=1, lr=2.0 ** -10, beta1=0.5, beta2=0.75, eps=0.125)


def sphere_case(scale):
    """ray_o, ray_d [15, 3] float32 for |ray_d| = scale: per target pn of SPHERE_PN an axis-aligned ray whose float32 pn is exact
    (origin (a, 0, 0), direction (0, scale, 0): d . o = 0 and pn = fl(a a); a = 1 - 2^-21 and 1 - 2^-24 give 1 - 2^-20 and 1 - 2^-23), for
    pn <= 1 - 2^-10 also a ray in general position through a closest point of that norm, a camera at the origin, and four random rays."""
    rs = np.random.RandomState(_seed('sphere', scale))
    a_of = {0.0: 0.0, 0.5: np.sqrt(0.5), 1 - 2.0 ** -10: np.sqrt(1 - 2.0 ** -10), 1 - 2.0 ** -20: 1 - 2.0 ** -21, 1 - 2.0 ** -23: 1 - 2.0 ** -24}
    o, d = [], []
    for pn in SPHERE_PN:
        o.append([a_of[pn], 0, 0])
        d.append([0, scale, 0])
        if pn <= 1 - 2.0 ** -10:
            q, _ = np.linalg.qr(rs.randn(3, 3))
            t = rs.uniform(-0.5, 0.5)
            o.append(np.sqrt(pn) * q[0] + t * q[1])
            d.append(scale * q[1])
    o.append([0, 0, 0])
    d.append(scale * np.array([0.6, 0, 0.8]))
    for _ in range(4):
        o.append(rs.uniform(-0.5, 0.5, 3))
        v = rs.randn(3)
        d.append(scale * v / np.linalg.norm(v))
    return np.asarray(o, np.float64).astype(f32), np.asarray(d, np.float64).astype(f32)


def bad_case(n, k):
    """n rays, k of them with pn >= 1 (spread evenly; the first of them has pn == 1 exactly: origin (1, 0, 0), direction (0, 1, 0)).
    Returns (ray_o, ray_d, min_depth, is_bad)."""
    rs = np.random.RandomState(_seed('bad', n, k))
    o = rs.uniform(-0.5, 0.5, (n, 3)).astype(f32)
    d = rs.randn(n, 3).astype(f32)
    bad = np.zeros(n, bool)
    if k:
        bad[np.unique(np.linspace(0, n - 1, k).astype(int))] = True
        assert bad.sum() == k
        idx = np.nonzero(bad)[0]
        o[idx] = [1.5, 0, 0]
        d[idx] = [0, 1, 0.25]
        o[idx[0]] = [1, 0, 0]
        d[idx[0]] = [0, 1, 0]
    return o, d, np.full(n, 1e-4, f32), bad

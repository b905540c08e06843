"""The Gaussian negative-log-likelihood depth loss (include/depthgnll_hip.h) in float64 numpy: value, both gradients,
stats and the per-ray classes, plus the generator of the test cases.  Not a test module; tests/test_depth_gnll.py,
tests/test_gpu_depth_gnll.py and tests/golden/make_golden_depth_gnll.py import it.

    per ray r:  samples x_s, weights w_s (s < S), the rendered depth D, the prior p, its standard deviation sigma, the bound lim
    m    = p > 0 and sigma > 0 and (lim is None or p < lim)               supervised
    M0   = sum w_s,  M1 = sum w_s x_s
    V    = sum w_s (x_s - D)^2 + 1e-5                                     rendered variance
    gate = m and (|D - p| - sigma > 0 or sigma^2 < V)                     outside the expected distribution
    Vc   = max(V, 1e-3)
    l    = 0.5 (log Vc + (D - p)^2 / Vc)
    value = (1 / n) sum_{gate} l_r                                        (n = all rays)
    gV   = 0.5 (1 / Vc - (D - p)^2 / Vc^2)                                (the clamp changes the value only)
    d value / d D   = gate [ (D - p) / Vc - 2 gV (M1 - D M0) ] / n
    d value / d w_s = gate gV (x_s - D)^2 / n
The gate is a constant for the gradient; positions receive none; D is an input, not recomputed as M1.
"""
import numpy as np

VAR_EPS, VAR_MIN = 1e-5, 1e-3
MARGIN = 1e-4                      # how far, relatively, the generator keeps every ray from the gate and from the clamp


def positions(x, edges=False):
    """float64 sample positions [n, S] of x: positions [n, S] as they are, or interval edges [n, S + 1], whose midpoint
    0.5f * (t[s] + t[s + 1]) is formed in float32 as written"""
    x = np.asarray(x)
    if edges:
        t = x.astype(np.float32)
        x = np.float32(0.5) * (t[:, :-1] + t[:, 1:])
    return x.astype(np.float64)


def gnll(w, x, d, p, sigma, limit=None, edges=False):
    """w [n, S], x [n, S] (or [n, S + 1] edges), d, p, sigma, limit [n] (any float dtype, taken to float64 value by value) ->
    dict(value, loss [n] (l_r, 0 when not gated), abs_sum = (1 / n) sum |l_r|, g_d [n], g_w [n, S] float64, sup / gated / clamped [n]
    bool, stats [3] = (supervised, gated, gated with V < 1e-3), V, M0, M1 [n], mean_test [n] bool = |D - p| - sigma > 0)"""
    w, xs = np.asarray(w).astype(np.float64), positions(x, edges)
    d, p, sigma = (np.asarray(a).astype(np.float64) for a in (d, p, sigma))
    n = w.shape[0]
    sup = (p > 0) & (sigma > 0)
    if limit is not None:
        sup &= p < np.asarray(limit).astype(np.float64)
    dx = xs - d[:, None]
    M0, M1 = w.sum(1), (w * xs).sum(1)
    V = (w * dx * dx).sum(1) + VAR_EPS
    diff = d - p
    gated = sup & ((np.abs(diff) - sigma > 0) | (sigma * sigma < V))
    clamped = gated & (V < VAR_MIN)
    Vc = np.maximum(V, VAR_MIN)
    loss = np.where(gated, 0.5 * (np.log(Vc) + diff * diff / Vc), 0.0)
    gV = 0.5 * (1.0 / Vc - diff * diff / (Vc * Vc))
    g_d = np.where(gated, (diff / Vc - 2.0 * gV * (M1 - d * M0)) / n, 0.0)
    g_w = np.where(gated[:, None], gV[:, None] * dx * dx / n, 0.0)
    return dict(value=loss.sum() / n, loss=loss, abs_sum=np.abs(loss).sum() / n, g_d=g_d, g_w=g_w, sup=sup, gated=gated, clamped=clamped,
                stats=np.array([sup.sum(), gated.sum(), clamped.sum()], np.float64), V=V, M0=M0, M1=M1,
                mean_test=np.abs(diff) - sigma > 0)


# ------------------------------------------------------------------------------------------------------------ test cases
CLASSES = ('p0', 'sigma0', 'limit', 'ungated', 'mean_only', 'var_only', 'clamped')


def classes(ref, p, sigma, limit=None):
    """{class name: rays [n] bool} of one level's reference result"""
    p, sigma = np.asarray(p, np.float64), np.asarray(sigma, np.float64)
    out = {'p0': p <= 0, 'sigma0': (p > 0) & (sigma <= 0), 'ungated': ref['sup'] & ~ref['gated'], 'clamped': ref['clamped']}
    out['limit'] = (p > 0) & (sigma > 0) & ~ref['sup'] if limit is not None else np.zeros(len(p), bool)
    var_test = sigma * sigma < ref['V']
    out['mean_only'] = ref['gated'] & ~var_test
    out['var_only'] = ref['gated'] & var_test & ~ref['mean_test']
    return out


def _margins(ref, d, p, sigma):
    """per ray: is it at least MARGIN (relative) off the two gate tests; off the clamp"""
    gap = np.abs(np.abs(d - p) - sigma)
    off_gate = (gap >= MARGIN * sigma) & (np.abs(sigma * sigma - ref['V']) >= MARGIN * ref['V'])
    off_clamp = np.abs(ref['V'] - VAR_MIN) >= MARGIN * VAR_MIN
    return off_gate, off_clamp


def draw(seed, n, samples, edges=False, with_limit=False, far=6.0, offset=0.3):
    """A case: float32 w[l] [n, S_l], x[l] [n, S_l] or [n, S_l + 1], d[l] [n] per level, p, sigma, limit (or None) [n].  A ray's
    weights are a bump of random width about a random depth (from one sample wide, so that V falls under the clamp, to a spread of
    0.5) between 0.5 and `far`, D is the bump's mean plus a little, the prior lies a random way off (normal, std `offset`) with a
    random standard deviation (offset / 30 .. 2 offset).  With n >= 64 the
    first rays are planted, one per class of CLASSES (on level 0's rendering).  Every ray is kept off the discontinuities in
    float64: a ray within MARGIN (relative) of either gate test on any level has its sigma multiplied by 1.01 until clear; no ray is
    left out.  (The clamp does not depend on sigma: a ray within MARGIN of it on a level has that level's weights multiplied by 1.01.)"""
    rs = np.random.RandomState(seed)
    f32 = np.float32
    W, X, D = [], [], []
    centre = rs.uniform(0.5 + 0.1 * (far - 0.5), far - 0.1 * (far - 0.5), n)
    width = np.exp(rs.uniform(np.log(0.004), np.log(0.5), n))
    for l, S in enumerate(samples):
        t = np.sort(rs.uniform(0.5, far, (n, S + 1)), axis=1).astype(f32)
        x = t if edges else (0.5 * (t[:, :-1] + t[:, 1:])).astype(f32)
        xs = positions(x, edges)
        if n >= 64 and l == 0:                              # the planted clamped ray: its bump sits on a sample and is one wide
            centre[6], width[6] = xs[6, S // 2], 0.004
        e = -0.5 * ((xs - centre[:, None]) / width[:, None]) ** 2
        w = np.exp(e - e.max(1, keepdims=True))
        w = (w / w.sum(1, keepdims=True) * rs.uniform(0.6, 1.0, (n, 1))).astype(f32)
        m1 = (w.astype(np.float64) * xs).sum(1) / w.astype(np.float64).sum(1)
        d = (m1 + rs.uniform(-0.02, 0.02, n)).astype(f32)
        W.append(w), X.append(x), D.append(d)
    d0 = D[0].astype(np.float64)
    sigma = np.exp(rs.uniform(np.log(offset / 30.0), np.log(2.0 * offset), n))
    p = d0 + rs.randn(n) * offset
    p = np.where(p > 0.05, p, 0.05)
    kill = rs.rand(n)
    p[kill < 0.1] = 0.0
    sigma[(kill >= 0.1) & (kill < 0.2)] = 0.0
    limit = None
    if with_limit:
        limit = np.where(rs.rand(n) < 0.15, p * 0.9, p + rs.uniform(0.1, 2.0, n)).astype(f32)
    if n >= 64:
        V0 = gnll(W[0], X[0], D[0], np.ones(n), np.ones(n), None, edges)['V']
        sd = np.sqrt(V0)
        p[0], sigma[0] = 0.0, 0.1                                              # unsupervised by p = 0
        p[1], sigma[1] = d0[1] + offset, 0.0                                      # unsupervised by sigma = 0
        p[2], sigma[2] = d0[2] + offset, offset                                      # unsupervised by p >= limit (where there is one)
        sigma[3] = 2.0 * sd[3]; p[3] = d0[3] + 0.3 * sigma[3]                  # supervised, not gated
        sigma[4] = 2.0 * sd[4]; p[4] = d0[4] + 3.0 * sigma[4]                  # gated by the mean test only
        sigma[5] = 0.5 * sd[5]; p[5] = d0[5] + 0.3 * sigma[5]                  # gated by the variance test only
        p[6], sigma[6] = d0[6] + 1.5 * offset, offset / 3.0                                      # gated (mean test) and clamped
        assert V0[6] < VAR_MIN
        if limit is not None:
            limit[2] = f32(p[2] * 0.5)
            for r in (3, 4, 5, 6):
                limit[r] = f32(p[r] + 1.0)
    p, sigma = p.astype(f32), sigma.astype(f32)
    nudged = 0
    for _ in range(200):
        close, clear = np.zeros(n, bool), True
        for l in range(len(samples)):
            ref = gnll(W[l], X[l], D[l], p, sigma, limit, edges)
            off_gate, off_clamp = _margins(ref, D[l].astype(np.float64), p.astype(np.float64), sigma.astype(np.float64))
            if not off_clamp.all():                          # V does not depend on sigma: the level's weights of that ray grow
                W[l][~off_clamp] *= f32(1.01)
                nudged += int((~off_clamp).sum())
                clear = False
            close |= ~off_gate & (sigma > 0)
        if clear and not close.any():
            break
        sigma = np.where(close, sigma * f32(1.01), sigma).astype(f32)
        nudged += int(close.sum())
    else:
        raise AssertionError('the generator could not clear the gate')
    return dict(w=W, x=X, d=D, p=p, sigma=sigma, limit=limit, edges=edges, samples=list(samples), n=n, nudged=nudged)


def census(case):
    """{class name: count over every (ray, level) of the case}"""
    out = dict.fromkeys(CLASSES, 0)
    for l in range(len(case['samples'])):
        ref = gnll(case['w'][l], case['x'][l], case['d'][l], case['p'], case['sigma'], case['limit'], case['edges'])
        for k, v in classes(ref, case['p'], case['sigma'], case['limit']).items():
            out[k] += int(v.sum())
    return out

"""numpy float64 restatement of the line-of-sight term on the weights along a ray (include/raylos_hip.h), and the
generator of the test cases.  Not a test module.

    per ray r with S samples: ascending positions z_s, weights w_s, far bound hi_r, prior p_r (0 = none), half-width sigma_r; float32
    e_s = z_s  s < S,  e_S = hi_r                                   a weight is the mass of the interval [e_s, e_{s+1}]
    m_r      = p_r > 0  and  p_r < hi_r  and  sigma_r > 0           supervised
    lo_b     = float32(p_r - sigma_r),  hi_b = float32(p_r + sigma_r)
    empty_s  = e_{s+1} <= lo_b                                      the whole interval lies in front of the band
    near_s   = not empty_s  and  e_s < hi_b                         the interval touches the band (otherwise behind it: no term)
    k_s      = Phi((e_{s+1} - p_r) / (sigma_r / 3)) - Phi((e_s - p_r) / (sigma_r / 3)),  Phi(x) = 0.5 (1 + erf(x / sqrt 2)), float64
    L_r      = sum_s near_s (w_s - k_s)^2 + sum_s empty_s w_s^2
    value    = (1/n) sum_r m_r L_r
    d value / d w_s = m_r (near_s 2 (w_s - k_s) + empty_s 2 w_s) / n
    front_r  = sum_s empty_s w_s
    stats    = [ number of supervised rays,  sum_r m_r front_r ]
The comparisons are float32, on the float32 inputs.
"""
import math

import numpy as np

_erf = np.vectorize(math.erf, otypes=[np.float64])


def Phi(x):
    return 0.5 * (1.0 + _erf(np.asarray(x, np.float64) / np.sqrt(2.0)))


def classes(z, hi, p, sigma):
    """From the float32 inputs, in float32: e [n, S + 1] the interval edges, m [n], empty [n, S], near [n, S] (the last two masked
    by m)"""
    z, hi, p, sigma = (np.asarray(a, np.float32) for a in (z, hi, p, sigma))
    e = np.concatenate([z, hi[:, None]], -1)
    with np.errstate(invalid='ignore'):
        m = (p > 0) & (p < hi) & (sigma > 0)
        lo_b, hi_b = (p - sigma).astype(np.float32), (p + sigma).astype(np.float32)
        empty = e[:, 1:] <= lo_b[:, None]
        near = ~empty & (e[:, :-1] < hi_b[:, None])
    return e, m, empty & m[:, None], near & m[:, None]


def target(e, p, sigma, near):
    """k [n, S] in float64: the mass of N(p, (sigma / 3)^2) in [e_s, e_{s+1}], evaluated where `near` (0 elsewhere)"""
    e, p, sigma = np.asarray(e, np.float64), np.asarray(p, np.float64), np.asarray(sigma, np.float64)
    sd = np.where(sigma > 0, sigma, 1.0) / 3.0
    a = (e[:, :-1] - p[:, None]) / sd[:, None]
    b = (e[:, 1:] - p[:, None]) / sd[:, None]
    k = np.zeros(near.shape)
    k[near] = Phi(b[near]) - Phi(a[near])
    return k


def ray_los(w, z, hi, p, sigma, lam=1.0):
    """The definition above on float32 inputs (w may be float64, for finite differences), everything past the comparisons in
    float64.  Returns a dict: values [1]; value = lam * values[0]; los, front [n] the per-ray terms (0 where unsupervised); grad
    [n, S] the gradient of `value` (lam included); k [n, S]; m [n]; empty, near [n, S]; stats [2]; abs_sum: the sum of the absolute
    values of the terms of values[0] (they are squares: the value itself); front_abs: the same for stats[1]; touched [n, S]: the
    entries of a gradient buffer that receive a term."""
    w = np.asarray(w, np.float64)
    n, S = w.shape
    e, m, empty, near = classes(z, hi, p, sigma)
    k = target(e, p, sigma, near)
    d = w - k
    los = np.sum(np.where(near, d * d, 0.0), -1) + np.sum(np.where(empty, w * w, 0.0), -1)
    front = np.sum(np.where(empty, w, 0.0), -1)
    grad = lam * (np.where(near, 2 * d, 0.0) + np.where(empty, 2 * w, 0.0)) / n
    values = np.array([los.sum() / n])
    return dict(values=values, value=lam * values[0], los=los, front=front, grad=grad, k=k, m=m, empty=empty, near=near,
                stats=np.array([m.sum(), front.sum()], np.float64), abs_sum=np.abs(los).sum() / n,
                front_abs=np.sum(np.where(empty, np.abs(w), 0.0)), touched=empty | near)


# the planted rays of draw(), by row (a case with n >= 3 holds all of them, cycling through the kinds that fit; n < 3 is generic)
KINDS = ('no_prior', 'prior_past_far', 'no_sigma', 'band_in_front_of_z0', 'edge_on_lo_b', 'edge_on_hi_b', 'narrow_band',
         'band_past_far', 'zero_weights')


def _plant(c, r, kind, rs):
    """Make row r of the case the planted ray `kind`, and assert that it is"""
    z, hi, p, sg, w = c['z'], c['hi'], c['p'], c['sigma'], c['w']
    S = z.shape[1]
    f32 = np.float32
    if kind == 'no_prior':
        p[r] = 0.0
    elif kind == 'prior_past_far':
        p[r] = hi[r] if rs.rand() < 0.5 else f32(hi[r] * 1.25)
    elif kind == 'no_sigma':
        sg[r] = 0.0
    elif kind == 'band_in_front_of_z0':            # supervised, yet every interval lies behind the band: no term at all
        p[r], sg[r] = f32(z[r, 0] * 0.5), f32(z[r, 0] * 0.25)
        assert f32(p[r] + sg[r]) <= z[r, 0] and p[r] > 0
    elif kind in ('edge_on_lo_b', 'edge_on_hi_b'):
        # The edge z_j is MOVED (by an ulp or so) onto the bound that float32(p -+ sigma) gives, so the equality is exact.  sigma is a
        # power of two below every z.  An interval can only END on an interior edge with index >= 1, so for S = 1 (whose one interval
        # ends at hi, and p > hi is no supervised ray) edge_on_lo_b lands on z_0 and pins nothing; edge_on_hi_b pins `<` at z_0.
        j = S // 2
        sg[r] = f32(2.0 ** -8)
        if kind == 'edge_on_lo_b':
            p[r] = f32(z[r, j] + sg[r])
            z[r, j] = f32(p[r] - sg[r])
        else:
            p[r] = f32(z[r, j] - sg[r])
            z[r, j] = f32(p[r] + sg[r])
        z[r] = np.sort(z[r])
        assert 0 < p[r] < hi[r] and z[r, -1] < hi[r], (kind, S)
    elif kind == 'narrow_band':                    # the band lies strictly inside the interval that holds p
        j = S // 2
        a, b = float(z[r, j]), float(z[r, j + 1] if j + 1 < S else hi[r])
        if not b > a:                               # a tie: widen to the far bound
            b = float(hi[r])
        p[r], sg[r] = f32(0.5 * (a + b)), f32(0.125 * (b - a))
        assert a < f32(p[r] - sg[r]) and f32(p[r] + sg[r]) < b and sg[r] > 0
    elif kind == 'band_past_far':
        sg[r] = f32(0.25 * hi[r])
        p[r] = f32(hi[r] * 0.875)
        assert f32(p[r] + sg[r]) > hi[r] and p[r] < hi[r]
    elif kind == 'zero_weights':
        w[r] = 0.0


def draw(seed, n, S):
    """A case of n rays with S samples, float32: w [n, S] weights of a rendering (alpha compositing of random densities: not
    negative, summing to at most 1), z [n, S] ascending positions below hi [n], p [n] priors (about a fifth of the generic rays
    without one), sigma [n] half-widths from a fraction of an interval to several.  With n >= 3 the rays of KINDS are planted, row
    r holding KINDS[(r + seed) % 9] for the first min(n, 9) rows and every kind for n >= 9; `planted` maps a kind to its rows.
    The prefill of a gradient buffer is `g0` [n, S]: magnitudes in [0.25, 1), both signs, no zero."""
    rs = np.random.RandomState(seed)
    lo = rs.uniform(0.01, 0.3, n).astype(np.float32)
    hi = (lo + rs.uniform(0.5, 2.0, n)).astype(np.float32)
    t = np.sort(rs.uniform(0.0, 1.0, (n, S)), -1)
    z = (lo[:, None] + t * (hi - lo)[:, None] * 0.98).astype(np.float32)
    z = np.sort(np.clip(z, lo[:, None], (hi * np.float32(0.99))[:, None]), -1)
    alpha = 1.0 - np.exp(-rs.gamma(0.3, 1.0, (n, S)) * 3.0 / max(1, S) ** 0.5)
    T = np.cumprod(np.concatenate([np.ones((n, 1)), 1.0 - alpha[:, :-1]], -1), -1)
    w = (alpha * T).astype(np.float32)
    p = (lo + rs.uniform(0.05, 0.95, n) * (hi - lo)).astype(np.float32)
    p[rs.rand(n) < 0.2] = 0.0
    sigma = ((hi - lo) * rs.uniform(0.2, 4.0, n) / max(S, 2)).astype(np.float32)
    sign = np.where(rs.rand(n, S) < 0.5, -1.0, 1.0)
    g0 = (sign * rs.uniform(0.25, 1.0, (n, S))).astype(np.float32)
    c = dict(w=w, z=z, hi=hi, p=p, sigma=sigma, g0=g0, planted={})
    if n >= 3:
        for r in range(min(n, len(KINDS))):
            kind = KINDS[(r + seed) % len(KINDS)]
            _plant(c, r, kind, rs)
            c['planted'].setdefault(kind, []).append(r)
    assert (np.abs(g0) >= 0.25).all()
    return c


def check_planted(c, ref):
    """Assert every planted ray of the case against its reference: the classes are what the kind says"""
    S = c['z'].shape[1]
    for kind, rows in c['planted'].items():
        for r in rows:
            m, empty, near = ref['m'][r], ref['empty'][r], ref['near'][r]
            if kind in ('no_prior', 'prior_past_far', 'no_sigma'):
                assert not m and not empty.any() and not near.any() and not ref['grad'][r].any() and ref['los'][r] == 0, kind
            elif kind == 'band_in_front_of_z0':
                assert m and not empty.any() and not near.any() and ref['los'][r] == 0, kind
            elif kind == 'edge_on_lo_b':           # e_{s+1} == lo_b: `<=` makes the interval that ends there empty, `<` would not
                lo_b = np.float32(c['p'][r] - c['sigma'][r])
                e = np.concatenate([c['z'][r], c['hi'][r:r + 1]])
                hit = np.nonzero(e[1:] == lo_b)[0]
                assert m and len(hit) >= (S >= 2) and empty[hit].all() and not near[hit].any(), kind
            elif kind == 'edge_on_hi_b':           # e_s == hi_b: `<` leaves the interval that starts there behind the band
                hi_b = np.float32(c['p'][r] + c['sigma'][r])
                e = np.concatenate([c['z'][r], c['hi'][r:r + 1]])
                hit = np.nonzero(e[:-1] == hi_b)[0]
                assert m and len(hit) >= 1 and not near[hit].any() and not empty[hit].any(), kind
            elif kind == 'narrow_band':
                assert m and near.sum() == 1 and ref['k'][r][near][0] > 0.997, (kind, ref['k'][r][near])
            elif kind == 'band_past_far':
                assert m and near[S - 1] and ref['k'][r].sum() < 0.999, kind
            elif kind == 'zero_weights':
                assert not c['w'][r].any() and ref['front'][r] == 0, kind

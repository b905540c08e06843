"""numpy float64 restatement of the two regularisers on the weights along a ray (include/rayreg_hip.h), in prefix form,
and the generator of the test cases.  Not a test module.

    per ray r with S samples: ascending positions z_s, weights w_s, bounds lo_r, hi_r
    valid_r = hi_r > lo_r
    e_s = (z_s - lo_r) / (hi_r - lo_r)  s < S,  e_S = (hi_r - lo_r) / (hi_r - lo_r);  u_s = (e_s + e_{s+1}) / 2,  d_s = e_{s+1} - e_s
    A_s = sum_{j<s} w_j,  B_s = sum_{j<s} w_j u_j,  A'_s, B'_s: the same over j > s
    dist_r = 2 sum_s w_s (u_s A_s - B_s) + (1/3) sum_s w_s^2 d_s
    d dist_r / d w_s = 2 [u_s (A_s - A'_s) - (B_s - B'_s)] + (2/3) w_s d_s
    o_r = sum_s w_s + 1e-10,  opac_r = -o_r log o_r,  d opac_r / d w_s = -(log o_r + 1)
    values = [(1/n) sum_{valid r} dist_r, (1/n) sum_r opac_r]
    gradient[r, s] = (lambda_dist * valid_r * d dist_r / d w_s + lambda_opac * d opac_r / d w_s) / n
"""
import numpy as np

OPAC_EPS = 1e-10


def edges(z, lo, hi):
    """The normalised interval edges [n, S + 1] of the valid rays (rows of invalid rays are 0) and valid [n]"""
    z, lo, hi = np.asarray(z, np.float64), np.asarray(lo, np.float64), np.asarray(hi, np.float64)
    valid = np.asarray(hi) > np.asarray(lo)
    span = np.where(valid, hi - lo, 1.0)[:, None]
    e = np.concatenate([(z - lo[:, None]) / span, (hi - lo)[:, None] / span], -1)
    return np.where(valid[:, None], e, 0.0), valid


def _excl(v):
    """exclusive prefix sums along the last axis"""
    return np.cumsum(v, -1) - v


def ray_reg(w, z, lo, hi, lambda_dist, lambda_opac):
    """The definition above on float32 (or float64) inputs, everything in float64.  Returns a dict:
    values [2]; value = lambda_dist * values[0] + lambda_opac * values[1]; dist, opac [n] the per-ray terms (0 where a term is off
    or the ray invalid); grad [n, S] the gradient of `value`; grad_abs [n, S] the sum of the absolute values of the terms that make
    up each gradient entry; abs_sum [2] the sums of the absolute values of the terms of values; valid [n]; stats [1]; touched [n]:
    the rows of a gradient buffer that receive a term."""
    w = np.asarray(w, np.float64)
    n, S = w.shape
    e, valid = edges(z, lo, hi)
    u, d = (e[:, :-1] + e[:, 1:]) / 2, e[:, 1:] - e[:, :-1]
    dist, opac = np.zeros(n), np.zeros(n)
    grad, grad_abs = np.zeros((n, S)), np.zeros((n, S))
    abs_sum = np.zeros(2)
    if lambda_dist > 0:
        wu = w * u
        A, B = _excl(w), _excl(wu)
        Ap, Bp = _excl(w[:, ::-1])[:, ::-1], _excl(wu[:, ::-1])[:, ::-1]
        per = 2 * np.sum(w * (u * A - B), -1) + np.sum(w * w * d, -1) / 3
        dist = np.where(valid, per, 0.0)
        g = 2 * (u * (A - Ap) - (B - Bp)) + 2 * w * d / 3
        grad += lambda_dist * valid[:, None] * g / n
        aw, au, awu = np.abs(w), np.abs(u), np.abs(wu)
        term_abs = 2 * (au * (_excl(aw) + _excl(aw[:, ::-1])[:, ::-1]) + _excl(awu) + _excl(awu[:, ::-1])[:, ::-1]) + 2 * aw * np.abs(d) / 3
        grad_abs += lambda_dist * valid[:, None] * term_abs / n
        per_abs = 2 * np.sum(aw * (au * _excl(aw) + _excl(awu)), -1) + np.sum(w * w * np.abs(d), -1) / 3
        abs_sum[0] = np.sum(np.where(valid, per_abs, 0.0)) / n
    if lambda_opac > 0:
        o = w.sum(-1) + OPAC_EPS
        opac = -o * np.log(o)
        grad += (lambda_opac * -(np.log(o) + 1) / n)[:, None]
        grad_abs += (lambda_opac * (np.abs(np.log(o)) + 1) / n)[:, None]
        abs_sum[1] = np.sum(np.abs(opac)) / n
    values = np.array([dist.sum() / n, opac.sum() / n])
    touched = (valid & (lambda_dist > 0)) | (lambda_opac > 0)
    return dict(values=values, value=lambda_dist * values[0] + lambda_opac * values[1], dist=dist, opac=opac, grad=grad,
                grad_abs=grad_abs, abs_sum=abs_sum, valid=valid, stats=np.array([valid.sum()], np.float64), touched=touched)


def pairwise(e, w):
    """sum_ij w_i w_j |u_i - u_j| + (1/3) sum w^2 d on edges e [n, S + 1]: the definition the prefix form restates"""
    e, w = np.asarray(e, np.float64), np.asarray(w, np.float64)
    u, d = (e[:, :-1] + e[:, 1:]) / 2, e[:, 1:] - e[:, :-1]
    return np.sum(w[:, :, None] * w[:, None, :] * np.abs(u[:, :, None] - u[:, None, :]), (1, 2)) + np.sum(w * w * d, -1) / 3


# the planted rays of draw(), by row (a case with n >= 3 holds all of them; n = 1 is one generic ray)
TIED, ZERO, INVALID, UNIT = 0, 1, 2, 0


def draw(seed, n, S):
    """A case of n rays with S samples, float32: w [n, S] weights of a rendering (alpha compositing of random densities, so they
    are not negative and sum to at most 1), z [n, S] ascending positions in [lo, hi], lo, hi [n].  With n >= 3: row 0 has tied
    positions (S >= 2: a run of equal z) and weights that sum to 1 (in float64, after the float32 rounding, to 1e-6); row 1 has
    all-zero weights; row 2 has hi <= lo.  The prefill of a gradient buffer is `g0` [n, S]."""
    rs = np.random.RandomState(seed)
    lo = rs.uniform(0.01, 0.3, n).astype(np.float32)
    hi = (lo + rs.uniform(0.5, 2.0, n)).astype(np.float32)
    t = np.sort(rs.uniform(0.0, 1.0, (n, S)), -1)
    z = (lo[:, None] + t * (hi - lo)[:, None] * 0.98).astype(np.float32)
    z = np.sort(np.clip(z, lo[:, None], hi[:, None]), -1)
    alpha = 1.0 - np.exp(-rs.gamma(0.3, 1.0, (n, S)) * 3.0 / max(1, S) ** 0.5)
    T = np.cumprod(np.concatenate([np.ones((n, 1)), 1.0 - alpha[:, :-1]], -1), -1)
    w = (alpha * T).astype(np.float32)
    if n >= 3:
        if S >= 2:
            k = S // 2
            z[TIED, k - 1:min(S, k + 2)] = z[TIED, k - 1]                # two or three equal positions
        w[UNIT] = (w[UNIT].astype(np.float64) / max(w[UNIT].astype(np.float64).sum(), 1e-30)).astype(np.float32)
        if not w[UNIT].any():
            w[UNIT, 0] = 1.0
        w[ZERO] = 0.0
        hi[INVALID] = lo[INVALID] if seed % 2 else np.float32(lo[INVALID] * 0.5)
    g0 = rs.standard_normal((n, S)).astype(np.float32) * np.float32(1e-3)
    return dict(w=w, z=z, lo=lo, hi=hi, g0=g0)

"""The depth-guided fine sampling of the NeRF++ path (include/depthguide_hip.h) in float64 numpy, and the case
generator the CPU and GPU tests share.

`depth_guide` is the per-ray rule as written, with the sums over the previous level's samples in the kernel's order (lane l adds
samples l, l + 64, ... ascending, the 64 lanes by the xor butterfly), so that everything but a last bit of the float64 square root
can be compared bit for bit.  max(a, b) is  a < b ? b : a  (a NaN a stays a NaN, and a NaN guides no ray).
"""
import numpy as np

K = 1024
TRUNCATE = 3.0
W_MIN = 1e-10


def table(K=K, truncate=TRUNCATE):
    """T[i] = Phi^-1(Phi(-t) + (Phi(t) - Phi(-t)) i / K) by the standard library, ends exact: written here a second time, on purpose"""
    from statistics import NormalDist
    nd = NormalDist()
    a, b = nd.cdf(-truncate), nd.cdf(truncate)
    T = np.array([nd.inv_cdf(a + (b - a) * i / K) for i in range(K + 1)], np.float64)
    T[0], T[K] = -truncate, truncate
    return T


def exact_inverse(q, truncate=TRUNCATE):
    from statistics import NormalDist
    nd = NormalDist()
    a, b = nd.cdf(-truncate), nd.cdf(truncate)
    return np.array([-truncate if x <= 0 else truncate if x >= 1 else nd.inv_cdf(a + (b - a) * x) for x in np.asarray(q, np.float64).ravel()])


def interpolate(T, q):
    """the kernel's read of the table at quantiles q in [0, 1)"""
    Kt = len(T) - 1
    t = q * Kt
    i = np.minimum(t.astype(np.int64), Kt - 1)
    f = t - i
    return T[i] + f * (T[i + 1] - T[i])


def lane_tree_sum(x):
    """rows of x [n, S] summed as the kernel does: 64 per-lane running sums over l, l + 64, ..., then the xor butterfly"""
    n, S = x.shape
    lanes = np.zeros((n, 64))
    for i in range(0, S, 64):
        c = x[:, i:i + 64]
        lanes[:, :c.shape[1]] = lanes[:, :c.shape[1]] + c
    idx = np.arange(64)
    for d in (32, 16, 8, 4, 2, 1):
        lanes = lanes + lanes[:, idx ^ d]
    return lanes[:, 0]


def _max(a, b):
    return np.where(a < b, b, a)


def depth_guide(zp, wp, zin, lo, hi, G, prior=None, prior_std=None, std_const=0.0, min_std=0.0, v=None, T=None):
    """-> dict(z_merged [n, S_in + G] float32, mode [n] int32, guide [n, G] float32, g [n, G] float64 before the rounding, mu, sd [n])"""
    T = table() if T is None else T
    zp, wp, lo, hi = (np.asarray(a, np.float32).astype(np.float64) for a in (zp, wp, lo, hi))
    zin = np.asarray(zin, np.float32)
    n = zp.shape[0]
    p = np.zeros(n) if prior is None else np.asarray(prior, np.float32).astype(np.float64)
    s = np.full(n, float(std_const)) if prior_std is None else np.asarray(prior_std, np.float32).astype(np.float64)
    v = np.full((n, G), 0.5, np.float32) if v is None else np.asarray(v, np.float32)
    with np.errstate(invalid='ignore', divide='ignore', over='ignore'):
        s_eff = _max(s, float(min_std))
        guided = (p > 0) & (p < hi) & (s_eff > 0) & (s_eff < np.inf)
        W = lane_tree_sum(wp)
        B = lane_tree_sum(wp * zp)
        mode = np.where(guided, 0, np.where(W > W_MIN, 1, 2)).astype(np.int32)
        mu1 = B / W
        d = zp - mu1[:, None]
        sd1 = _max(np.sqrt(lane_tree_sum(wp * (d * d)) / W), float(min_std))
        mu, sd = np.where(guided, p, mu1), np.where(guided, s_eff, sd1)
        q = (np.arange(G, dtype=np.float64)[None] + v.astype(np.float64)) / float(G)
        x = interpolate(T, q)
        g = mu[:, None] + sd[:, None] * x
        g = np.where(g < lo[:, None], lo[:, None], g)
        g = np.where(g > hi[:, None], hi[:, None], g)
        g2 = lo[:, None] + (hi - lo)[:, None] * q
        g = np.where((mode == 2)[:, None], g2, g)
        guide = g.astype(np.float32)
    z = np.sort(np.concatenate([zin, guide], axis=-1), axis=-1, kind='stable')
    return dict(z_merged=z, mode=mode, guide=guide, g=g, mu=mu, sd=sd)


# ------------------------------------------------------------------------------------------------ cases
# the planted rays of a case, in this order (a case of fewer rays per call than kinds spreads them over several calls)
KINDS = ('prior_zero', 'prior_far', 'std_nan', 'std_zero', 'std_tiny', 'std_huge', 'prior_on_sample', 'zero_weights', 'one_weight',
         'inverted', 'unsorted_in', 'nan_in')
EXPECTED_MODE = dict(prior_zero=1, prior_far=1, std_nan=1, std_zero=1, std_tiny=0, std_huge=0, prior_on_sample=0, zero_weights=2,
                     one_weight=1, inverted=0, unsorted_in=0, nan_in=0)


def _ray(rs, S_prev, S_in, G, kind=None):
    """one ray: (zp, wp, zin, lo, hi, p, s, v); a plain one has a prior with probability 2/3"""
    lo = np.float32(rs.uniform(0.01, 0.1))
    hi = np.float32(lo + rs.uniform(0.5, 2.0))
    u = lambda m: np.sort((lo + (hi - lo) * rs.uniform(0.0, 0.98, m)).astype(np.float32))
    zp, zin = u(S_prev), u(S_in)
    wp = rs.uniform(0.0, 1.0, S_prev) ** 3
    wp = (wp * rs.uniform(0.2, 1.0) / wp.sum()).astype(np.float32)           # W >= 0.2: far from the 1e-10 decision
    p = np.float32(lo + (hi - lo) * rs.uniform(0.1, 0.9))
    s = np.float32(p * np.exp(rs.uniform(np.log(0.005), np.log(0.2))))
    if kind is None and rs.rand() < 1.0 / 3.0:
        p = np.float32(0)
    v = (rs.randint(0, 1 << 24, G) / float(1 << 24)).astype(np.float32)
    if kind == 'prior_zero':
        p = np.float32(0)
    elif kind == 'prior_far':
        p = hi
    elif kind == 'std_nan':
        s = np.float32(np.nan)
    elif kind == 'std_zero':
        s = np.float32(0)
    elif kind == 'std_tiny':
        s = np.float32(1e-30)
    elif kind == 'std_huge':
        s = np.float32(1e30)
        v = np.maximum(v, np.float32(2.0 ** -24))                             # (no quantile of exactly 1/2, whose x is 0)
    elif kind == 'prior_on_sample':
        p, s = zin[S_in // 2], np.float32(1e-30)
    elif kind == 'zero_weights':
        wp, p = np.zeros(S_prev, np.float32), np.float32(0)
    elif kind == 'one_weight':
        wp, p = np.zeros(S_prev, np.float32), np.float32(0)
        wp[S_prev // 2] = np.float32(0.5)
    elif kind == 'inverted':
        lo, hi, p, s = np.float32(0.5), np.float32(0.25), np.float32(0.1), np.float32(0.05)
    elif kind == 'unsorted_in':
        zin = zin[::-1].copy()
    elif kind == 'nan_in':
        zin[0] = np.float32(np.nan)
    return zp, wp, zin, lo, hi, p, s, v


def draw(seed, n, S_prev, S_in, G):
    """The case of shape (n, S_prev, S_in, G): a list of calls, each a dict of arrays for n rays (zp, wp, zin, lo, hi, p, s, v) with
    `kinds` [n] (the planted kind's name or '').  n >= 3: the calls together hold one ray of every kind (one call where n >= the
    number of kinds); n < 3: one call of plain rays."""
    rs = np.random.RandomState(seed)
    kinds = list(KINDS) if n >= 3 else []
    calls = []
    while True:
        take, kinds = kinds[:n], kinds[n:]
        rays = [_ray(rs, S_prev, S_in, G, k) for k in take] + [_ray(rs, S_prev, S_in, G) for _ in range(n - len(take))]
        c = {name: np.stack([np.asarray(r[i]) for r in rays]) for i, name in enumerate(('zp', 'wp', 'zin', 'lo', 'hi', 'p', 's', 'v'))}
        c['kinds'] = np.array(take + [''] * (n - len(take)))
        calls.append(c)
        if not kinds:
            return calls

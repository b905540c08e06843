"""The scale-and-shift-invariant depth loss (include/depthssi_hip.h) in float64 numpy: value, gradient, fit and
stats.  Not a test module; tests/test_depth_ssi.py and tests/test_gpu_depth_ssi.py import it.

    m_i = p_i > 0 and 0 <= g_i < G
    per group k:  N = sum m, Sd = sum m d, Sdd = sum m d^2, Sp = sum m p, Sdp = sum m d p       (float64 sums of the float32 inputs)
    fitted  iff   N >= min_rays  and  N Sdd - Sd^2 > 1e-8 N Sdd
    w = (N Sdp - Sd Sp) / (N Sdd - Sd^2),  q = (Sp - w Sd) / N,  r_i = w d_i + q - p_i
    L = (1 / D) sum_{fitted k} sum_i m_i r_i^2,   dL/dd_i = 2 w r_i / D on the supervised rays of fitted groups, 0 elsewhere
    D = n ('all') or max(N_sup, 1) ('supervised'), N_sup = sum over all groups of m
"""
import numpy as np

FLAT = 1e-8
NORMS = ('all', 'supervised')


def ssi(d, p, g=None, n_groups=1, min_rays=8, norm='all'):
    """d, p [n] (any float dtype, taken to float64 value by value), g [n] integer ids or None (one group) ->
    dict(value, grad [n] float64, fit [G, 4] float64 = (w, q, N, fitted), stats [2] = (N_sup, supervised rays in fitted groups),
    touched [n] bool = the rays whose gradient entry the loss owns, D)"""
    assert norm in NORMS
    d, p = np.asarray(d).astype(np.float64), np.asarray(p).astype(np.float64)
    n = d.shape[0]
    g = np.zeros(n, np.int64) if g is None else np.asarray(g).astype(np.int64)
    sup = (p > 0) & (g >= 0) & (g < n_groups)
    n_sup = float(sup.sum())
    D = float(n) if norm == 'all' else max(n_sup, 1.0)
    grad, touched, fit = np.zeros(n), np.zeros(n, bool), np.zeros((n_groups, 4))
    total, n_fit = 0.0, 0.0
    for k in range(n_groups):
        m = sup & (g == k)
        N = float(m.sum())
        dk, pk = d[m], p[m]
        Sd, Sdd, Sp, Sdp = dk.sum(), (dk * dk).sum(), pk.sum(), (dk * pk).sum()
        var = N * Sdd - Sd * Sd
        fit[k, 2] = N
        if not (N >= min_rays and var > FLAT * N * Sdd):
            continue
        w = (N * Sdp - Sd * Sp) / var
        q = (Sp - w * Sd) / N
        r = w * dk + q - pk
        total += (r * r).sum()
        grad[m] = 2.0 * w * r / D
        touched[m] = True
        fit[k] = (w, q, N, 1.0)
        n_fit += N
    return dict(value=total / D, grad=grad, fit=fit, stats=np.array([n_sup, n_fit]), touched=touched, D=D)


def coefficient_of_variation(d, p, g=None, n_groups=1):
    """per group: std / |mean| of d over the group's supervised rays (NaN for a group without any)"""
    d, p = np.asarray(d).astype(np.float64), np.asarray(p)
    g = np.zeros(d.shape[0], np.int64) if g is None else np.asarray(g).astype(np.int64)
    out = np.full(n_groups, np.nan)
    for k in range(n_groups):
        m = (p > 0) & (g == k)
        if m.any():
            out[k] = d[m].std() / abs(d[m].mean())
    return out

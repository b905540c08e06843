"""numpy reference of the per-ray 'kl_ray' / 'urf_ray' depth losses of the MipNeRF-360 path (mip360_depth_loss_rays):
value and closed-form gradients of ONE level.

    steps = 0.5 (t[s] + t[s+1]),  len = (t[s+1] - t[s]) |dir|,  m_r = sup_r > 0,  gt = sup_r
    kl_ray  = (1/n) sum_r m_r sum_s -log(w + 1e-7) exp(-(steps - gt)^2 / (2 sigma)) len
    urf_ray = (1/n) sum_r m_r [ (gt - dm_r)^2 + sum_s near (w - pdf)^2 + sum_s empty w^2 ]
        pdf = exp(-(steps - gt)^2 / (2 (sigma/3)^2) - log(sigma/3) - log(sqrt(2 pi)))
        near = steps <= gt + sigma and steps >= gt - sigma,  empty = steps < gt - sigma

The inputs are float32 arrays.  `near` / `empty` are ALWAYS formed in float32 from them, as the definition says (0.5f * (t0 + t1),
gt + sigma and gt - sigma are one rounding each), so there is no band around the edges in which an implementation and this file
may disagree.  Everything else runs in `dtype`: float64 (the reference) or float32 (what float32 arithmetic costs on the same
inputs: the yardstick of the gradient gates).
"""
import numpy as np

KINDS = ('kl_ray', 'urf_ray')


def flags(tdist, depth_sup, sigma):
    """(near, empty) [n, S] booleans, in float32"""
    t = np.asarray(tdist, np.float32)
    gt = np.asarray(depth_sup, np.float32)[:, None]
    sg = np.float32(sigma)
    steps = np.float32(0.5) * (t[:, :-1] + t[:, 1:])
    hi, lo = gt + sg, gt - sg
    assert steps.dtype == hi.dtype == lo.dtype == np.float32
    return (steps <= hi) & (steps >= lo), steps < lo


def value_and_grads(kind, weights, tdist, depth_sup, distance_mean, directions, sigma, dtype=np.float64):
    """-> (value, g_weights [n, S], g_distance_mean [n]) of one level, all of `dtype`"""
    assert kind in KINDS, kind
    f = lambda a: np.asarray(np.asarray(a, np.float32), dtype)
    w, t, sup = f(weights), f(tdist), f(depth_sup)
    n = w.shape[0]
    sg = dtype(np.float32(sigma))
    m = (np.asarray(depth_sup, np.float32) > 0).astype(dtype)
    gt = sup[:, None]
    steps = dtype(0.5) * (t[:, :-1] + t[:, 1:])
    d = steps - gt
    g_dm = np.zeros(n, dtype)
    if kind == 'kl_ray':
        dirs = f(directions)
        length = (t[:, 1:] - t[:, :-1]) * np.sqrt((dirs * dirs).sum(-1))[:, None]
        e = np.exp(-(d * d) / (dtype(2) * sg)) * length
        per_ray = (-np.log(w + dtype(1e-7)) * e).sum(-1)
        g_w = -e / (w + dtype(1e-7))
    else:
        dm = f(distance_mean)
        near, empty = flags(tdist, depth_sup, sigma)
        us = sg / dtype(3)
        pdf = np.exp(-(d * d) / (dtype(2) * us * us) - np.log(us) - np.log(np.sqrt(dtype(2) * dtype(np.pi))))
        diff = sup - dm
        per_ray = diff * diff + (near * (w - pdf) ** 2).sum(-1) + (empty * w * w).sum(-1)
        g_w = near * (dtype(2) * (w - pdf)) + empty * (dtype(2) * w)
        g_dm = -dtype(2) * diff * m / dtype(n)
    value = (per_ray * m).sum() / dtype(n)
    g_w = g_w * m[:, None] / dtype(n)
    assert g_w.dtype == dtype and g_dm.dtype == dtype
    return value, g_w, g_dm


def accumulated(kind, weights, tdist, depth_sup, distance_mean, directions, sigma, scale=1.0, fill_w=0.0, fill_dm=0.0,
                dtype=np.float64):
    """What the entry point leaves in its gradient buffers: fill + scale * gradient -> (g_weights [n, S], g_distance_mean [n]);
    fill_w / fill_dm: what the buffers held before, a number or an array of the buffer's shape.
    In float32 the product and the sum are rounded like any float32 `buffer += scale * gradient`."""
    _, g_w, g_dm = value_and_grads(kind, weights, tdist, depth_sup, distance_mean, directions, sigma, dtype)
    c = lambda v: np.asarray(np.asarray(v, np.float32), dtype)
    return c(fill_w) + c(scale) * g_w, c(fill_dm) + c(scale) * g_dm


def grad_errors(got_w, got_dm, kind, weights, tdist, depth_sup, distance_mean, directions, sigma, scale=1.0, fill_w=0.0,
                fill_dm=0.0):
    """Errors of the buffers (got_w, got_dm) against the float64 `accumulated`, as a fraction of max |scale * gradient| of the
    level -> (e_weights, e_distance_mean); e_distance_mean is 0 for kl_ray (no gradient: compare the buffer exactly instead)."""
    args = (kind, weights, tdist, depth_sup, distance_mean, directions, sigma, scale, fill_w, fill_dm)
    want_w, want_dm = accumulated(*args)
    size_w = np.abs(want_w - np.asarray(fill_w, np.float32).astype(np.float64)).max()
    size_dm = np.abs(want_dm - np.asarray(fill_dm, np.float32).astype(np.float64)).max()
    e_w = np.abs(np.asarray(got_w, np.float64) - want_w).max() / max(size_w, 1e-300)
    e_dm = np.abs(np.asarray(got_dm, np.float64) - want_dm).max() / size_dm if size_dm > 0 else 0.0
    return float(e_w), float(e_dm)


def float32_errors(kind, weights, tdist, depth_sup, distance_mean, directions, sigma, scale=1.0, fill_w=0.0, fill_dm=0.0):
    """grad_errors of this file's own float32 evaluation: what float32 arithmetic costs on these inputs (the yardstick of the
    gradient gates; it never sees the code under test)."""
    args = (kind, weights, tdist, depth_sup, distance_mean, directions, sigma, scale, fill_w, fill_dm)
    return grad_errors(*accumulated(*args, dtype=np.float32), *args)

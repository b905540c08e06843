"""The definition of the per-frame robust scale-and-shift alignment of relative depth priors to sparse metric depth (DESIGN 8.9,
include/depthalign_hip.h) as executable float64 numpy, every product and sum written out.  csrc/depthalign_kernels.hip computes
the same expressions without contraction; only the order of its sums differs (a fixed tree where numpy adds pairwise).

A value is valid iff > 0 (0, negatives and NaN are not).  space 'depth': target t = a, model z = s p + b.  space 'disparity': the
prior is relative inverse depth, t = 1.0 / a in float64, model 1 / z = s p + b.  Per frame, over the pairs with p > 0 and a > 0, an
iteratively reweighted least-squares fit with Cauchy weights whose scale is the weighted mean absolute residual; then the fit is
applied to every pixel with p > 0.
"""
import numpy as np

DEFAULTS = dict(space='depth', iters=10, c=1.0, min_points=16, max_depth=float('inf'), keep_anchor=False, std_floor=0.0)
SPACES = ('depth', 'disparity')
ROW_NAMES = ('s', 'b', 'sigma', 'n_pairs', 'n_inliers', 'status', 'iterations', 'rms')
STATUS_FITTED, STATUS_FEW, STATUS_DEGENERATE, STATUS_INVERTED = 0, 1, 2, 3
GAUSS = 1.2533141373155001            # sqrt(pi / 2): the standard deviation of a Gaussian over its mean absolute deviation


def pairs(p, a, space):
    """(x, t) float64 of one frame, in pixel order: the exactly widened prior and the target of the pairs with p > 0 and a > 0"""
    p, a = np.asarray(p, np.float32).reshape(-1), np.asarray(a, np.float32).reshape(-1)
    with np.errstate(invalid='ignore'):
        m = (p > 0) & (a > 0)
    x, a64 = p[m].astype(np.float64), a[m].astype(np.float64)
    return x, (1.0 / a64 if space == 'disparity' else a64)


def fit(x, t, iters=10, c=1.0, min_points=16, dtype=np.float64):
    """The row of one frame from its pairs: (s, b, sigma, n_pairs, n_inliers, status, iterations run, rms) in `dtype`"""
    x, t = np.asarray(x, dtype), np.asarray(t, dtype)
    n = len(x)
    bad = lambda status, it: np.array([0, 0, 0, n, 0, status, it, 0], dtype)
    if n < min_points:
        return bad(STATUS_FEW, 0)
    one, c = dtype(1.0), dtype(c)
    w = np.full(n, one)
    done = 0
    with np.errstate(all='ignore'):
        for k in range(iters + 1):
            wx = w * x
            Sw, Sx, St, Sxx, Sxt = np.sum(w), np.sum(wx), np.sum(w * t), np.sum(wx * x), np.sum(wx * t)
            den = Sw * Sxx - Sx * Sx
            if not den > (dtype(1e-8) * Sw) * Sxx:
                return bad(STATUS_DEGENERATE, done)
            s = (Sw * Sxt - Sx * St) / den
            b = (St - s * Sx) / Sw
            done += 1
            r = (s * x + b) - t
            sigma = dtype(GAUSS) * (np.sum(w * np.abs(r)) / Sw)
            rss = np.sum(r * r)
            if not (k < iters and sigma > 0):
                break
            q = np.abs(r) / (c * sigma)
            w = one / (one + q * q)
        rms = np.sqrt(rss / dtype(n))
        if not (s > 0 and np.isfinite(s) and np.isfinite(b) and np.isfinite(sigma) and np.isfinite(rms)):
            return bad(STATUS_INVERTED, done)
        n_in = int(np.sum(np.abs(r) <= dtype(3.0) * sigma))
    return np.array([s, b, sigma, n, n_in, STATUS_FITTED, done, rms], dtype)


def apply(p, a, rows, space='depth', max_depth=float('inf'), keep_anchor=False, std_floor=0.0):
    """(depth_out, std_out) float32 [F, H, W] of step 6 and 7 with the rows given"""
    p, a = np.asarray(p, np.float32), np.asarray(a, np.float32)
    rows = np.asarray(rows, np.float64)
    depth_out, std_out = np.zeros(p.shape, np.float32), np.zeros(p.shape, np.float32)
    with np.errstate(all='ignore'):
        for f in range(p.shape[0]):
            s, b, sigma = rows[f, 0], rows[f, 1], rows[f, 2]
            if rows[f, 5] == STATUS_FITTED:
                x = p[f].astype(np.float64)
                v = s * x + b
                z = 1.0 / v if space == 'disparity' else v
                ok = (p[f] > 0) & (v > 0) & (z <= max_depth)
                std = (sigma * z) * z if space == 'disparity' else np.full(z.shape, sigma)
                depth_out[f] = np.where(ok, z.astype(np.float32), np.float32(0))
                std_out[f] = np.where(ok, np.where(std > std_floor, std, std_floor).astype(np.float32), np.float32(0))
            if keep_anchor:
                own = a[f] > 0
                depth_out[f].view(np.int32)[own] = a[f].view(np.int32)[own]
                std_out[f][own] = np.float32(std_floor)
    return depth_out, std_out


def align(prior, anchor, space='depth', iters=10, c=1.0, min_points=16, max_depth=float('inf'), keep_anchor=False, std_floor=0.0):
    """{'depth_out', 'std_out' float32 [F, H, W], 'rows' float64 [F, 8]}"""
    prior, anchor = np.asarray(prior, np.float32), np.asarray(anchor, np.float32)
    assert prior.shape == anchor.shape and prior.ndim == 3 and space in SPACES
    rows = np.stack([fit(*pairs(prior[f], anchor[f], space), iters=iters, c=c, min_points=min_points) for f in range(prior.shape[0])], 0)
    depth_out, std_out = apply(prior, anchor, rows, space, max_depth, keep_anchor, std_floor)
    return dict(depth_out=depth_out, std_out=std_out, rows=rows)

"""The plane sweep with semi-global smoothing as executable code: steps 4a and 4b, and steps 5 to 7 on S, on top
of tests/depth_mvs_reference.py, whose census, luma, cost_volume, aggregate and refine are imported, not copied.  numpy, integers for
everything new.  sweep() is the vectorised form (a whole row or column of a direction at a time), sweep_pixel() the scalar one, which
walks every path of one pixel naively from the frame's border, plane by plane.

    P1 = smooth_p1 * best_views * (2 a + 1)^2, P2 likewise: penalties per census bit in the units of C
    L_r(p, k) = C(p, k)                                                                          q = p - r outside the frame
    L_r(p, k) = C(p, k) + min(L_r(q, k), L_r(q, k - 1) + P1, L_r(q, k + 1) + P1, M + P2') - M    M = min_k L_r(q, k)
    P2' = P2 (smooth_edge 0) or max(P1, P2 // (1 + |Y(p) - Y(q)| // smooth_edge))
    S(p, k) = sum_r L_r(p, k)
"""
import numpy as np

from tests import depth_mvs_reference as R
from tests.depth_mvs_reference import ACCEPTED, END, AMBIGUOUS, UNSEEN      # noqa: F401

DIRS = ((1, 0), (-1, 0), (0, 1), (0, -1), (1, 1), (-1, -1), (1, -1), (-1, 1))          # (dx, dy), in the definition's order
MAX_P2 = 32767
DEFAULTS = dict(smooth_paths=8, smooth_p1=1, smooth_p2=8, smooth_edge=0)
_BIG = 1 << 40


def penalties(best_views, agg_radius, smooth_p1, smooth_p2):
    unit = int(best_views) * (2 * int(agg_radius) + 1) ** 2
    P1, P2 = int(smooth_p1) * unit, int(smooth_p2) * unit
    assert 1 <= P1 <= P2 <= MAX_P2
    return P1, P2


# ------------------------------------------------------------------------------------------------ step 4a, vectorised
def path(C, Y, dx, dy, P1, P2, edge):
    """L_r int64 [D, H, W] of direction r = (dx, dy) from C int64 [D, H, W] and the luma Y int64 [H, W]"""
    if dy == 0:                                               # along the rows: the same walk on the transposed frame
        return path(C.transpose(0, 2, 1), Y.T, 0, dx, P1, P2, edge).transpose(0, 2, 1)
    D, H, W = C.shape
    L = np.zeros((D, H, W), np.int64)
    xs = np.arange(W)
    qx = xs - dx
    inside = (qx >= 0) & (qx < W)
    qxc = np.clip(qx, 0, W - 1)
    for y in (range(H) if dy > 0 else range(H - 1, -1, -1)):
        qy = y - dy
        if not 0 <= qy < H:
            L[:, y] = C[:, y]
            continue
        Lq = L[:, qy][:, qxc]                                 # [D, W]: the predecessor's values (clipped ones are masked below)
        M = Lq.min(0)
        below = np.full((D, W), _BIG, np.int64)
        above = np.full((D, W), _BIG, np.int64)
        below[1:] = Lq[:-1] + P1
        above[:-1] = Lq[1:] + P1
        p2 = P2 if edge == 0 else np.maximum(P1, P2 // (1 + np.abs(Y[y] - Y[qy, qxc]) // edge))
        t = np.minimum(np.minimum(Lq, np.minimum(below, above)), M + p2)
        L[:, y] = np.where(inside, C[:, y] + t - M, C[:, y])
    return L


def paths(C, Y, n_paths, P1, P2, edge):
    """[L_r] of the first n_paths directions"""
    assert n_paths in (4, 8) and 0 <= int(edge) <= 255
    return [path(C, Y, dx, dy, P1, P2, int(edge)) for dx, dy in DIRS[:n_paths]]


# ------------------------------------------------------------------------------------------------ steps 5 to 7 on S
def select(S, n_in, inv_depth, best_views, uniqueness, std_planes):
    """{'depth', 'std', 'status', 'plane', 'cost', 'second', 'rows' (one frame's row)} of one frame from S and n_in int64 [D, H, W]"""
    D, H, W = S.shape
    ks = np.arange(D)[:, None, None]
    kb = np.argmin(S, axis=0)                                                        # the lowest k of minimal S
    Ss = np.take_along_axis(S, kb[None], 0)[0]
    second = np.where(np.abs(ks - kb[None]) > 1, S, np.iinfo(np.int64).max).min(0)
    nb = np.take_along_axis(n_in, kb[None], 0)[0]
    status = np.full((H, W), ACCEPTED, np.uint8)
    status[~(Ss.astype(np.float64) <= np.float64(uniqueness) * second.astype(np.float64))] = AMBIGUOUS
    status[(kb == 0) | (kb == D - 1)] = END
    status[nb < best_views] = UNSEEN
    depth, std = np.zeros((H, W), np.float32), np.zeros((H, W), np.float32)
    for y, x in zip(*np.nonzero(status == ACCEPTED)):
        k = int(kb[y, x])
        depth[y, x], std[y, x] = R.refine(k, Ss[y, x], S[k - 1, y, x], S[k + 1, y, x], inv_depth, np.float64(std_planes))
    return dict(depth=depth, std=std, status=status, plane=kb.astype(np.uint8), cost=Ss.astype(np.uint32), second=second.astype(np.uint32),
                rows=np.array([(status == v).sum() for v in (ACCEPTED, END, AMBIGUOUS, UNSEEN)], np.int64))


def volumes(rgb, cams, nbr, inv_depth, i, best_views, agg_radius, cen=None):
    """(C int64 [D, H, W], n_in int64 [D, H, W], Y int64 [H, W]) of frame i: steps 1 to 4 of the plain sweep"""
    rgb = np.asarray(rgb)
    cen = R.census(rgb) if cen is None else cen
    c, n_in = R.cost_volume(cen, np.asarray(cams, np.float64), nbr, np.asarray(inv_depth, np.float64), i, best_views)
    return R.aggregate(c, agg_radius), n_in, R.luma(rgb[i])


def sweep(rgb, cams, nbr, inv_depth, best_views=None, agg_radius=2, uniqueness=0.9, std_planes=0.5, smooth_paths=8, smooth_p1=1,
          smooth_p2=8, smooth_edge=0, keep=False):
    """The outputs of tests.depth_mvs_reference.sweep (without 'off'), taken on S; cost and second are uint32.  keep: also 'S'
    int64 [F, D, H, W] and 'L_max' (the largest value of any path)."""
    rgb = np.asarray(rgb)
    assert rgb.dtype == np.uint8 and rgb.ndim == 4 and rgb.shape[3] == 3
    cams = np.asarray(cams, np.float64)
    F, H, W = rgb.shape[:3]
    nbr = np.asarray(nbr, np.int64).reshape(F, -1)
    inv_depth = np.asarray(inv_depth, np.float64)
    m, a, uniq, std_planes = R._params(nbr.shape[1], best_views, agg_radius, uniqueness, std_planes)
    P1, P2 = penalties(m, a, smooth_p1, smooth_p2)
    cen = R.census(rgb)
    out = dict(depth=np.zeros((F, H, W), np.float32), std=np.zeros((F, H, W), np.float32), status=np.zeros((F, H, W), np.uint8),
               plane=np.zeros((F, H, W), np.uint8), cost=np.zeros((F, H, W), np.uint32), second=np.zeros((F, H, W), np.uint32),
               census=cen, rows=np.zeros((F, 4), np.int64))
    if keep:
        out['S'], out['L_max'] = np.zeros((F, len(inv_depth), H, W), np.int64), 0
    for i in range(F):
        C, n_in, Y = volumes(rgb, cams, nbr, inv_depth, i, m, a, cen)
        Ls = paths(C, Y, smooth_paths, P1, P2, smooth_edge)
        S = np.sum(Ls, axis=0)                                                      # step 4b
        one = select(S, n_in, inv_depth, m, uniq, std_planes)
        for name, v in one.items():
            out[name][i] = v
        if keep:
            out['S'][i], out['L_max'] = S, max(out['L_max'], max(int(L.max()) for L in Ls))
    return out


# ------------------------------------------------------------------------------------------------ the scalar form
def path_pixel(C, Y, y, x, dx, dy, P1, P2, edge):
    """[L_r(p, k) for k] of pixel p = (x, y): the path walked from the border, one pixel and one plane at a time"""
    D, H, W = C.shape
    sx, sy = x, y
    while 0 <= sx - dx < W and 0 <= sy - dy < H:              # back to the pixel whose predecessor is outside
        sx, sy = sx - dx, sy - dy
    L = [int(C[k, sy, sx]) for k in range(D)]
    while (sx, sy) != (x, y):
        qx, qy = sx, sy
        sx, sy = sx + dx, sy + dy
        M = min(L)
        p2 = P2
        if edge > 0:
            p2 = max(P1, P2 // (1 + abs(int(Y[sy, sx]) - int(Y[qy, qx])) // edge))
        new = []
        for k in range(D):
            t = min(L[k], M + p2)
            if k > 0:
                t = min(t, L[k - 1] + P1)
            if k < D - 1:
                t = min(t, L[k + 1] + P1)
            new.append(int(C[k, sy, sx]) + t - M)
        L = new
    return L


def sweep_pixel(rgb, cams, nbr, inv_depth, i, y, x, best_views=None, agg_radius=2, uniqueness=0.9, std_planes=0.5, smooth_paths=8,
                smooth_p1=1, smooth_p2=8, smooth_edge=0, vol=None):
    """One pixel: (depth float32, std float32, status, plane, cost, second).  vol: volumes() of frame i, to share between pixels."""
    f64 = np.float64
    F = np.asarray(rgb).shape[0]
    nbr = np.asarray(nbr, np.int64).reshape(F, -1)
    m, a, uniq, std_planes = R._params(nbr.shape[1], best_views, agg_radius, uniqueness, std_planes)
    P1, P2 = penalties(m, a, smooth_p1, smooth_p2)
    C, n_in, Y = volumes(rgb, cams, nbr, inv_depth, i, m, a) if vol is None else vol
    D = C.shape[0]
    S = [0] * D
    for dx, dy in DIRS[:smooth_paths]:
        L = path_pixel(C, Y, y, x, dx, dy, P1, P2, int(smooth_edge))
        S = [s + l for s, l in zip(S, L)]
    kb = min(range(D), key=lambda k: (S[k], k))
    second = min(S[k] for k in range(D) if abs(k - kb) > 1)
    if n_in[kb, y, x] < m:
        status = UNSEEN
    elif kb == 0 or kb == D - 1:
        status = END
    elif not f64(S[kb]) <= uniq * f64(second):
        status = AMBIGUOUS
    else:
        status = ACCEPTED
    z, s = np.float32(0), np.float32(0)
    if status == ACCEPTED:
        z, s = R.refine(kb, S[kb], S[kb - 1], S[kb + 1], np.asarray(inv_depth, np.float64), std_planes)
    return z, s, status, kb, S[kb], second

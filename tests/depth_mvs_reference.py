"""The plane-sweep multi-view stereo depth prior as executable code: numpy, integers for everything discrete and
float64 with every product and sum written out element by element in the order libdepthmvs_hip.so follows (no `@`, no dot: BLAS may
fuse or reorder).  sweep() is the vectorised form, sweep_pixel() the scalar one, step by step as DESIGN 8.11 numbers them.

Conventions: frame i has fx, fy, cx, cy and a camera-to-world [R_i | t_i] in the OpenCV convention (x right, y down, z forward);
pixel centres sit at +0.5; depth is z-depth in scene units.

    rgb        uint8 [F, H, W, 3]
    cams       float64 [F, 16]: fx fy cx cy, then the 12 values of the 3 x 4 camera-to-world, row-major
    nbr        int [F, V]: the frames a frame is matched against, in list order; j < 0 (and j >= F) is no neighbour
    inv_depth  float64 [D]: the planes as inverse depths, strictly increasing, >= 0
"""
import numpy as np

ACCEPTED, END, AMBIGUOUS, UNSEEN = 0, 1, 2, 3
OUT = 24                                                     # the cost of a view that is out of bounds: every census bit
DEFAULTS = dict(best_views=None, agg_radius=2, uniqueness=0.9, std_planes=0.5)
_POP8 = np.array([bin(v).count('1') for v in range(256)], np.int64)


def popcount24(x):
    x = np.asarray(x, np.int64)
    return _POP8[x & 255] + _POP8[(x >> 8) & 255] + _POP8[(x >> 16) & 255]


# ------------------------------------------------------------------------------------------------ step 1: luma and census
def luma(rgb):
    """int64 [..., H, W]: (77 R + 150 G + 29 B + 128) >> 8"""
    c = np.asarray(rgb).astype(np.int64)
    return (77 * c[..., 0] + 150 * c[..., 1] + 29 * c[..., 2] + 128) >> 8


def census(rgb):
    """uint32 [F, H, W]: bit t of the 24 is set when tap t of the 5 x 5 window, in row-major (dy, dx) order skipping the centre, is
    below the centre; taps outside the frame read the nearest pixel inside"""
    y = luma(rgb)
    F, H, W = y.shape
    pad = np.pad(y, ((0, 0), (2, 2), (2, 2)), mode='edge')
    out = np.zeros((F, H, W), np.int64)
    tap = 0
    for dy in range(-2, 3):
        for dx in range(-2, 3):
            if dy == 0 and dx == 0:
                continue
            out |= (pad[:, 2 + dy:2 + dy + H, 2 + dx:2 + dx + W] < y).astype(np.int64) << tap
            tap += 1
    return out.astype(np.uint32)


# ------------------------------------------------------------------------------------------------ step 2: geometry
def view_terms(ci, cj):
    """(A [3][3], b [3]) of reference camera ci and view camera cj [16]: A = Rj^T Ri, b = Rj^T (ti - tj).  The point of pixel
    (X, Y, 1) of ci at inverse depth w is, in cj's camera and up to the factor w, h = A (X, Y, 1) + w b."""
    d0, d1, d2 = ci[7] - cj[7], ci[11] - cj[11], ci[15] - cj[15]
    A = [[(cj[4 + c] * ci[4 + q] + cj[8 + c] * ci[8 + q]) + cj[12 + c] * ci[12 + q] for q in range(3)] for c in range(3)]
    b = [(cj[4 + c] * d0 + cj[8 + c] * d1) + cj[12 + c] * d2 for c in range(3)]
    return A, b


def project(A, b, cj, X, Y, w):
    """(in_bounds-before-the-frame test, floor(u), floor(v)) of pixel rays (X, Y, 1) on plane w in view cj:
    h_c = (A_c0 X + A_c1 Y) + (A_c2 + w b_c), u = fx (h_0 / h_2) + cx, v = fy (h_1 / h_2) + cy"""
    h = [(A[c][0] * X + A[c][1] * Y) + (A[c][2] + w * b[c]) for c in range(3)]
    fu = np.floor(cj[0] * (h[0] / h[2]) + cj[2])
    fv = np.floor(cj[1] * (h[1] / h[2]) + cj[3])
    return h[2] > 0, fu, fv


def best_default(n_views):
    return (int(n_views) + 1) // 2


def _params(n_views, best_views, agg_radius, uniqueness, std_planes):
    m = best_default(n_views) if best_views is None else int(best_views)
    assert 1 <= m <= n_views and 0 <= int(agg_radius) <= 4
    return m, int(agg_radius), np.float64(uniqueness), np.float64(std_planes)


def refine(k, Cs, cm, cp, inv_depth, std_planes):
    """step 7 of one accepted pixel: (z float32, std float32)"""
    den = int(cm) - 2 * int(Cs) + int(cp)
    off = np.float64(int(cm) - int(cp)) / np.float64(2 * den) if den > 0 else np.float64(0)
    wk = np.float64(inv_depth[k])
    step = wk - np.float64(inv_depth[k - 1]) if off < 0 else np.float64(inv_depth[k + 1]) - wk
    w = wk + off * step
    z = np.float64(1) / w
    return np.float32(z), np.float32(((std_planes * z) * z) * step)


# ------------------------------------------------------------------------------------------------ the vectorised form
def cost_volume(cen, cams, nbr, inv_depth, i, best_views):
    """(c int64 [D, H, W], n_in int64 [D, H, W]) of frame i: steps 2 and 3"""
    F, H, W = cen.shape
    D = len(inv_depth)
    ci = cams[i]
    ys, xs = np.meshgrid(np.arange(H), np.arange(W), indexing='ij')
    X = ((xs + 0.5) - ci[2]) / ci[0]
    Y = ((ys + 0.5) - ci[3]) / ci[1]
    mine = cen[i].astype(np.int64)
    views = [int(j) for j in nbr[i]]
    c = np.zeros((D, H, W), np.int64)
    n_in = np.zeros((D, H, W), np.int64)
    terms = {j: view_terms(ci, cams[j]) for j in views if 0 <= j < F}
    with np.errstate(all='ignore'):
        for k in range(D):
            costs = np.full((len(views), H, W), OUT, np.int64)
            for s, j in enumerate(views):
                if not 0 <= j < F:
                    continue
                A, b = terms[j]
                front, fu, fv = project(A, b, cams[j], X, Y, np.float64(inv_depth[k]))
                inb = front & (fu >= 0) & (fu < W) & (fv >= 0) & (fv < H)          # a NaN is outside
                xi, yi = np.where(inb, fu, 0).astype(np.int64), np.where(inb, fv, 0).astype(np.int64)
                costs[s] = np.where(inb, popcount24(mine ^ cen[j].astype(np.int64)[yi, xi]), OUT)
                n_in[k] += inb
            c[k] = np.sort(costs, axis=0)[:best_views].sum(0)
    return c, n_in


def aggregate(c, radius):
    """C [D, H, W]: the sum of c over the (2 a + 1)^2 window, taps outside the frame reading the nearest pixel inside"""
    D, H, W = c.shape
    pad = np.pad(c, ((0, 0), (radius, radius), (radius, radius)), mode='edge')
    C = np.zeros_like(c)
    for dy in range(2 * radius + 1):
        for dx in range(2 * radius + 1):
            C += pad[:, dy:dy + H, dx:dx + W]
    return C


def sweep(rgb, cams, nbr, inv_depth, best_views=None, agg_radius=2, uniqueness=0.9, std_planes=0.5):
    """{'depth', 'std': float32 [F, H, W], 'status', 'plane': uint8, 'cost', 'second': uint16, 'census': uint32 [F, H, W], 'rows':
    int64 [F, 4] (n_accepted, n_end, n_ambiguous, n_unseen), 'off': float64 [F, H, W] (the refinement's offset, 0 where not
    accepted)}"""
    rgb = np.asarray(rgb)
    assert rgb.dtype == np.uint8 and rgb.ndim == 4 and rgb.shape[3] == 3
    cams = np.asarray(cams, np.float64)
    F, H, W = rgb.shape[:3]
    nbr = np.asarray(nbr, np.int64).reshape(F, -1)
    inv_depth = np.asarray(inv_depth, np.float64)
    D = len(inv_depth)
    m, a, uniq, std_planes = _params(nbr.shape[1], best_views, agg_radius, uniqueness, std_planes)
    cen = census(rgb)
    out = dict(depth=np.zeros((F, H, W), np.float32), std=np.zeros((F, H, W), np.float32), status=np.zeros((F, H, W), np.uint8),
               plane=np.zeros((F, H, W), np.uint8), cost=np.zeros((F, H, W), np.uint16), second=np.zeros((F, H, W), np.uint16),
               census=cen, rows=np.zeros((F, 4), np.int64), off=np.zeros((F, H, W), np.float64))
    ks = np.arange(D)[:, None, None]
    for i in range(F):
        c, n_in = cost_volume(cen, cams, nbr, inv_depth, i, m)
        C = aggregate(c, a)                                                         # step 4
        kb = np.argmin(C, axis=0)                                                   # step 5: the lowest k of minimal C
        Cs = np.take_along_axis(C, kb[None], 0)[0]
        second = np.where(np.abs(ks - kb[None]) > 1, C, np.iinfo(np.int64).max).min(0)
        nb = np.take_along_axis(n_in, kb[None], 0)[0]
        status = np.full((H, W), ACCEPTED, np.uint8)                                # step 6, the last rule first
        status[~(Cs.astype(np.float64) <= uniq * second.astype(np.float64))] = AMBIGUOUS
        status[(kb == 0) | (kb == D - 1)] = END
        status[nb < m] = UNSEEN
        out['status'][i], out['plane'][i], out['cost'][i], out['second'][i] = status, kb, Cs, second
        for y, x in zip(*np.nonzero(status == ACCEPTED)):                           # step 7
            k = int(kb[y, x])
            cm, cp = C[k - 1, y, x], C[k + 1, y, x]
            out['depth'][i, y, x], out['std'][i, y, x] = refine(k, Cs[y, x], cm, cp, inv_depth, std_planes)
            den = int(cm) - 2 * int(Cs[y, x]) + int(cp)
            out['off'][i, y, x] = (int(cm) - int(cp)) / (2.0 * den) if den > 0 else 0.0
        out['rows'][i] = [(status == v).sum() for v in (ACCEPTED, END, AMBIGUOUS, UNSEEN)]
    return out


# ------------------------------------------------------------------------------------------------ the scalar form
def sweep_pixel(rgb, cams, nbr, inv_depth, i, y, x, best_views=None, agg_radius=2, uniqueness=0.9, std_planes=0.5, cen=None):
    """One pixel, step by step: (depth float32, std float32, status, plane, cost, second).  The scalar twin of sweep()."""
    f64 = np.float64
    cams = np.asarray(cams, np.float64)
    F, H, W = np.asarray(rgb).shape[:3]
    nbr = np.asarray(nbr, np.int64).reshape(F, -1)
    D = len(inv_depth)
    m, a, uniq, std_planes = _params(nbr.shape[1], best_views, agg_radius, uniqueness, std_planes)
    if cen is None:
        cen = census(rgb)                                                           # step 1
    ci = cams[i]
    C, n_centre = [], []
    with np.errstate(all='ignore'):
        for k in range(D):
            total = 0
            for dy in range(-a, a + 1):
                for dx in range(-a, a + 1):
                    qy, qx = min(max(y + dy, 0), H - 1), min(max(x + dx, 0), W - 1)      # step 4: the nearest pixel inside
                    X, Y = ((f64(qx) + 0.5) - ci[2]) / ci[0], ((f64(qy) + 0.5) - ci[3]) / ci[1]
                    costs, n_in = [], 0
                    for j in nbr[i]:
                        cost = OUT
                        if 0 <= j < F:
                            A, b = view_terms(ci, cams[j])                          # step 2
                            front, fu, fv = project(A, b, cams[j], X, Y, f64(inv_depth[k]))
                            if front and fu >= 0 and fu < W and fv >= 0 and fv < H:
                                cost = bin(int(cen[i, qy, qx]) ^ int(cen[j, int(fv), int(fu)])).count('1')
                                n_in += 1
                        costs.append(cost)
                    total += sum(sorted(costs)[:m])                                 # step 3
                    if dy == 0 and dx == 0:
                        n_centre.append(n_in)
            C.append(total)
    kb = min(range(D), key=lambda k: (C[k], k))                                     # step 5
    second = min(C[k] for k in range(D) if abs(k - kb) > 1)
    if n_centre[kb] < m:                                                            # step 6
        status = UNSEEN
    elif kb == 0 or kb == D - 1:
        status = END
    elif not f64(C[kb]) <= uniq * f64(second):
        status = AMBIGUOUS
    else:
        status = ACCEPTED
    z, s = np.float32(0), np.float32(0)
    if status == ACCEPTED:
        z, s = refine(kb, C[kb], C[kb - 1], C[kb + 1], np.asarray(inv_depth, np.float64), std_planes)   # step 7
    return z, s, status, kb, C[kb], second

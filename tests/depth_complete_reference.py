"""Completing sparse depth priors by image-guided filtering as executable code: numpy float64, every product and
sum written out in the order libdepthcomp_hip.so follows.  Two forms that agree bit for bit: complete() over whole arrays, tap by
tap, and complete_scalar() pixel by pixel, step by step as DESIGN 8.10 numbers them.

    depth     float32 [F, H, W]: z-depth, valid iff > 0 (0, negatives and NaN are not)
    rgb       uint8 [F, H, W, 3]: the guide
    std_in    float32 [F, H, W] or None: the standard deviation of the own measurements; a value not > 0 counts as 0
    w_space   float64 [(2 r + 1)^2], row-major over (dy, dx);  w_colour float64 [766], indexed by |dR| + |dG| + |dB|

Both return a dict: depth, std, conf (float32), origin, pass (uint8) [F, H, W] and rows int64 [F, 4] = n_own, n_filled, n_refused,
n_none.
"""
import numpy as np

DEFAULTS = dict(radius=4, sigma_space=2.0, sigma_colour=20.0, iters=3, min_conf=0.02, min_points=2, max_rel_spread=0.1, decay=0.5)
ORIGIN_NONE, ORIGIN_OWN, ORIGIN_FILLED, ORIGIN_REFUSED = 0, 1, 2, 3
N_COLOUR = 766


def tables(radius, sigma_space, sigma_colour):
    """(w_space [(2 r + 1)^2], w_colour [766]) float64: the Gaussians the Python side builds (depth_complete.tables)"""
    d = np.arange(-radius, radius + 1, dtype=np.float64)
    w_space = np.exp(-(d[:, None] * d[:, None] + d[None, :] * d[None, :]) / (2.0 * sigma_space * sigma_space)).reshape(-1)
    s = np.arange(N_COLOUR, dtype=np.float64)
    return w_space, np.exp(-(s * s) / (2.0 * sigma_colour * sigma_colour))


def initial_state(depth, std_in):
    """(z, c, v) float32 [F, H, W]: own pixels z = depth, c = 1, v = float32(std_in * std_in) in float64; the others empty, all 0"""
    depth = np.asarray(depth, np.float32)
    own = depth > 0
    z = np.where(own, depth, np.float32(0)).astype(np.float32)
    c = own.astype(np.float32)
    v = np.zeros(depth.shape, np.float32)
    if std_in is not None:
        s = np.asarray(std_in, np.float32).astype(np.float64)
        with np.errstate(all='ignore'):
            v = np.where(own & (s > 0), s * s, 0.0).astype(np.float32)
    return z, c, v


def outputs(depth, z, c, v, status, pas):
    have = c > 0
    with np.errstate(all='ignore'):
        std = np.where(have, np.sqrt(v.astype(np.float64)), 0.0).astype(np.float32)
    origin = np.where(have, np.where(pas == 0, ORIGIN_OWN, ORIGIN_FILLED), status).astype(np.uint8)
    F = depth.shape[0]
    rows = np.stack([(origin == o).reshape(F, -1).sum(1) for o in (ORIGIN_OWN, ORIGIN_FILLED, ORIGIN_REFUSED, ORIGIN_NONE)], 1)
    return dict(depth=np.where(have, z, np.asarray(depth, np.float32)).astype(np.float32), std=std, conf=c.copy(), origin=origin,
                rows=rows.astype(np.int64), **{'pass': pas.copy()})


def complete(depth, rgb, std_in, w_space, w_colour, radius, iters, min_points=2, min_conf=0.02, max_rel_spread=0.1, decay=0.5,
             snapshots=None):
    """The whole-array form: one sweep over the frames per tap, taps in raster order.  snapshots: pass counts <= iters; the result is
    then {k: what a call with iters = k returns} (the state after pass k and that pass's refusals), all from one run."""
    depth, rgb = np.asarray(depth, np.float32), np.asarray(rgb, np.uint8)
    w_space, w_colour = np.asarray(w_space, np.float64).reshape(-1), np.asarray(w_colour, np.float64)
    F, H, W = depth.shape
    r, side = radius, 2 * radius + 1
    z, c, v = initial_state(depth, std_in)
    pas = np.zeros((F, H, W), np.uint8)
    status = np.zeros((F, H, W), np.uint8)
    col = rgb.astype(np.int64)
    colp = np.zeros((F, H + 2 * r, W + 2 * r, 3), np.int64)
    colp[:, r:r + H, r:r + W] = col
    inp = np.zeros((H + 2 * r, W + 2 * r), bool)
    inp[r:r + H, r:r + W] = True

    def pad(a):
        p = np.zeros((F, H + 2 * r, W + 2 * r), np.float64)
        p[:, r:r + H, r:r + W] = a
        return p
    with np.errstate(all='ignore'):
        taken, settled = {}, False
        for k in range(1, iters + 1):
            if settled:                                # a pass that filled nothing read the state it left: every later one repeats it
                if snapshots is not None and k in snapshots:
                    taken[k] = outputs(depth, z, c, v, status, pas)
                continue
            zp, cp, vp = pad(z), pad(c), pad(v)
            G, S, SZ, SZZ, SV = (np.zeros((F, H, W), np.float64) for _ in range(5))
            n = np.zeros((F, H, W), np.int64)
            for dy in range(-r, r + 1):
                for dx in range(-r, r + 1):
                    win = (slice(None), slice(r + dy, r + dy + H), slice(r + dx, r + dx + W))
                    inside = inp[win[1:]][None]
                    sad = np.abs(colp[win] - col).sum(-1)
                    g = np.where(inside, w_space[(dy + r) * side + dx + r] * w_colour[sad], 0.0)      # step 1
                    G = G + g
                    zq = zp[win]
                    gc = g * cp[win]                                                                    # step 2
                    use = gc > 0
                    gc = np.where(use, gc, 0.0)
                    n = n + use
                    S = S + gc
                    t = gc * zq
                    SZ = SZ + t
                    SZZ = SZZ + t * zq
                    SV = SV + gc * vp[win]
            empty = ~(c > 0)
            enough = (n >= min_points) & (G > 0)                                                        # step 3
            conf = S / G
            enough &= ~(conf < min_conf)
            mean = SZ / S                                                                               # step 4
            d = SZZ / S - mean * mean
            var = np.where(d > 0, d, 0.0)
            refused = enough & (np.sqrt(var) > max_rel_spread * mean)
            z32, c32, v32 = mean.astype(np.float32), (decay * conf).astype(np.float32), (var + SV / S).astype(np.float32)   # step 5
            fill = empty & enough & ~refused & np.isfinite(z32) & (z32 > 0) & (c32 > 0)
            z, c, v = np.where(fill, z32, z), np.where(fill, c32, c), np.where(fill, v32, v)
            pas = np.where(fill, np.uint8(k), pas)
            status = np.where(empty & refused, ORIGIN_REFUSED, ORIGIN_NONE).astype(np.uint8)
            settled = not fill.any()
            if snapshots is not None and k in snapshots:
                taken[k] = outputs(depth, z, c, v, status, pas)
    return outputs(depth, z, c, v, status, pas) if snapshots is None else taken


def complete_scalar(depth, rgb, std_in, w_space, w_colour, radius, iters, min_points=2, min_conf=0.02, max_rel_spread=0.1, decay=0.5):
    """The same pixel by pixel, in Python floats (IEEE float64), as DESIGN 8.10 numbers the steps"""
    depth, rgb = np.asarray(depth, np.float32), np.asarray(rgb, np.uint8)
    ws, wc = [float(x) for x in np.asarray(w_space, np.float64).reshape(-1)], [float(x) for x in np.asarray(w_colour, np.float64)]
    F, H, W = depth.shape
    r, side = radius, 2 * radius + 1
    z, c, v = initial_state(depth, std_in)
    pas = np.zeros((F, H, W), np.uint8)
    status = np.zeros((F, H, W), np.uint8)
    col = rgb.astype(np.int64).tolist()
    with np.errstate(all='ignore'):
        for k in range(1, iters + 1):
            z0, c0, v0 = z.astype(np.float64).tolist(), c.astype(np.float64).tolist(), v.astype(np.float64).tolist()   # state k - 1
            z, c, v = z.copy(), c.copy(), v.copy()
            status = np.zeros((F, H, W), np.uint8)
            for f in range(F):
                for y in range(H):
                    for x in range(W):
                        if c0[f][y][x] > 0:
                            continue                                    # carried unchanged
                        G = S = SZ = SZZ = SV = 0.0
                        n = 0
                        p = col[f][y][x]
                        for dy in range(-r, r + 1):
                            if not 0 <= y + dy < H:
                                continue
                            for dx in range(-r, r + 1):
                                if not 0 <= x + dx < W:
                                    continue
                                q = col[f][y + dy][x + dx]
                                g = ws[(dy + r) * side + dx + r] * wc[abs(p[0] - q[0]) + abs(p[1] - q[1]) + abs(p[2] - q[2])]   # 1
                                G += g
                                gc = g * c0[f][y + dy][x + dx]                                                           # 2
                                if gc > 0:
                                    zq = z0[f][y + dy][x + dx]
                                    n += 1
                                    S += gc
                                    t = gc * zq
                                    SZ += t
                                    SZZ += t * zq
                                    SV += gc * v0[f][y + dy][x + dx]
                        if n < min_points or not G > 0:                                                                  # 3
                            continue
                        conf = np.float64(S) / np.float64(G)
                        if conf < min_conf:
                            continue
                        mean = np.float64(SZ) / np.float64(S)                                                            # 4
                        d = np.float64(SZZ) / np.float64(S) - mean * mean
                        var = d if d > 0 else np.float64(0.0)
                        if np.sqrt(var) > np.float64(max_rel_spread) * mean:
                            status[f, y, x] = ORIGIN_REFUSED
                            continue
                        z32, c32 = np.float32(mean), np.float32(np.float64(decay) * conf)                                # 5
                        v32 = np.float32(var + np.float64(SV) / np.float64(S))
                        if np.isfinite(z32) and z32 > 0 and c32 > 0:
                            z[f, y, x], c[f, y, x], v[f, y, x], pas[f, y, x] = z32, c32, v32, k
    return outputs(depth, z, c, v, status, pas)


# ------------------------------------------------------------------------------------------------------------ inputs of the tests
def guide(depth_true, seed=0):
    """A guide image that follows the surfaces: a colour per depth layer (its integer part), plus noise of a few levels"""
    rs = np.random.RandomState(seed)
    palette = rs.randint(0, 256, (64, 3))
    layer = np.clip(np.floor(np.nan_to_num(np.asarray(depth_true, np.float64))), 0, 63).astype(np.int64)
    return np.clip(palette[layer] + rs.randint(-3, 4, layer.shape + (3,)), 0, 255).astype(np.uint8)

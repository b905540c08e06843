"""Densifying sparse depth priors from neighbouring frames as executable code: numpy float64, every product and
sum written out element by element in the order libdepthacc_hip.so follows (no `@`, no dot: BLAS may fuse or reorder).  Two forms
that agree: accumulate() over whole arrays and accumulate_scalar() pixel by pixel, step by step as DESIGN 8.8 numbers them.

Conventions (those of tests/depth_consistency_reference.py): frame i has fx, fy, cx, cy and a camera-to-world [R_i | t_i] in the
OpenCV convention; depth is float32 z-depth, valid iff d > 0 (0, negatives and NaN are not); pixel centres sit at +0.5.

    cams   float64 [F, 16]: fx fy cx cy, then the 12 values of the 3 x 4 camera-to-world, row-major
    nbr    int [F, V]: the frames whose measurements are taken into a frame, slot by slot; j < 0 (and j >= F) is skipped
"""
import numpy as np

from tests.depth_consistency_reference import pack_cams, to_world, to_cam          # noqa: F401  (the same written order)

DEFAULTS = dict(occl_radius=2, occl_tol=0.05)
EMPTY = np.uint64(0xFFFFFFFFFFFFFFFF)
ORIGIN_NONE, ORIGIN_OWN, ORIGIN_ADDED, ORIGIN_HIDDEN = 0, 1, 2, 3


def scatter(depth, cams, nbr):
    """Pass A: zbuf uint64 [F, H, W], the smallest key (z bits << 32 | slot << 28 | source pixel) that reached every pixel, all ones
    where none did.  (The library leaves out the keys of pixels that have a measurement of their own: nothing reads them.)"""
    F, H, W = depth.shape
    zbuf = np.full((F, H * W), EMPTY, np.uint64)
    ys, xs = np.meshgrid(np.arange(H), np.arange(W), indexing='ij')
    with np.errstate(all='ignore'):
        for i in range(F):
            ci = cams[i]
            for v, j in enumerate(nbr[i]):
                if j < 0 or j >= F:
                    continue
                cj = cams[j]
                valid = depth[j] > 0
                y, x = ys[valid], xs[valid]
                d = depth[j][valid].astype(np.float64)
                P = to_cam(ci, to_world(cj, x + 0.5, y + 0.5, d))                  # steps 1 - 3
                ok = P[2] > 0                                                       # step 4
                u = ci[0] * (P[0] / P[2]) + ci[2]                                   # step 5
                w = ci[1] * (P[1] / P[2]) + ci[3]
                ok &= (u >= 0) & (u < W) & (w >= 0) & (w < H)                       # step 6: in float64; a NaN is outside
                px, py = np.floor(np.where(ok, u, 0)).astype(np.int64), np.floor(np.where(ok, w, 0)).astype(np.int64)   # step 7
                z32 = P[2].astype(np.float32)                                       # step 8: to nearest
                ok &= np.isfinite(z32) & (z32 > 0)
                key = (z32.view(np.uint32).astype(np.uint64) << np.uint64(32)) | np.uint64(v << 28) | (y * W + x).astype(np.uint64)   # step 9
                np.minimum.at(zbuf[i], (py * W + px)[ok], key[ok])                  # step 10
    return zbuf.reshape(F, H, W)


def window_min(surface, r):
    """the minimum of surface [F, H, W] over the (2 r + 1)^2 window of every pixel, clipped to the frame"""
    F, H, W = surface.shape
    pad = np.full((F, H + 2 * r, W + 2 * r), np.inf, np.float32)
    pad[:, r:r + H, r:r + W] = surface
    out = surface.copy()
    for dy in range(2 * r + 1):
        for dx in range(2 * r + 1):
            out = np.minimum(out, pad[:, dy:dy + H, dx:dx + W])
    return out


def resolve(depth, zbuf, occl_radius=2, occl_tol=0.05):
    """Pass B: {'depth_out' float32, 'origin' uint8, 'src' int32 [F, H, W], 'rows' int64 [F, 4]}"""
    F, H, W = depth.shape
    own_valid = depth > 0
    cand = ~own_valid & (zbuf != EMPTY)
    z = (zbuf >> np.uint64(32)).astype(np.uint32).view(np.float32)
    surface = np.where(own_valid, depth, np.where(cand, z, np.float32(np.inf))).astype(np.float32)
    zmin = window_min(surface, int(occl_radius))
    with np.errstate(all='ignore'):
        hidden = cand & (z.astype(np.float64) > zmin.astype(np.float64) * (1.0 + float(occl_tol)))
    added = cand & ~hidden
    depth_out = depth.copy()                                    # what is not replaced passes through bit for bit
    depth_out[added] = z[added]
    origin = np.where(own_valid, ORIGIN_OWN, np.where(added, ORIGIN_ADDED, np.where(hidden, ORIGIN_HIDDEN, ORIGIN_NONE))).astype(np.uint8)
    src = np.where(cand, (zbuf & np.uint64(0xFFFFFFFF)).astype(np.uint32).view(np.int32), np.int32(-1)).astype(np.int32)
    n = lambda m: m.reshape(F, -1).sum(1)
    rows = np.stack([n(own_valid), n(cand), n(added), n(hidden)], 1).astype(np.int64)
    return dict(depth_out=depth_out, origin=origin, src=src, rows=rows)


def _inputs(depth, cams, nbr):
    depth = np.asarray(depth)
    assert depth.dtype == np.float32 and depth.ndim == 3
    return depth, np.asarray(cams, np.float64), np.asarray(nbr, np.int64).reshape(depth.shape[0], -1)


def accumulate(depth, cams, nbr, occl_radius=2, occl_tol=0.05):
    """The vectorised form: {'depth_out', 'origin', 'src', 'rows'} of depth float32 [F, H, W]"""
    depth, cams, nbr = _inputs(depth, cams, nbr)
    return resolve(depth, scatter(depth, cams, nbr), occl_radius, occl_tol)


def accumulate_scalar(depth, cams, nbr, occl_radius=2, occl_tol=0.05):
    """The scalar form, one pixel at a time in Python scalars: the same dict"""
    depth, cams, nbr = _inputs(depth, cams, nbr)
    F, H, W = depth.shape
    f64, r = np.float64, int(occl_radius)
    zbuf = [[[int(EMPTY)] * W for _ in range(H)] for _ in range(F)]
    with np.errstate(all='ignore'):
        for i in range(F):
            ci = cams[i]
            for v, j in enumerate(nbr[i]):
                if j < 0 or j >= F:
                    continue
                cj = cams[j]
                for y in range(H):
                    for x in range(W):
                        d32 = depth[j, y, x]
                        if not d32 > 0:
                            continue
                        P = to_cam(ci, to_world(cj, f64(x) + 0.5, f64(y) + 0.5, f64(d32)))       # steps 1 - 3
                        if not P[2] > 0:                                                          # step 4
                            continue
                        u, w = ci[0] * (P[0] / P[2]) + ci[2], ci[1] * (P[1] / P[2]) + ci[3]       # step 5
                        if not (u >= 0 and u < W and w >= 0 and w < H):                           # step 6
                            continue
                        px, py = int(np.floor(u)), int(np.floor(w))                               # step 7
                        z32 = np.float32(P[2])                                                    # step 8
                        if not (np.isfinite(z32) and z32 > 0):
                            continue
                        key = (int(z32.view(np.uint32)) << 32) | (v << 28) | (y * W + x)          # step 9
                        zbuf[i][py][px] = min(zbuf[i][py][px], key)                               # step 10
        depth_out = depth.copy()
        origin, src, rows = np.zeros((F, H, W), np.uint8), np.full((F, H, W), -1, np.int32), np.zeros((F, 4), np.int64)

        def surface(i, y, x):
            if depth[i, y, x] > 0:
                return depth[i, y, x]
            key = zbuf[i][y][x]
            return np.float32(np.inf) if key == int(EMPTY) else np.uint32(key >> 32).view(np.float32)
        for i in range(F):
            for y in range(H):
                for x in range(W):
                    if depth[i, y, x] > 0:
                        origin[i, y, x] = ORIGIN_OWN
                        rows[i, 0] += 1
                        continue
                    key = zbuf[i][y][x]
                    if key == int(EMPTY):
                        continue
                    z = np.uint32(key >> 32).view(np.float32)
                    zmin = min(surface(i, yy, xx) for yy in range(max(0, y - r), min(H, y + r + 1))
                               for xx in range(max(0, x - r), min(W, x + r + 1)))
                    src[i, y, x] = np.uint32(key & 0xFFFFFFFF).view(np.int32)
                    rows[i, 1] += 1
                    if f64(z) > f64(zmin) * (1.0 + float(occl_tol)):
                        origin[i, y, x] = ORIGIN_HIDDEN
                        rows[i, 3] += 1
                    else:
                        origin[i, y, x], depth_out[i, y, x] = ORIGIN_ADDED, z
                        rows[i, 2] += 1
    return dict(depth_out=depth_out, origin=origin, src=src, rows=rows)

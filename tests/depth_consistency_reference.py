"""The multi-view consistency check of depth priors as executable code: numpy float64, every product and sum
written out element by element in the order libdepthcons_hip.so follows (no `@`, no dot: BLAS may fuse or reorder).

Conventions: frame i has fx, fy, cx, cy and a camera-to-world [R_i | t_i] in the OpenCV convention (x right, y down, z forward);
depth is z-depth in scene units; pixel centres sit at +0.5; a depth is valid iff d > 0 (0, negatives and NaN pass through).

    cams   float64 [F, 16]: fx fy cx cy, then the 12 values of the 3 x 4 camera-to-world, row-major
    nbr    int [F, K]: the frames a frame is checked against, in list order; j < 0 (and j >= F) is skipped
"""
import numpy as np

DEFAULTS = dict(pix_tol=1.0, rel_tol=0.01, min_views=2, keep_unverified=True, std_floor=0.0)


def pack_cams(fx, fy, cx, cy, c2w):
    """cams [F, 16] float64 of per-frame (or shared scalar) intrinsics and c2w [F, 3 or 4, 4]"""
    c2w = np.asarray(c2w, np.float64)
    F = c2w.shape[0]
    out = np.empty((F, 16), np.float64)
    for k, v in enumerate((fx, fy, cx, cy)):
        out[:, k] = np.broadcast_to(np.asarray(v, np.float64), (F,))
    out[:, 4:] = c2w[:, :3, :4].reshape(F, 12)
    return out


def to_world(c, px, py, d):
    """pixel (px, py) at z-depth d of camera c [16] -> world: Pc = ((px - cx) / fx * d, (py - cy) / fy * d, d), Pw = R Pc + t"""
    xc = (px - c[2]) / c[0] * d
    yc = (py - c[3]) / c[1] * d
    return (((c[4] * xc + c[5] * yc) + c[6] * d) + c[7],
            ((c[8] * xc + c[9] * yc) + c[10] * d) + c[11],
            ((c[12] * xc + c[13] * yc) + c[14] * d) + c[15])


def to_cam(c, w):
    """world -> camera c: R^T (Pw - t)"""
    dx, dy, dz = w[0] - c[7], w[1] - c[11], w[2] - c[15]
    return ((c[4] * dx + c[8] * dy) + c[12] * dz,
            (c[5] * dx + c[9] * dy) + c[13] * dz,
            (c[6] * dx + c[10] * dy) + c[14] * dz)


def check(depth, cams, nbr, pix_tol=1.0, rel_tol=0.01, min_views=2, keep_unverified=True, std_floor=0.0):
    """{'depth_out', 'std_out': float32 [F, H, W], 'counts': uint8 [F, H, W, 2] (n_seen, n_ok), 'keep': bool [F, H, W] (of the valid
    pixels), 'rows': int64 [F, 4] (n_valid, n_verifiable, n_kept, n_dropped)} of depth float32 [F, H, W]"""
    depth = np.asarray(depth)
    assert depth.dtype == np.float32 and depth.ndim == 3
    cams = np.asarray(cams, np.float64)
    F, H, W = depth.shape
    nbr = np.asarray(nbr, np.int64).reshape(F, -1)
    pix_tol, rel_tol, std_floor = float(pix_tol), float(rel_tol), float(std_floor)
    pix_tol2 = pix_tol * pix_tol
    depth_out = depth.copy()
    std_out = np.zeros((F, H, W), np.float32)
    counts = np.zeros((F, H, W, 2), np.uint8)
    keep_all = np.zeros((F, H, W), bool)
    rows = np.zeros((F, 4), np.int64)
    ys, xs = np.meshgrid(np.arange(H), np.arange(W), indexing='ij')
    with np.errstate(all='ignore'):
        for i in range(F):
            valid = depth[i] > 0
            y, x = ys[valid], xs[valid]
            d = depth[i][valid].astype(np.float64)
            px, py = x + 0.5, y + 0.5
            ci = cams[i]
            pw = to_world(ci, px, py, d)
            n_seen, n_ok, s = np.zeros(d.shape, np.int64), np.zeros(d.shape, np.int64), np.zeros(d.shape, np.float64)
            for j in nbr[i]:
                if j < 0 or j >= F:
                    continue
                cj = cams[j]
                pj = to_cam(cj, pw)
                alive = ~(pj[2] <= 0)
                u = cj[0] * (pj[0] / pj[2]) + cj[2]
                v = cj[1] * (pj[1] / pj[2]) + cj[3]
                xi, yi = np.floor(u), np.floor(v)
                alive &= (xi >= 0) & (xi < W) & (yi >= 0) & (yi < H)                # a NaN is outside
                xi_s, yi_s = np.where(alive, xi, 0).astype(np.int64), np.where(alive, yi, 0).astype(np.int64)
                dj32 = depth[j][yi_s, xi_s]
                alive &= dj32 > 0
                n_seen += alive
                qi = to_cam(ci, to_world(cj, xi + 0.5, yi + 0.5, dj32.astype(np.float64)))
                alive &= ~(qi[2] <= 0)
                du = (ci[0] * (qi[0] / qi[2]) + ci[2]) - px
                dv = (ci[1] * (qi[1] / qi[2]) + ci[3]) - py
                e_pix2 = du * du + dv * dv
                e = qi[2] - d
                ok = alive & (e_pix2 <= pix_tol2) & (np.abs(e) <= rel_tol * d)     # a NaN is not ok
                n_ok += ok
                s = np.where(ok, s + e * e, s)
            verifiable = n_seen >= min_views
            keep = np.where(verifiable, n_ok >= min_views, bool(keep_unverified))
            spread = np.where(n_ok > 0, np.sqrt(s / np.maximum(n_ok, 1)), rel_tol * d)
            spread = np.where(spread < std_floor, std_floor, spread)
            depth_out[i][y, x] = np.where(keep, depth[i][valid], np.float32(0))
            std_out[i][y, x] = np.where(keep, spread, 0.0).astype(np.float32)
            counts[i][y, x, 0], counts[i][y, x, 1] = n_seen, n_ok
            keep_all[i][y, x] = keep
            rows[i] = (d.size, int(verifiable.sum()), int(keep.sum()), d.size - int(keep.sum()))
    return dict(depth_out=depth_out, std_out=std_out, counts=counts, keep=keep_all, rows=rows)


def check_pixel(depth, cams, nbr, i, y, x, pix_tol=1.0, rel_tol=0.01, min_views=2, keep_unverified=True, std_floor=0.0):
    """One pixel, step by step as DESIGN 8.7 numbers them: (depth_out, std_out, n_seen, n_ok).  The scalar twin of check()."""
    F, H, W = depth.shape
    d32 = depth[i, y, x]
    if not d32 > 0:
        return d32, np.float32(0), 0, 0
    f64 = np.float64
    d, px, py = f64(d32), f64(x) + 0.5, f64(y) + 0.5
    cams = np.asarray(cams, np.float64)
    ci = cams[i]
    pw = to_world(ci, px, py, d)
    n_seen, n_ok, s = 0, 0, f64(0)
    with np.errstate(all='ignore'):
        for j in np.asarray(nbr).reshape(F, -1)[i]:
            if j < 0 or j >= F:
                continue
            cj = cams[j]
            pj = to_cam(cj, pw)                                                  # step 1
            if pj[2] <= 0:
                continue
            u, v = cj[0] * (pj[0] / pj[2]) + cj[2], cj[1] * (pj[1] / pj[2]) + cj[3]   # step 2
            xi, yi = np.floor(u), np.floor(v)
            if not (xi >= 0 and xi < W and yi >= 0 and yi < H):
                continue
            dj = depth[j, int(yi), int(xi)]
            if not dj > 0:
                continue
            n_seen += 1
            qi = to_cam(ci, to_world(cj, xi + 0.5, yi + 0.5, f64(dj)))             # step 3
            if qi[2] <= 0:
                continue
            du, dv = (ci[0] * (qi[0] / qi[2]) + ci[2]) - px, (ci[1] * (qi[1] / qi[2]) + ci[3]) - py
            e = qi[2] - d
            if du * du + dv * dv <= f64(pix_tol) * f64(pix_tol) and abs(e) <= f64(rel_tol) * d:
                n_ok += 1
                s = s + e * e
        keep = (n_ok >= min_views) if n_seen >= min_views else bool(keep_unverified)   # step 4
        if not keep:
            return np.float32(0), np.float32(0), n_seen, n_ok
        spread = np.sqrt(s / n_ok) if n_ok > 0 else f64(rel_tol) * d               # step 5
        return d32, np.float32(spread if not spread < std_floor else std_floor), n_seen, n_ok

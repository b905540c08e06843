"""The sparse depth prior from a point cloud with tracks as executable code: numpy float64, every product and sum
written out element by element in the order libdepthpoints_hip.so follows (no `@`, no dot: BLAS may fuse or reorder), with loops
where vectorising would reorder a sum or a minimum.

Conventions (those of tests/depth_consistency_reference.py): frame i has fx, fy, cx, cy and a camera-to-world [R_i | t_i] in the
OpenCV convention; depth is z-depth; pixel centres sit at +0.5.

    cams    float64 [F, 16]: fx fy cx cy, then the 12 values of the 3 x 4 camera-to-world, row-major
    points  float64 [P, 4]: x y z in the cameras' world, then coef (the standard deviation of a pixel at depth z is coef z^2 / fx)
    obs     int [T, 2] = (point, frame), or None: every point into every frame
"""
import numpy as np

from tests.depth_consistency_reference import pack_cams, to_cam          # noqa: F401  (the same written order)

DEFAULTS = dict(near=0.5, far=200.0, occl_radius=0, occl_tol=0.05, std_scale=1.0, std_floor=0.0)
EMPTY = int(0xFFFFFFFFFFFFFFFF)
ORIGIN_NONE, ORIGIN_POINT, ORIGIN_HIDDEN = 0, 1, 2


# ------------------------------------------------------------------------------------------------------ host selection
def select(xyz, error, off, track_pos, centres, frame_of, max_error=2.0, min_track=3, err_floor=0.5):
    """(points float64 [P', 4], obs int32 [T', 2], kept bool [P]) of a cloud already in the scene's frame.  xyz [P, 3], error [P];
    the track of point p is track_pos[off[p]:off[p + 1]], positions into centres [N, 3] (all the model's cameras, scene frame);
    frame_of [N]: a camera's position in the split, or -1.  One point at a time, every sum in the written order."""
    points, obs, kept = [], [], np.zeros(len(xyz), bool)
    for p in range(len(xyz)):
        track = [int(v) for v in track_pos[off[p]:off[p + 1]]]
        if not (np.all(np.isfinite(xyz[p])) and 0 <= error[p] <= max_error and len(track) >= min_track):
            continue
        c = centres[track]
        dx, dy, dz = (c[:, k].max() - c[:, k].min() for k in range(3))
        B = np.sqrt((dx * dx + dy * dy) + dz * dz)
        if not B > 0:
            continue
        kept[p] = True
        new = len(points)
        points.append((xyz[p, 0], xyz[p, 1], xyz[p, 2], max(float(error[p]), float(err_floor)) / B))
        obs += [(new, int(frame_of[v])) for v in track if frame_of[v] >= 0]
    obs = sorted(obs, key=lambda r: (r[1], r[0]))
    return np.array(points, np.float64).reshape(-1, 4), np.array(obs, np.int32).reshape(-1, 2), kept


# --------------------------------------------------------------------------------------------------------- the call
def project(c, w, near, far, H, W):
    """steps 1 - 6 of one point w (x, y, z) and one camera c [16]: (pixel index, z32) or None"""
    with np.errstate(all='ignore'):
        x, y, z = to_cam(c, w)                                           # step 1
        if not (z >= near and z <= far):                                 # step 2 (a NaN fails; far is finite, so z is)
            return None
        u, v = c[0] * x / z + c[2], c[1] * y / z + c[3]                  # step 3
        if not (u >= 0 and u < W and v >= 0 and v < H):                  # step 4: in float64; a NaN is outside
            return None
        px, py = int(np.floor(u)), int(np.floor(v))                      # step 5
        z32 = np.float32(z)                                              # step 6: to nearest
        if not (z32 > 0 and np.isfinite(z32)):
            return None
        return py * W + px, z32


def scatter(cams, points, obs, shape, near, far):
    """Pass A: (zbuf [F][H * W] of Python ints: the smallest key (z bits << 32 | point) that reached every pixel, all ones where none
    did; n_obs [F]; n_projected [F])"""
    F, H, W = shape
    P = len(points)
    zbuf = [[EMPTY] * (H * W) for _ in range(F)]
    n_obs, n_proj = np.zeros(F, np.int64), np.zeros(F, np.int64)
    f64 = np.float64
    if obs is None:
        pairs = ((p, f) for f in range(F) for p in range(P))
    else:
        pairs = ((int(p), int(f)) for p, f in np.asarray(obs).reshape(-1, 2))
    for p, f in pairs:
        if not (0 <= p < P and 0 <= f < F):                              # a row outside the tables is skipped
            continue
        n_obs[f] += 1
        hit = project(cams[f], (f64(points[p, 0]), f64(points[p, 1]), f64(points[p, 2])), f64(near), f64(far), H, W)
        if hit is None:
            continue
        n_proj[f] += 1
        t, z32 = hit
        key = (int(z32.view(np.uint32)) << 32) | p                       # step 7
        zbuf[f][t] = min(zbuf[f][t], key)                                # step 8
    return zbuf, n_obs, n_proj


def resolve(cams, points, zbuf, shape, occl_radius, occl_tol, std_scale, std_floor):
    """Pass B: depth_out, std_out float32, point int32, origin uint8 [F, H, W], (n_kept, n_hidden) [F, 2]"""
    F, H, W = shape
    f64, r = np.float64, int(occl_radius)
    depth = np.zeros(shape, np.float32)
    std = np.zeros(shape, np.float32)
    point = np.full(shape, -1, np.int32)
    origin = np.zeros(shape, np.uint8)
    counts = np.zeros((F, 2), np.int64)
    for f in range(F):
        keys = np.array(zbuf[f], np.uint64).reshape(H, W)
        has = keys != np.uint64(EMPTY)
        z = (keys >> np.uint64(32)).astype(np.uint32).view(np.float32)
        surf = np.where(has, z, np.float32(np.inf)).astype(np.float32)
        for y, x in zip(*np.nonzero(has)):
            zmin = surf[max(0, y - r):y + r + 1, max(0, x - r):x + r + 1].min()      # (a minimum of float32 values: any order)
            if f64(z[y, x]) > f64(zmin) * (1.0 + f64(occl_tol)):
                origin[f, y, x] = ORIGIN_HIDDEN
                counts[f, 1] += 1
                continue
            idx = int(keys[y, x] & np.uint64(0xFFFFFFFF))
            zd = f64(z[y, x])
            with np.errstate(all='ignore'):
                s = f64(std_scale) * f64(points[idx, 3]) * zd * zd / f64(cams[f, 0])
            origin[f, y, x], depth[f, y, x], point[f, y, x] = ORIGIN_POINT, z[y, x], idx
            std[f, y, x] = np.float32(f64(std_floor) if s < f64(std_floor) else s)
            counts[f, 0] += 1
    return depth, std, point, origin, counts


def splat(cams, points, obs, shape, near=0.5, far=200.0, occl_radius=0, occl_tol=0.05, std_scale=1.0, std_floor=0.0):
    """{'depth_out', 'std_out' float32, 'point' int32, 'origin' uint8 [F, H, W], 'rows' int64 [F, 4]}"""
    cams = np.asarray(cams, np.float64)
    points = np.asarray(points, np.float64).reshape(-1, 4)
    shape = tuple(int(v) for v in shape)
    assert cams.shape == (shape[0], 16)
    zbuf, n_obs, n_proj = scatter(cams, points, obs, shape, near, far)
    depth, std, point, origin, counts = resolve(cams, points, zbuf, shape, occl_radius, occl_tol, std_scale, std_floor)
    rows = np.stack([n_obs, n_proj, counts[:, 0], counts[:, 1]], 1).astype(np.int64)
    return dict(depth_out=depth, std_out=std, point=point, origin=origin, rows=rows)

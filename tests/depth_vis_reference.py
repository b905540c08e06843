"""numpy float64 restatement of the depth pictures: what libdepthvis_hip.so is held to.

Percentiles: upstream's vis.weighted_percentile -- stable argsort (NaN last), running sum of the weights, np.interp -- with the
straddling bin (j, w_j) of every percentile, which the tests' error gate needs.  Pictures: visualize_cmap / matte /
visualize_coord_mod of mipnerf360/internal/vis.py and colorize_np of nerfplusplus/utils.py, to the bytes of the PNG, with a
`fragile` mask: the pixels whose quantity in front of a floor (t * 256 at the colour table, v * 255 at the byte) is within 1e-9
of an integer without being one, where a last-bit difference of `log` may move the byte.  (An exact integer comes from a clip
to 0 or 1, the matte's constants or float32 rounding, which IEEE arithmetic repeats bit for bit.)  Behind a colour table only
the table's index can move: the byte is then IEEE arithmetic on a table row, the same bits everywhere, and many rows of jet
are k / 255 to the last bit, so the quantity at the byte is not looked at there.
"""
import os

import numpy as np

EPS32 = float(np.finfo(np.float32).eps)
TABLES = dict(np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'colormaps.npz')))
CURVES = {'identity': lambda x: x, 'neg_log': lambda x: -np.log(x + EPS32), 'log': lambda x: np.log(x + EPS32)}
SUITE_PS = (0.5, 99.5)


def weighted_percentile(value, weight, ps):
    """(result [P], j [P], w_j [P], sorted value, cw): np.interp(ps * (cw[-1] / 100), cw, sorted value) written out.  j is the
    last index whose running sum is <= q (-1: none, N - 1: q is at or past the end) and w_j = cw[j + 1] - cw[j] the weight of
    the straddling element (nan where there is none)."""
    x = np.asarray(value, np.float32).reshape(-1)
    w = np.asarray(weight, np.float32).reshape(-1).astype(np.float64)
    order = np.argsort(x, kind='stable')
    x, w = x[order].astype(np.float64), w[order]
    cw = np.cumsum(w)
    n = x.size
    out, js, wjs = [], [], []
    for p in ps:
        q = float(p) * (cw[-1] / 100)
        j = int(np.searchsorted(cw, q, side='right')) - 1     # the last index with cw[j] <= q
        wj = np.nan
        with np.errstate(invalid='ignore', divide='ignore'):
            if not q == q or j >= n - 1:
                r, j = x[-1], n - 1
            elif j < 0:
                r = x[0]
            elif cw[j] == q:
                r = x[j]
            else:
                wj = cw[j + 1] - cw[j]
                slope = (x[j + 1] - x[j]) / wj
                r = slope * (q - cw[j]) + x[j]
                if np.isnan(r):
                    r = slope * (q - cw[j + 1]) + x[j + 1]
                    if np.isnan(r) and x[j] == x[j + 1]:
                        r = x[j]
        out.append(r)
        js.append(j)
        wjs.append(wj)
    return np.array(out, np.float64), np.array(js), np.array(wjs, np.float64), x, cw


def percentiles(value, weight, ps):
    return weighted_percentile(value, weight, ps)[0]


def minmax(x):
    """float32 (min, max, nanmin, nanmax) as numpy gives them"""
    x = np.asarray(x, np.float32).reshape(-1)
    with np.errstate(invalid='ignore'), np.testing.suppress_warnings() as sup:
        sup.filter(RuntimeWarning)
        return np.array([x.min(), x.max(), np.nanmin(x) if not np.isnan(x).all() else np.nan,
                         np.nanmax(x) if not np.isnan(x).all() else np.nan], np.float32)


def cmap_lookup(t, name):
    """matplotlib's lookup of float32 t: row clamp(floor(t * 256), 0, 255) of the 256 x 3 table, NaN -> (0, 0, 0).
    Returns (colours float64 [..., 3], the float64 quantity in front of the floor)."""
    t = np.asarray(t, np.float32)
    pre = t.astype(np.float64) * 256
    with np.errstate(invalid='ignore'):
        idx = np.clip(np.floor(np.where(np.isnan(pre), 0, pre)), 0, 255).astype(np.int64)
    c = TABLES[name][idx]
    c[np.isnan(t)] = 0.0
    return c, pre


def _near_integer(q):
    with np.errstate(invalid='ignore'):
        d = np.abs(q - np.rint(q))
        return np.isfinite(q) & (d > 0) & (d < 1e-9)


def to_bytes(v):
    """(uint8 bytes of clip(nan_to_num(v), 0, 1) * 255 truncated, fragile [...] over the last axis)"""
    pre = np.clip(np.nan_to_num(v), 0., 1.) * 255.
    return pre.astype(np.uint8), _near_integer(pre).any(-1)


def matte_bg(H, W):
    mask = np.logical_xor((np.arange(H) % 16 // 8)[:, None], (np.arange(W) % 16 // 8)[None, :])
    return np.where(mask, 1.0, 0.8)


def matte(vis, acc):
    acc = np.asarray(acc, np.float32).astype(np.float64)
    return vis * acc[:, :, None] + (matte_bg(*acc.shape) * (1 - acc))[:, :, None]


def unit_interval(value, lo_auto, hi_auto, curve):
    """nan_to_num(clip((c(value) - min(c(lo), c(hi))) / |c(hi) - c(lo)|, 0, 1)), lo = lo_auto - eps, hi = hi_auto + eps"""
    fn = CURVES[curve]
    with np.errstate(invalid='ignore', divide='ignore'):
        v = fn(np.asarray(value, np.float32).astype(np.float64))
        lo, hi = fn(np.float64(lo_auto) - EPS32), fn(np.float64(hi_auto) + EPS32)
        return np.nan_to_num(np.clip((v - np.minimum(lo, hi)) / np.abs(hi - lo), 0, 1))


def visualize_cmap(value, acc, cmap='turbo', curve='neg_log', lohi=None, ps=SUITE_PS):
    """(bytes uint8 [H, W, 3], fragile [H, W], (lo_auto, hi_auto)).  cmap None: the 3-channel form (depth_triplet), whose
    percentiles give every channel entry its pixel's acc."""
    value, acc = np.asarray(value, np.float32), np.asarray(acc, np.float32)
    if lohi is None:
        w = acc if cmap is not None else np.repeat(acc[..., None], 3, -1)
        lohi = percentiles(value, w, ps)
    t = unit_interval(value, lohi[0], lohi[1], curve)
    if cmap is not None:
        c, pre = cmap_lookup(t.astype(np.float32), cmap)
        fragile = _near_integer(pre)
    else:
        c, fragile = t, np.zeros(acc.shape, bool)
    b, fr = to_bytes(matte(c, acc))
    return b, fragile if cmap is not None else fr, (float(lohi[0]), float(lohi[1]))


def colorize_minmax(x, cmap='jet'):
    """colorize_np without a mask or colour bar: (bytes, fragile, (vmin, vmax)); float32 arithmetic in front of the table"""
    x = np.asarray(x, np.float32)
    mm = minmax(x)
    vmin, vmax = mm[0], np.float32(mm[1] + np.float32(1e-6))
    with np.errstate(invalid='ignore', divide='ignore'):
        t = ((x - vmin) / np.float32(vmax - vmin)).astype(np.float32)
    c, pre = cmap_lookup(t, cmap)
    return to_bytes(c)[0], _near_integer(pre), (float(vmin), float(vmax))


def matte_rgb(rgb, acc):
    return to_bytes(matte(np.asarray(rgb, np.float32).astype(np.float64), acc))


def coords_mod(origins, directions, distance, acc):
    o, d = np.asarray(origins, np.float32).astype(np.float64), np.asarray(directions, np.float32).astype(np.float64)
    dist = np.asarray(distance, np.float32).astype(np.float64)
    with np.errstate(invalid='ignore'):
        coords = o + d * dist[..., None]
        return to_bytes(matte(((coords + 1) % 2) / 2, acc))


def effective_acc(acc, distance_mean):
    return np.where(np.isnan(distance_mean), np.float32(0), np.asarray(acc, np.float32)).astype(np.float32)


def triplet_value(distance_median, p5, p95):
    med = np.asarray(distance_median, np.float32)
    return np.stack([np.float32(2) * med - np.asarray(p5, np.float32), med, np.asarray(p95, np.float32)], -1).astype(np.float32)


def mip360_suite(rgb, acc, dmean, dmedian, p5, p95, origins, directions):
    """{name: (bytes, fragile)} of one frame's five pictures, plus 'lohi_*'"""
    acc = effective_acc(acc, dmean)
    out = {}
    for key, v in (('mean', dmean), ('median', dmedian)):
        b, fr, lohi = visualize_cmap(v, acc, 'turbo', 'neg_log')
        out['depth_' + key], out['lohi_' + key] = (b, fr), lohi
    b, fr, lohi = visualize_cmap(triplet_value(dmedian, p5, p95), acc, None, 'log')
    out['depth_triplet'], out['lohi_triplet'] = (b, fr), lohi
    out['color_matte'] = matte_rgb(rgb, acc)
    out['coords_mod'] = coords_mod(origins, directions, dmean, acc)
    return out

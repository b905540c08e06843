"""The depth-error metrics of DESIGN.md 8.5 as numpy: with that text, the definition libdepthmetrics_hip.so is held to.

Per frame: pred, gt [H, W] float32 in scene units and one scale.  The division by float32(scale), the valid mask, the clip and the
error map are float32, exactly what the evaluators' host function (eval_outputs.depth_errors)
computes with a Python-float scale; the nine numbers are float64 sums over the valid pixels of terms formed in float64 from the
float32 g and vp."""
import numpy as np

METRIC_NAMES = ('n_valid', 'rmse', 'absrel', 'sqrel', 'absdiff', 'rmse_log', 'a1', 'a2', 'a3')
LO, HI = np.float32(1e-3), np.float32(80.0)
THRESHOLDS = (1.25, 1.5625, 1.953125)
U53 = 2.0 ** -53
LOG_ATOL = 1.5e-14       # (3 + 1) ulp of a float64 log of magnitude <= log(1000) = 6.91 (2^-51 there), twice: see rmse_log_gate


def prepare(pred, gt, scale):
    """(g, vp, valid, err_map): float32 metres, the clipped prediction (a NaN stays NaN), the valid mask, |g - vp| on it"""
    pred, gt = np.asarray(pred, np.float32), np.asarray(gt, np.float32)
    s = np.float32(scale)
    with np.errstate(invalid='ignore', divide='ignore', over='ignore'):
        g, p = gt / s, pred / s
        valid = (g < HI) & (g > LO)
        vp = np.where(p < LO, LO, np.where(p > HI, HI, p)).astype(np.float32)
        err = np.where(valid, np.abs(g - vp), np.float32(0)).astype(np.float32)
    return g, vp, valid, err


def frame_metrics(pred, gt, scale):
    """dict: 'row' float64 [9] (METRIC_NAMES), 'valid' bool [H, W], 'err_map' float32 [H, W], 'near' -- how many thresh values
    of the frame lie within 1e-12 relative of one of the three thresholds (where a last-bit difference could move a count)"""
    g, vp, valid, err = prepare(pred, gt, scale)
    G, V = g[valid].astype(np.float64), vp[valid].astype(np.float64)
    n = G.size
    with np.errstate(invalid='ignore', divide='ignore'):
        d = G - V
        L = np.log(G) - np.log(V)
        thresh = np.maximum(G / V, V / G)
        nf = np.float64(n)
        row = np.array([nf,
                        np.sqrt(np.sum(d * d) / nf),
                        np.sum(np.abs(d) / G) / nf,
                        np.sum(d * d / G) / nf,
                        np.sum(np.abs(d)) / nf,
                        np.sqrt(np.sum(L * L) / nf)] + [np.float64(np.count_nonzero(thresh < t)) / nf for t in THRESHOLDS], np.float64)
        near = int(sum(np.count_nonzero(np.abs(thresh - t) <= 1e-12 * t) for t in THRESHOLDS))
    return dict(row=row, valid=valid, err_map=err, near=near)


def split_metrics(pred, gt, scale):
    """({name: float64 [F]}, err_map float32 [F, H, W], near): frame_metrics over [F, H, W]"""
    frames = [frame_metrics(p, g, scale) for p, g in zip(pred, gt)]
    rows = np.stack([f['row'] for f in frames])
    return ({name: rows[:, k] for k, name in enumerate(METRIC_NAMES)}, np.stack([f['err_map'] for f in frames]),
            sum(f['near'] for f in frames))


def sum_rtol(n_valid):
    """rmse, absrel, sqrel, absdiff: sums of non-negative terms, so any order of summation is within (N - 1) u of the exact sum
    on either side; 8 u for the final division, the root and a last-bit difference in a term"""
    return (2.0 * n_valid + 8.0) * U53


def assert_rows_close(got, ref, what=''):
    """got, ref: {name: [F]}.  n_valid and a1 / a2 / a3 equal; the four plain sums within sum_rtol; rmse_log within that plus
    LOG_ATOL (the device's float64 log is held to OpenCL's 3 ulp, numpy's to 1: each L moves by at most 1.2e-14, and a root
    mean square moves by no more than its terms).  A NaN matches only a NaN."""
    n = np.asarray(ref['n_valid'])
    np.testing.assert_array_equal(got['n_valid'], n, err_msg=what)
    for k in ('a1', 'a2', 'a3'):
        np.testing.assert_array_equal(got[k], ref[k], err_msg='%s %s' % (what, k))
    for k in ('rmse', 'absrel', 'sqrel', 'absdiff', 'rmse_log'):
        g, r = np.asarray(got[k], np.float64), np.asarray(ref[k], np.float64)
        nan = np.isnan(r)
        assert np.array_equal(np.isnan(g), nan), '%s %s: NaN in %s, expected in %s' % (what, k, np.isnan(g), nan)
        gate = sum_rtol(n) * np.abs(r) + (LOG_ATOL if k == 'rmse_log' else 0.0)
        err = np.abs(g - r)
        print('%s %s: worst error %.3e of gate %.3e' % (what, k, np.max(err[~nan], initial=0.0), np.min(gate[~nan], initial=np.inf)))
        assert np.all(err[~nan] <= gate[~nan]), '%s %s: error %s exceeds %s' % (what, k, err, gate)


def seeded_frames(shape, scale, seed, n_frames=1):
    """(pred, gt) float32 [F, H, W] in scene units: gt uniform in (0.5, 75) m with about 30 % invalid (zero, negative or beyond
    80 m), predictions around gt with some negative, some below 1e-3 m and some above 80 m"""
    rs = np.random.RandomState(seed)
    full = (n_frames,) + tuple(shape)
    gt = rs.uniform(0.5, 75.0, full)
    kind = rs.rand(*full)
    gt = np.where(kind < 0.1, 0.0, np.where(kind < 0.2, -1.0, np.where(kind < 0.3, rs.uniform(80.5, 120.0, full), gt)))
    pred = gt * rs.uniform(0.4, 2.5, full) + rs.normal(0, 0.5, full)
    kind = rs.rand(*full)
    pred = np.where(kind < 0.05, -rs.uniform(0.1, 5.0, full), np.where(kind < 0.1, rs.uniform(81.0, 200.0, full),
                                                                       np.where(kind < 0.13, 1e-4, pred)))
    s = np.float32(scale)
    return (pred.astype(np.float32) * s).astype(np.float32), (gt.astype(np.float32) * s).astype(np.float32)

"""The colour correction of DESIGN.md 8.3 as numpy float64, written from that text: the yardstick of libcolorcc_hip.so.

It restates upstream's image.color_correct (nerf-methods/mipnerf360/internal/image.py:81-124) with `np.linalg.lstsq(rcond=-1)`
on the full masked [pixels, 10] matrix, as upstream solves it -- NOT through the normal equations the kernels use.  jax is on
none of this project's machines, so no golden file could be made from the imported original; the helper is pinned by upstream's
own property test instead (tests/test_color_correct.py).
"""
import numpy as np

NUM_ITERS = 5
EPS = 0.5 / 255
N_SUMS = 66


def unclipped(z):
    return (z >= EPS) & (z <= 1 - EPS)


def features(x):
    """[P, 10] of x [P, 3]: r*r r*g r*b g*g g*b b*b r g b 1 (upstream's column order)"""
    cols = [x[:, c:c + 1] * x[:, c:] for c in range(3)]
    return np.concatenate(cols + [x, np.ones_like(x[:, :1])], -1)


def prepare(img, ref_u8):
    x0 = np.asarray(img).astype(np.float64).reshape(-1, 3)
    x0 = np.where(np.isfinite(x0), x0, 0.)
    ref = np.asarray(ref_u8).astype(np.float64).reshape(-1, 3) / 255.
    return x0, ref


def color_correct(img, ref_u8, num_iters=NUM_ITERS):
    """(rgb_cc float64 like img, warps [num_iters, 10, 3], mask counts [num_iters, 3]) of a float render and uint8 ground truth"""
    assert np.asarray(ref_u8).dtype == np.uint8 and np.shape(img) == np.shape(ref_u8) and np.shape(img)[-1] == 3
    x0, ref = prepare(img, ref_u8)
    mask0 = unclipped(x0)
    x = x0
    warps, counts = [], []
    for _ in range(num_iters):
        a = features(x)
        w = np.zeros((10, 3))
        n = np.zeros(3)
        for c in range(3):
            mask = mask0[:, c] & unclipped(x[:, c]) & unclipped(ref[:, c])
            n[c] = mask.sum()
            w[:, c] = np.linalg.lstsq(np.where(mask[:, None], a, 0.), np.where(mask, ref[:, c], 0.), rcond=-1)[0]
        assert np.isfinite(w).all()
        warps.append(w)
        counts.append(n)
        x = np.clip(a @ w, 0., 1.)
    return x.reshape(np.shape(img)), np.stack(warps), np.stack(counts)


def normal_equations(img, ref_u8):
    """[3, 66] masked sums of iteration 0 in the layout of COLORCC_SUMS, and the sums of absolute products (same layout)"""
    x0, ref = prepare(img, ref_u8)
    a = features(x0)
    iu = np.triu_indices(10)
    out, mag = np.zeros((3, N_SUMS)), np.zeros((3, N_SUMS))
    for c in range(3):
        mask = unclipped(x0[:, c]) & unclipped(ref[:, c])
        am, b = a[mask], ref[mask, c]
        out[c, :55] = (am.T @ am)[iu]
        out[c, 55:65] = am.T @ b
        out[c, 65] = mask.sum()
        mag[c, :55] = (np.abs(am).T @ np.abs(am))[iu]
        mag[c, 55:65] = np.abs(am).T @ np.abs(b)
        mag[c, 65] = mask.sum()
    return out, mag


def to_u8(x):
    """the PNG's bytes: clip, x 255, truncate (utils.save_img_u8)"""
    return (np.clip(np.nan_to_num(x), 0., 1.) * 255.).astype(np.uint8)


def psnr_cc(rgb_cc, ref_u8, quantize=True):
    q = np.round(rgb_cc * 255) / 255 if quantize else rgb_cc
    mse = ((q - np.asarray(ref_u8).astype(np.float64) / 255.) ** 2).mean()
    with np.errstate(divide='ignore'):                    # an exact fit: +inf
        return float(-10. / np.log(10.) * np.log(mse))


def byte_rule(dev_u8, rgb_cc):
    """(number of differing bytes, number of them the rule does not excuse, number of helper values the rule covers): a byte may
    differ from the helper's only where the helper's value v has 0 < v < 1 and |255 v - rint(255 v)| < 1e-6, and then by 1."""
    want = to_u8(rgb_cc)
    near = (rgb_cc > 0) & (rgb_cc < 1) & (np.abs(255 * rgb_cc - np.rint(255 * rgb_cc)) < 1e-6)
    diff = np.asarray(dev_u8).astype(np.int64) - want.astype(np.int64)
    bad = (diff != 0) & ~(near & (np.abs(diff) == 1))
    return int((diff != 0).sum()), int(bad.sum()), int(near.sum())


# ------------------------------------------------------------------------------------------------ test frames
def natural_frame(H, W, seed):
    """A smooth, natural-looking float64 image in about [0.05, 0.95] with correlated channels and texture"""
    rs = np.random.RandomState(seed)
    yy, xx = np.mgrid[0:H, 0:W]
    yy, xx = yy / max(H - 1, 1), xx / max(W - 1, 1)
    base = 0.5 + 0.25 * np.sin(3.1 * xx + 1.3 * rs.rand()) * np.cos(2.3 * yy + rs.rand())
    chans = []
    for c in range(3):
        tint = 0.18 * np.sin((2 + c) * xx * 2.2 + rs.rand() * 6) * np.sin((1.5 + c) * yy * 2.9 + rs.rand() * 6)
        chans.append(base + tint + 0.06 * rs.randn(H, W))
    return np.clip(np.stack(chans, -1), 0.05, 0.95)


def gained_pair(H, W, seed, noise=0.0, saturate=0.0, quantise_img=False):
    """(img float32, ref_u8): ref a natural frame, img = clip(ref * gain + offset [+ noise]) with per-channel gains in
    [0.6, 1.4].  saturate > 0 scales both so that about that share of values clips at 1 (in img and in ref)."""
    rs = np.random.RandomState(seed + 1000)
    gt = natural_frame(H, W, seed)
    if saturate > 0:
        gt = np.clip((gt - 0.05) * (1.0 / np.quantile(gt - 0.05, 1 - saturate)), 0, 1)
    gain, off = rs.uniform(0.6, 1.4, 3), rs.uniform(-0.03, 0.03, 3)
    img = gt * gain + off + noise * rs.randn(H, W, 3)
    if saturate > 0:
        img = img * (1.0 / np.quantile(img, 1 - saturate))
    img = np.clip(img, 0, 1)
    if quantise_img:
        img = np.rint(img * 255) / 255
    return img.astype(np.float32), np.rint(gt * 255).astype(np.uint8)


def nonfinite_pair(H, W, seed):
    """a gained pair whose render holds NaN, +inf and -inf pixels (they count as 0: DESIGN 8.3)"""
    img, ref = gained_pair(H, W, seed)
    rs = np.random.RandomState(seed + 2000)
    idx = rs.randint(0, H * W * 3, 300)
    flat = img.reshape(-1)
    flat[idx[:100]], flat[idx[100:200]], flat[idx[200:]] = np.nan, np.inf, -np.inf
    return img, ref


def well_conditioned_cases():
    """[(label, img float32 [H, W, 3], ref_u8)]: the list the rgb_cc gate of DESIGN 8.3 is measured and held on"""
    return [('natural', *gained_pair(375, 1242, 0)),
            ('natural+noise', *gained_pair(375, 1242, 1, noise=0.02)),
            ('quantised', *gained_pair(375, 1242, 2, quantise_img=True)),
            ('saturated', *gained_pair(375, 1242, 3, noise=0.01, saturate=0.05)),
            ('ragged 375x1241', *gained_pair(375, 1241, 4)),
            ('1x1', *gained_pair(1, 1, 5)),
            ('7x7', *gained_pair(7, 7, 6)),
            ('37x53', *gained_pair(37, 53, 7)),
            ('nonfinite', *nonfinite_pair(375, 1242, 8))]


def degenerate_cases(H=64, W=96):
    """[(label, img, ref_u8)]: rank-deficient systems, where lstsq(rcond=-1) itself is ill-defined -- only
    finiteness, range and reproducibility can be asked.  The last one, all saturated, is exactly black."""
    _, ref = gained_pair(H, W, 20)
    base = natural_frame(H, W, 21).astype(np.float32)
    grey = np.repeat(base[..., :1], 3, -1)
    two = base.copy()
    two[..., 1] = two[..., 0]
    return [('grey', grey, ref), ('constant', np.full((H, W, 3), 0.4, np.float32), ref), ('two equal channels', two, ref),
            ('all saturated', np.ones((H, W, 3), np.float32), ref)]

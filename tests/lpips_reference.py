"""LPIPS v0.1 (net='vgg', lpips=True, spatial=False, evaluation mode) restated as executable code on torch CPU: what
liblpips_hip.so is held to.  Written from knowledge of the `lpips` and `torchvision` packages, neither of
which is installed where this project is built or tested, so it has NOT been compared with them.

    x = byte / 255 * 2 - 1;  x = (x - shift) / scale
    VGG-16 features: 3 x 3 convolutions, stride 1, zero padding 1, bias, ReLU; 2 x 2 max-pool stride 2 (floor);
      a tap after the ReLU of convolutions 1, 3, 6, 9, 12 (0-based)
    per tap: n = f / (sqrt(sum_c f^2) + 1e-10);  d_l = mean_pixels sum_c w_l[c] * (n0[c] - n1[c])^2
    LPIPS = d_0 + ... + d_4

`lpips(gt, pred, weights, dtype)` runs it in float64 (the yardstick) or float32 (what utils/eval.py of the reference
delivers).  `random_weights(seed)` makes the seeded test weights: He-scaled convolutions, small biases, non-negative lin
weights as the real ones are; no weight file is committed.
"""
import numpy as np
import torch
import torch.nn.functional as F

CONV_INDEX = (0, 2, 5, 7, 10, 12, 14, 17, 19, 21, 24, 26, 28)
CONV_SHAPES = ((3, 64), (64, 64), (64, 128), (128, 128), (128, 256), (256, 256), (256, 256), (256, 512), (512, 512),
               (512, 512), (512, 512), (512, 512), (512, 512))
TAP_AFTER = (1, 3, 6, 9, 12)
TAP_CHANNELS = (64, 128, 256, 512, 512)
SHIFT = (-.030, -.088, -.188)
SCALE = (.458, .448, .450)
EPS = 1e-10


def random_weights(seed, lin_scale=1.0):
    """{state-dict key: float32 numpy array}: He-scaled convolutions, biases ~ 0.05 N(0, 1), lin weights lin_scale * U[0, 1)"""
    rs = np.random.RandomState(seed)
    w = {}
    for idx, (cin, cout) in zip(CONV_INDEX, CONV_SHAPES):
        w['features.%d.weight' % idx] = (rs.standard_normal((cout, cin, 3, 3)) * np.sqrt(2.0 / (9 * cin))).astype(np.float32)
        w['features.%d.bias' % idx] = (0.05 * rs.standard_normal(cout)).astype(np.float32)
    for l, c in enumerate(TAP_CHANNELS):
        w['lin%d.model.1.weight' % l] = (lin_scale * rs.rand(1, c, 1, 1)).astype(np.float32)
    return w


def scale_input(u8, dtype):
    """uint8 [N, H, W, 3] -> [N, 3, H, W] of dtype: byte / 255 * 2 - 1, then the scaling layer"""
    x = torch.from_numpy(np.ascontiguousarray(u8)).to(dtype) / 255 * 2 - 1
    shift, scale = torch.tensor(SHIFT, dtype=dtype), torch.tensor(SCALE, dtype=dtype)
    return ((x - shift) / scale).permute(0, 3, 1, 2).contiguous()


def features(x, weights, dtype):
    """the five tapped maps [N, C_l, H_l, W_l] of x [N, 3, H, W]"""
    taps = []
    for i, idx in enumerate(CONV_INDEX):
        wt = torch.from_numpy(weights['features.%d.weight' % idx]).to(dtype)
        b = torch.from_numpy(weights['features.%d.bias' % idx]).to(dtype)
        x = F.relu(F.conv2d(x, wt, b, stride=1, padding=1))
        if i in TAP_AFTER:
            taps.append(x)
            if len(taps) < 5:
                x = F.max_pool2d(x, kernel_size=2, stride=2)
    return taps


def tap_distance(f0, f1, w):
    """[N]: mean over pixels of sum_c w[c] * (n0 - n1)^2 with n = f / (sqrt(sum_c f^2) + 1e-10); f [N, C, H, W], w [C]"""
    n0 = f0 / (torch.sqrt(torch.sum(f0 * f0, dim=1, keepdim=True)) + EPS)
    n1 = f1 / (torch.sqrt(torch.sum(f1 * f1, dim=1, keepdim=True)) + EPS)
    d = (n0 - n1) ** 2
    return (d * w.view(1, -1, 1, 1)).sum(dim=1).mean(dim=(1, 2))


def lpips(gt_u8, pred_u8, weights, dtype=torch.float64):
    """(total [N], per_tap [N, 5]) float64 numpy arrays of uint8 [N, H, W, 3] (or [H, W, 3]) image pairs"""
    gt_u8, pred_u8 = np.asarray(gt_u8), np.asarray(pred_u8)
    if gt_u8.ndim == 3:
        gt_u8, pred_u8 = gt_u8[None], pred_u8[None]
    assert gt_u8.dtype == np.uint8 and pred_u8.dtype == np.uint8 and gt_u8.shape == pred_u8.shape and gt_u8.shape[-1] == 3
    assert gt_u8.shape[1] >= 16 and gt_u8.shape[2] >= 16, 'H, W >= 16'
    per = []
    with torch.no_grad():
        for g, p in zip(gt_u8, pred_u8):                      # one pair at a time: bounded memory at 375 x 1242
            t0 = features(scale_input(g[None], dtype), weights, dtype)
            t1 = features(scale_input(p[None], dtype), weights, dtype)
            per.append([float(tap_distance(a, b, torch.from_numpy(weights['lin%d.model.1.weight' % l]).to(dtype).reshape(-1))[0])
                        for l, (a, b) in enumerate(zip(t0, t1))])
    per = np.asarray(per, np.float64)
    return per.sum(axis=1), per


def conv3x3_relu_nhwc(x_nhwc, w, b, dtype=torch.float64):
    """one layer on an NHWC numpy array -> NHWC numpy array of dtype (for the single-layer GPU tests)"""
    with torch.no_grad():
        x = torch.from_numpy(np.ascontiguousarray(x_nhwc)).to(dtype).permute(0, 3, 1, 2)
        y = F.relu(F.conv2d(x, torch.from_numpy(w).to(dtype), torch.from_numpy(b).to(dtype), stride=1, padding=1))
    return y.permute(0, 2, 3, 1).contiguous().numpy()


# ---- the image pairs the tests gate (tests/test_lpips.py checks their range on the CPU, tests/test_gpu_lpips.py the kernel)
CONTENTS = ('noise', 'smooth', 'flat', 'saturated')
PRED_KINDS = ('same', 'noise2', 'noise25', 'unrelated')
LIN_SCALE = 1.0           # scale of the random lin weights: puts the float64 totals of the pairs in RANGED_KINDS into RANGE
RANGE = (0.05, 1.5)       # the paper's LPIPS column is 0.5 - 0.6
# the pairs whose total must lie in RANGE (tests/test_lpips.py).  The others are below it whatever the scale: pred = gt is 0 by
# definition, sigma-2 noise gives 1e-4 .. 2e-2 and sigma-25 noise on the saturated image 2e-2, four decades under 'unrelated'.
RANGED = tuple((c, k) for c in CONTENTS for k in ('noise25', 'unrelated') if (c, k) != ('saturated', 'noise25'))
WEIGHT_SEED = 20260


def content(name, H, W, rs):
    if name == 'noise':
        return rs.randint(0, 256, (H, W, 3)).astype(np.uint8)
    if name == 'smooth':
        yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
        ch = [127.5 + 127.5 * np.sin(xx / (17.0 + 5 * c) + c) * np.cos(yy / (23.0 - 4 * c)) for c in range(3)]
        return np.clip(np.stack(ch, -1), 0, 255).astype(np.uint8)
    if name == 'flat':
        return np.full((H, W, 3), 93, np.uint8)
    if name == 'saturated':
        return (255 * (rs.rand(H, W, 3) < 0.5)).astype(np.uint8)
    raise KeyError(name)


def make_pair(cname, kind, H, W, seed):
    """(gt, pred) uint8 [H, W, 3]: pred = gt, gt + N(0, 2), gt + N(0, 25) (rounded, clipped) or an unrelated noise image"""
    rs = np.random.RandomState(seed)
    gt = content(cname, H, W, rs)
    if kind == 'same':
        return gt, gt.copy()
    if kind == 'unrelated':
        return gt, content('noise', H, W, rs)
    sigma = {'noise2': 2.0, 'noise25': 25.0}[kind]
    return gt, np.clip(np.rint(gt + rs.normal(0, sigma, gt.shape)), 0, 255).astype(np.uint8)


def gated_pairs(H, W, full=True):
    """[(label, gt, pred)]: every content x every pred kind (full), or each content with one pred kind in rotation"""
    out = []
    for i, c in enumerate(CONTENTS):
        for j, k in enumerate(PRED_KINDS):
            if full or j == (i + 1) % 4:
                out.append(('%s/%s/%dx%d' % (c, k, H, W), ) + make_pair(c, k, H, W, 1000 * i + 10 * j + H + W))
    return out

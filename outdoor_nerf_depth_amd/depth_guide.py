"""Depth-guided fine sampling of the NeRF++ path, on the device.  ctypes binding of libdepthguide_hip.so (include/depthguide_hip.h).

Level m > 0 of the cascade draws its new depths from the previous level's weights (`sample_pdf`).  Early in training, and on small
sample budgets, that histogram is almost flat, while a depth prior with a standard deviation already says where the surface is.
`depth_guide` takes G of the level's new foreground depths from a Gaussian around the prior, truncated at three standard deviations
(Roessle et al., Dense Depth Priors for NeRF); a ray without a prior, and every ray of a render, takes them around the depth and
spread the previous level rendered.  Per ray, with the previous level's depths zp and weights wp, the S_in depths zin the existing
fine sampling produced, the ray's bounds lo and hi, the prior p with standard deviation s, and uniforms v [G]:

    s_eff  = max(s, min_std)
    mode 0   p > 0 and p < hi and 0 < s_eff < inf (kl's and gnll's mask):   mu = p, sd = s_eff
    mode 1   else, W = sum wp > 1e-10:   mu = sum(wp zp) / W,  sd = max(sqrt(sum(wp (zp - mu)^2) / W), min_std)
    mode 2   else: the G depths are stratified over [lo, hi]
    q_j = (j + v_j) / G;   g_j = clamp(mu + sd * T(q_j), lo, hi)   (mode 2: lo + (hi - lo) q_j);   out = sort(cat(zin, float32(g)))

T is the inverse CDF of the standard normal truncated at +-3, read from a table of 1025 entries by linear interpolation
(`table()`, built here with statistics.NormalDist and uploaded once per device).  The quantiles are stratified, so the number of
depths per sigma band is fixed to within the two boundary strata whatever the uniforms are.  The definition is DESIGN.md 9.12
(restated as code in tests/depth_guide_reference.py).  Sample positions carry no gradient anywhere in this path.

One level per call, enqueued on torch's current stream; nothing synchronises.  torch only allocates.  There is no host path: without
libdepthguide_hip.so and a device `depth_guide` raises.  The trainer and the CLIs import this module only when
depth_guide_samples > 0: with 0 nothing of it is imported, loaded or launched, and a step and a render make exactly the calls they
made without it.
"""
import ctypes as C
import math
import os

from . import _ctypes_util as U

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get('DEPTHGUIDE_HIP_LIB') or os.path.join(_HERE, 'libdepthguide_hip.so')
OK = 0
ABI_VERSION = 1
MAX_RAYS = 1 << 20
MAX_PREV = 1024
MAX_MERGED = 512
TABLE_K = 1024
TRUNCATE = 3.0                      # the Gaussian ends at +- this many standard deviations
RNG_STREAM = 5

_fp = C.c_void_p
# every symbol include/depthguide_hip.h declares: name -> (restype, argtypes)
SYMBOLS = {
    'depthguide_last_error': (C.c_char_p, []),
    'depthguide_abi_version': (C.c_int, []),
    'depthguide_merge': (C.c_int, [_fp, C.c_int, C.c_int, C.c_int, C.c_int, _fp, _fp, _fp, _fp, _fp, _fp, _fp, C.c_double, C.c_double,
                                   _fp, _fp, C.c_int, C.c_uint64, C.c_uint64, _fp, _fp, _fp]),
}

_lib = None


class DepthGuideError(RuntimeError):
    pass


def lib():
    """The loaded library with typed prototypes.  Raises if it has not been built."""
    global _lib
    if _lib is None:
        _lib = U.load(LIB_PATH, 'libdepthguide_hip.so', SYMBOLS, 'depthguide_abi_version', ABI_VERSION, DepthGuideError,
                      ' (hipcc --offload-arch=gfx950). There is no CPU fallback for the depth-guided sampling.')
    return _lib


def last_error():
    return lib().depthguide_last_error().decode('utf-8', 'replace')


check = U.checker(lib, 'depthguide_last_error', DepthGuideError, 'depthguide call')


# ------------------------------------------------------------------------------------------------ configuration (no device, no library)
def check_samples(n_guide, n_new):
    """depth_guide_samples = n_guide against the level's n_new new foreground samples: 0 <= n_guide < n_new, or ValueError.
    Returns n_guide as an int."""
    if isinstance(n_guide, bool) or int(n_guide) != n_guide:
        raise ValueError('depth_guide_samples = %r: expected an integer' % (n_guide,))
    n_guide = int(n_guide)
    if n_guide < 0 or (n_guide > 0 and n_guide >= int(n_new)):
        raise ValueError('depth_guide_samples = %d: expected 0 (off) .. %d, fewer than the %d new samples of a level (the others '
                         'are still drawn from the previous level\'s weights)' % (n_guide, max(int(n_new) - 1, 0), int(n_new)))
    return n_guide


def check_std(std, have_map, name='depth_guide_std'):
    """The constant standard deviation of the prior: with have_map (every batch carries depth_std) it is not read and None or
    anything not negative passes; without one it must be positive and finite, or ValueError.  Returns it as a float, or None."""
    if std is None:
        if not have_map:
            raise ValueError('%s: the prior has no standard-deviation map, so a positive constant (metres) is needed' % name)
        return None
    std = float(std)
    if not math.isfinite(std) or std < 0 or (not have_map and std <= 0):
        raise ValueError('%s = %r: expected a finite positive value in metres%s'
                         % (name, std, '' if have_map else ' (the prior has no standard-deviation map)'))
    return std


def check_min_std(min_std):
    min_std = float(min_std)
    if not math.isfinite(min_std) or min_std < 0:
        raise ValueError('depth_guide_min_std = %r: expected a finite value that is not negative' % (min_std,))
    return min_std


# ------------------------------------------------------------------------------------------------ the table
def table(K=TABLE_K, truncate=TRUNCATE):
    """T[i] = Phi^-1(Phi(-t) + (Phi(t) - Phi(-t)) i / K), i = 0 .. K: float64 numpy [K + 1], T[0] = -t and T[K] = t exactly."""
    import numpy as np
    from statistics import NormalDist
    nd = NormalDist()
    a, b = nd.cdf(-truncate), nd.cdf(truncate)
    T = np.array([nd.inv_cdf(a + (b - a) * i / K) for i in range(K + 1)], np.float64)
    T[0], T[K] = -truncate, truncate
    return T


_tables = {}                        # device index -> the table on that device, uploaded at the first call


def device_table(device):
    t = _tables.get(device.index)
    if t is None:
        import torch
        t = _tables[device.index] = torch.from_numpy(table()).to(device)
    return t


# ------------------------------------------------------------------------------------------------ the call
def _tensor(t, name, shape, dev):
    return U.inplace_f32(t, name, shape, dev, DepthGuideError, 'depth-guided sampling', 'z_prev')


def depth_guide(z_prev, w_prev, z_in, lo, hi, n_guide, prior=None, prior_std=None, std_const=0.0, min_std=0.0, v=None, rng=None,
                return_guide=False):
    """n_guide guided depths per ray merged into z_in.  z_prev, w_prev [n, S_prev]: the previous level's foreground depths and
    weights; z_in [n, S_in]: the output of the existing fine sampling (ascending); lo, hi [n]: the rays' bounds; prior [n] or None
    (no ray has one); prior_std [n] or None (every ray has std_const): contiguous float32 device tensors, n in 1 .. 2^20, S_prev in
    1 .. 1024, S_in + n_guide <= 512.  std_const, min_std: in the units of the depths.  The uniforms: rng = (seed, step) draws them
    in the kernel (Philox stream 5, element ray * n_guide + j); else v [n, n_guide]; else 0.5 (deterministic).
    Returns (z_merged [n, S_in + n_guide] float32, mode [n] int32) and, with return_guide, guide [n, n_guide] (float32(g), in the
    order of j).  Enqueue only."""
    import torch
    if not isinstance(z_prev, torch.Tensor) or z_prev.dim() != 2:
        raise DepthGuideError('z_prev: expected a float32 device tensor [n, S_prev], got %s' % (tuple(getattr(z_prev, 'shape', ())),))
    n, S_prev = int(z_prev.shape[0]), int(z_prev.shape[1])
    if not 1 <= n <= MAX_RAYS:
        raise DepthGuideError('z_prev: %d rays, expected 1 .. 2^20' % n)
    if not 1 <= S_prev <= MAX_PREV:
        raise DepthGuideError('z_prev: %d samples per ray, expected 1 .. %d' % (S_prev, MAX_PREV))
    if not isinstance(z_in, torch.Tensor) or z_in.dim() != 2:
        raise DepthGuideError('z_in: expected a float32 device tensor [n, S_in], got %s' % (tuple(getattr(z_in, 'shape', ())),))
    S_in, G = int(z_in.shape[1]), int(n_guide)
    if S_in < 1 or G < 1 or S_in + G > MAX_MERGED:
        raise DepthGuideError('z_in: %d samples per ray and %d guided ones, expected at least 1 each and at most %d together'
                              % (S_in, G, MAX_MERGED))
    dev = z_prev.device if z_prev.is_cuda else None
    _tensor(z_prev, 'z_prev', (n, S_prev), dev)
    _tensor(w_prev, 'w_prev', (n, S_prev), dev)
    _tensor(z_in, 'z_in', (n, S_in), dev)
    _tensor(lo, 'lo', (n,), dev)
    _tensor(hi, 'hi', (n,), dev)
    if prior is not None:
        _tensor(prior, 'prior', (n,), dev)
    if prior_std is not None:
        _tensor(prior_std, 'prior_std', (n,), dev)
    if v is not None:
        if rng is not None:
            raise DepthGuideError('v and rng: the uniforms are either given or drawn in the kernel')
        _tensor(v, 'v', (n, G), dev)
    min_std = float(min_std)
    if not math.isfinite(min_std) or min_std < 0.0:
        raise DepthGuideError('min_std = %r: expected a finite value that is not negative' % min_std)
    with torch.cuda.device(dev):
        z_merged = torch.empty(n, S_in + G, device=dev)
        mode = torch.empty(n, dtype=torch.int32, device=dev)
        guide = torch.empty(n, G, device=dev) if return_guide else None
        seed, step = (int(rng[0]), int(rng[1])) if rng is not None else (0, 0)
        check(lib().depthguide_merge(U.stream(), n, S_prev, S_in, G, U.p(z_prev), U.p(w_prev), U.p(z_in), U.p(lo), U.p(hi), U.p(prior),
                                     U.p(prior_std), float(std_const), min_std, U.p(device_table(dev)), U.p(v), int(rng is not None),
                                     seed & (2 ** 64 - 1), step & (2 ** 64 - 1), U.p(z_merged), U.p(mode), U.p(guide)), 'depthguide_merge')
    return (z_merged, mode, guide) if return_guide else (z_merged, mode)


def fine_level(fg_z, fg_weights, bg_z, bg_weights, n_new, n_guide, lo, hi, prior=None, prior_std=None, std_const=0.0, min_std=0.0,
               u_fg=None, u_bg=None, v_fg=None, rng=None, det=False):
    """The depths of a level m > 0 with n_guide of its n_new new foreground depths guided: the foreground is fine-sampled with
    n_new - n_guide depths and the background with n_new through the existing single-volume ops.sample_fine, then the one
    depth_guide call.  The uniforms: det: none (the deterministic forms of both); rng = (seed, step): the in-kernel generator's --
    streams 2 and 3 through ops.rng_uniform for the two fine calls, stream 5 inside depth_guide; else u_fg [n, n_new - n_guide],
    u_bg [n, n_new], v_fg [n, n_guide], each drawn with torch.rand, in that order, where it is None.
    Returns (fg_z [n, S_old + n_new], bg_z [n, S_old + n_new], mode [n])."""
    import torch
    from . import ops
    n, dev = fg_z.shape[0], fg_z.device
    if det:
        u_fg = u_bg = v_fg = rng = None
    elif rng is not None:
        u_fg = ops.rng_uniform(rng[0], rng[1], 2, (n, n_new - n_guide), dev)
        u_bg = ops.rng_uniform(rng[0], rng[1], 3, (n, n_new), dev)
        v_fg = None
    else:
        u_fg = torch.rand(n, n_new - n_guide, device=dev) if u_fg is None else u_fg
        u_bg = torch.rand(n, n_new, device=dev) if u_bg is None else u_bg
        v_fg = torch.rand(n, n_guide, device=dev) if v_fg is None else v_fg
    z_in = ops.sample_fine(fg_z, fg_weights, n_new - n_guide, det=det, u=u_fg)
    bg_new = ops.sample_fine(bg_z, bg_weights, n_new, det=det, u=u_bg)
    fg_new, mode = depth_guide(fg_z.contiguous().float(), fg_weights.contiguous().float(), z_in, lo, hi, n_guide, prior=prior,
                               prior_std=prior_std, std_const=std_const, min_std=min_std, v=v_fg, rng=rng)
    return fg_new, bg_new, mode

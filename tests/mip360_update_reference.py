"""Float64 restatements and per-element error bounds for the parameter-update side of the MipNeRF-360 trainer
(csrc/mip360_train.hip: slab_sum_kernel, slab_sum2_kernel, col_sum_kernel, grad_weight_col_kernel, head_backward_kernel,
sumsq_partial_kernel, clip_mult_kernel, adam_kernel, pack_weight_kernel), for tests/test_mip360_update_reference.py (CPU) and
tests/test_gpu_mip360_update.py (GPU).  Plain numpy; nothing here touches the code under test.

Every bound is absolute and is built from sums of magnitudes of the inputs: a relative bound on a quantity that can cancel (mu,
1 - exp(-d), s (1 - s), a sum of slabs of both signs) holds for no correct float32 implementation.  U = 2^-24 is the unit roundoff
of float32; gamma(k) = (1 + U)^k - 1 is what k roundings in a row can do to a product or to a sum of same-signed terms.  A fused
multiply-add drops one rounding of the count, so every bound admits a compiler that contracts a * b + c (the file is built without
-ffp-contract=off); division and square root are correctly rounded (-fhip-fp32-correctly-rounded-divide-sqrt).

The Adam functions take `xp` (numpy by default): they use operators and the seven functions where / sqrt / abs / isnan / frexp /
ldexp / ones_like only, so that a caller can hand in float64 torch tensors and keep a 13 M element chain on the device.

Known distance of adam_kernel from optax / oracle.mip360_oracle.apply_gradients (documented, not a rounding error):
  the kernel receives b2 as a float, b2_f = 0.999000012874603 (0.999 (1 + 1.289e-8)), and forms 1.f - b2 in float32, which is exact
  (Sterbenz: 1/2 <= b2 <= 2): 1 - b2_f = 0.000999987125397 = 0.001 (1 - 1.2875e-5).  The second moment of one step is therefore
  1.2875e-5 below optax's in relative terms, sqrt(v_hat) 6.44e-6 below, and the update lr m_hat / (sqrt(v_hat) + eps) larger by
  6.44e-6 sqrt(v_hat) / (sqrt(v_hat) + eps).  Likewise b1_f = 0.899999976158142, 1 - b1_f = 0.1 (1 + 2.384e-7): m_hat of step 1 is
  2.4e-7 larger (bc1 = (float)(1 - 0.9) carries 1.5e-8).  Together 6.7e-6 of the update at step 1 where sqrt(v_hat) >> eps, and less
  with more steps (the weights b2^k (1 - b2) of nu sum to 1 - b2^t whatever b2 is; the bias correction divides by the double value).
  adam_constants(..., exact=True) are optax's constants, exact=False the kernel's; constant_distance() turns the difference into the
  relative perturbations adam_bounds() carries, and ADAM_STEP1_DISTANCE is the figure above, asserted by the CPU test."""
import numpy as np

U = 2.0 ** -24                      # unit roundoff of float32
TINY = 2.0 ** -126                  # smallest normal float32 (and bfloat16): what a flushed result can lose
DENORM = 2.0 ** -149                # smallest float32
FMAX = float(np.finfo(np.float32).max)
NORM_EPS = 2.0 ** -23               # clip_gradients' eps (np.finfo(float32).eps)
BF16_HALF_ULP = 2.0 ** -8           # round-to-nearest bfloat16 (8 significand bits) relative to the binade's base
ADAM_STEP1_DISTANCE = 6.7e-6        # see the module docstring


def f64(a):
    return np.asarray(a, np.float64)


def f32r(x):
    """a Python float as the kernel receives it: rounded to float32, held in a double"""
    return float(np.float32(x))


def gamma(k):
    return (1.0 + U) ** k - 1.0


def round_bf16(x):
    """float32 -> nearest bfloat16, ties to even, as float32 (the bits `(__bf16)x` gives)"""
    u = np.ascontiguousarray(x, np.float32).view(np.uint32)
    r = ((u >> np.uint32(16)) & np.uint32(1)) + np.uint32(0x7FFF)
    return ((u + r) & np.uint32(0xFFFF0000)).view(np.float32)


def ratio(got, want, bound):
    """|got - want| / bound per element; an element that is not finite where the reference is, or off where the bound is 0,
    counts as inf (a NaN must not pass a comparison by being unordered)."""
    got, want, bound = f64(got), f64(want), f64(bound) + np.zeros_like(f64(want))
    err = np.abs(got - want)
    with np.errstate(divide='ignore', invalid='ignore'):
        r = np.where(err == 0, 0.0, err / bound)
    return np.where(np.isfinite(got) | ~np.isfinite(want), np.nan_to_num(r, nan=np.inf), np.inf)


# ------------------------------------------------------------------------------------------------------------ norm and clip
def norm_reference(tensors):
    """oracle.mip360_oracle.tree_norm over a list of arrays: sqrt of the float64 sum of squares"""
    return float(np.sqrt(sum(float(np.sum(np.square(f64(t)))) for t in tensors)))


def norm_bound(norm, n_partial):
    """sumsq_partial_kernel + clip_mult_kernel: squares and sums in double (exact next to U), then
      1 rounding: every block's partial cast to float (same-signed terms: U of the sum of squares, so U / 2 of the norm), and a
        partial below 2^-126 may be flushed: n_partial 2^-126 of the sum, at most its square root of the norm;
      1 rounding: norm = (float)sqrt(double).                                                   gamma(2) norm + sqrt(n_partial 2^-126)"""
    return gamma(2) * norm + np.sqrt(n_partial * TINY)


def clip_reference(norm, max_norm):
    """the clip lines of oracle.mip360_oracle.apply_gradients with max_norm as the float the kernel receives"""
    mx = f32r(max_norm)
    if not mx > 0:
        return 1.0
    with np.errstate(invalid='ignore'):
        r = mx / (NORM_EPS + norm)
    return r if np.isnan(r) else min(1.0, r)


def clip_bound(norm, max_norm, n_partial):
    """ratio = max_norm / (eps + norm): the norm's own error against eps + norm, 1 rounding of the sum, 1 of the division; min(1, .)
    is 1-Lipschitz, so the bound of the ratio is a bound of the multiplier.  max_norm <= 0: exactly 1."""
    mx = f32r(max_norm)
    if not mx > 0:
        return 0.0
    r = mx / (NORM_EPS + norm)
    return r * (gamma(2) + norm_bound(norm, n_partial) / (NORM_EPS + norm))


# ------------------------------------------------------------------------------------------------------------ Adam
def adam_constants(step, lr, b1=0.9, b2=0.999, eps=1e-6, exact=False):
    """exact=False: what mip360_adam_step hands adam_kernel -- (float)lr, (float)b1, (float)b2, (float)eps, (float)(1 - b^step) with the
    power in double -- and the kernel's 1.f - b, which float32 forms exactly.  exact=True: optax's / the oracle's double constants."""
    bc1, bc2 = 1.0 - b1 ** step, 1.0 - b2 ** step
    if exact:
        return dict(lr=float(lr), b1=b1, omb1=1 - b1, b2=b2, omb2=1 - b2, eps=eps, bc1=bc1, bc2=bc2)
    return dict(lr=f32r(lr), b1=f32r(b1), omb1=1.0 - f32r(b1), b2=f32r(b2), omb2=1.0 - f32r(b2), eps=f32r(eps), bc1=f32r(bc1),
                bc2=f32r(bc2))


def _clean_gradient(g, mult, xp):
    """gi = g * mult, THEN nan_to_num (train_utils.py:345 after the clipping): NaN -> 0, +-inf -> +-FLT_MAX"""
    with np.errstate(invalid='ignore'):
        gi = g if mult is None else g * mult
    gi = xp.where(xp.isnan(gi), 0.0 * xp.ones_like(g), gi)
    gi = xp.where(gi > FMAX, FMAX * xp.ones_like(g), gi)
    return xp.where(gi < -FMAX, -FMAX * xp.ones_like(g), gi)


def adam_reference(p, g, m, v, mult, c, xp=np):
    """adam_kernel line by line on float64 arrays with the constants `c` of adam_constants.  mult: the clip multiplier (a float, NaN
    included) or None for 1.  Returns (p, mu, nu).  With exact constants and a finite or zero / NaN multiplier this is
    oracle.mip360_oracle.apply_gradients' inner loop.  (A +-inf gradient under a finite non-zero multiplier is clamped to FLT_MAX, whose
    square overflows float32 and not float64: no caller gets there, an infinite gradient makes the norm infinite and the multiplier 0.)"""
    gi = _clean_gradient(g, mult, xp)
    mi = c['b1'] * m + c['omb1'] * gi
    vi = c['b2'] * v + c['omb2'] * gi * gi
    return p - c['lr'] * (mi / c['bc1']) / (xp.sqrt(vi / c['bc2']) + c['eps']), mi, vi


def ulp32(a, xp=np):
    """spacing of float32 at |a| (2^-149 below the normal range)"""
    a = xp.abs(a)
    _, e = xp.frexp(a)                                         # a = f 2^e, 1/2 <= f < 1: the binade's base is 2^(e-1)
    return xp.where(a < TINY, DENORM * xp.ones_like(a), xp.ldexp(xp.ones_like(a), e - 24))


def constant_distance(c, c_other):
    """The relative perturbations by which the constants `c_other` differ from `c`, in the three places adam_bounds carries them:
    rel_m on A_m = b1 |m| + (1 - b1) |g| and on m_hat's divisor, rel_v on nu and v_hat's divisor, rel_u on lr and eps."""
    d = lambda k: abs(c[k] - c_other[k]) / abs(c[k])
    return dict(rel_m=max(d('b1'), d('omb1')) + d('bc1'), rel_v=max(d('b2'), d('omb2')) + d('bc2'), rel_u=d('lr') + d('eps'))


def adam_bounds(p, g, m, v, mult, c, xp=np, rel_m=0.0, rel_v=0.0, rel_u=0.0, m_err=0.0, v_rel=0.0, p_err=0.0):
    """How far a float32 adam_kernel may be from adam_reference on the same float32 inputs and constants.  Per element:
      gi = g * mult: 1 rounding (none without a multiplier; counted anyway).
      mu = b1 m + (1 - b1) gi: gi's rounding, 2 products, 1 sum -- 4 roundings, each at most U of A_m = b1 |m| + (1 - b1) |gi|, the sum
        of the magnitudes (the two terms cancel when m and g have opposite signs):                       d_mu <= gamma(4) A_m
      nu = b2 v + ((1 - b2) gi) gi: same-signed terms; gi's rounding twice, 2 products, 1 sum on the second term, 1 product and the
        sum on the first -- at most 5 in a row:                                                     d_nu <= gamma(5) nu
      m_hat = mu / bc1 and v_hat = nu / bc2: 1 rounding each; s = sqrt(v_hat): half of v_hat's relative error and 1 rounding:
        d_mh <= d_mu / bc1 + U |m_hat|,   d_s <= s ((gamma(5) + U) / 2 + U)
      u = lr m_hat / (s + eps): 3 roundings of its own (product, sum, division) and, to first order, the two operands' errors;
        the second-order remainder is the factor 1 / (1 - d_s / (s + eps)):
        d_u <= (lr d_mh / (s + eps) + |u| d_s / (s + eps)) / (1 - d_s / (s + eps)) + gamma(3) |u|
      p - u: half a float32 spacing at the result (taken at |p_ref| + everything above, which may sit in the next binade).
    A result below 2^-126 may be flushed: TINY on mu and nu.
    Optional, for a chain that is not restarted or a reference with other constants (constant_distance): rel_m / rel_v / rel_u are
    further relative perturbations of A_m / nu / u, m_err (absolute) and v_rel (relative) the errors already on the m and v that came
    in, p_err the one on p.  Returns dict(p, mu, nu, v_rel): v_rel is nu's relative bound, to hand to the next step."""
    gi = _clean_gradient(g, mult, xp)
    _, mi, vi = adam_reference(p, g, m, v, mult, c, xp)
    p_ref = adam_reference(p, g, m, v, mult, c, xp)[0]
    A_m = c['b1'] * xp.abs(m) + c['omb1'] * xp.abs(gi)
    d_mu = (gamma(4) + rel_m) * A_m + c['b1'] * m_err + TINY
    rv = gamma(5) + rel_v + v_rel
    d_nu = rv * vi + TINY
    mh, s = mi / c['bc1'], xp.sqrt(vi / c['bc2'])
    d_mh = d_mu / c['bc1'] + U * xp.abs(mh)
    d_s = s * ((rv + U) / 2 + U) + float(np.sqrt(TINY / c['bc2']))       # (sqrt(v + d) - sqrt(v) <= sqrt(d) for the flushed part)
    den = s + c['eps']
    u = c['lr'] * mh / den
    d_u = (c['lr'] * d_mh / den + xp.abs(u) * d_s / den) / (1 - d_s / den) + (gamma(3) + rel_u) * xp.abs(u)
    d_p = d_u + p_err
    d_p = d_p + 0.5 * ulp32(xp.abs(p_ref) + d_p, xp)
    return dict(p=d_p, mu=d_mu, nu=d_nu, v_rel=rv)


# ------------------------------------------------------------------------------------------------------------ slab and column sums
def slab_sum_reference(slabs, scale):
    """slabs [ksplit, ...] float32 -> scale * sum over the slabs, float64"""
    return scale * f64(slabs).sum(0)


def slab_sum_bound(slabs, scale):
    """slab_sum_kernel / slab_sum2_kernel: group g adds s = g, g + 4, ... one after the other -- ceil(ksplit / 4) terms, so at most
    that many roundings on any term --, the 4 group sums are added in order (3 roundings), the product with `scale` is 1 more; each at
    most U of the sum of magnitudes.  The count is ceil(ksplit / 4) + 3 (the first term of a group is not rounded).
                                                                          (ceil(ksplit / 4) + 3) U |scale| sum_s |slabs[s][e]|"""
    ksplit = np.shape(slabs)[0]
    return (-(-ksplit // 4) + 3) * U * abs(scale) * np.abs(f64(slabs)).sum(0)


def col_sum_reference(dz, scale=1.0):
    """dz [m, n_out] bfloat16 values (held in float32) -> scale * column sums, float64"""
    return scale * f64(dz).sum(0)


def col_sum_bound(dz, nslice, scale=1.0):
    """col_sum_kernel adds a slice's rows_per_slice = ceil(m / nslice) rows one after the other (that many roundings at most on a
    term), slab_sum_kernel then adds the nslice partials: ceil(nslice / 4) + 3 more, as slab_sum_bound counts them.
                                                                 (rows_per_slice + ceil(nslice / 4) + 3) U |scale| sum_m |dZ[m][o]|"""
    m = np.shape(dz)[0]
    return (-(-m // nslice) + -(-nslice // 4) + 3) * U * abs(scale) * np.abs(f64(dz)).sum(0)


def col_dot_reference(h, z):
    """the one-column weight gradient: h [m, n_in], z [m] bfloat16 values -> (H^T z [n_in], sum z), float64"""
    return f64(h).T @ f64(z), f64(z).sum()


def col_dot_tolerance(want):
    """The tolerance form of tests/test_gpu_mip360_fm.py::test_one_column_kernels for a float32 column dot product of bfloat16
    operands: 2e-5 of the largest entry.  (Products of two bfloat16 values are exact in float32; a sum of m terms in float32 loses at
    most m U of the sum of magnitudes, 2e-5 is 336 U.)"""
    return 2e-5 * np.abs(want).max()


def col_dot_bias_bound(z, m, ksplit):
    """grad_weight_col_kernel's bias: a thread adds every 8th row of its slice of ceil(m / ksplit) rows one after the other, the 8 row
    threads are added in order, the slices as slab_sum_bound counts them.
                                                          (ceil(ceil(m / ksplit) / 8) + 8 + ceil(ksplit / 4) + 3) U sum_m |z[m]|
    and never more than the 1e-4 tests/test_gpu_mip360_fm.py::test_one_column_kernels allows the same sum (bfloat16 values of unit size
    have 8 significant bits, so most of these float32 additions are exact and the count above is generous)."""
    per = -(-m // ksplit)
    return min((-(-per // 8) + 8 + -(-ksplit // 4) + 3) * U * np.abs(f64(z)).sum(), 1e-4)


# ------------------------------------------------------------------------------------------------------------ head backward
def head_backward_reference(density, g_density, rgb=None, g_rgb=None, pad=0.001):
    """d_raw = g (1 - e^-d) as g (-expm1(-d)); d_pre = g (1 + 2p) s (1 - s), s = (rgb + p) / (1 + 2p); p as the float the kernel gets.
    Returns (d_raw, d_pre or None) in float64, before the bfloat16 rounding."""
    d, g = f64(density), f64(g_density)
    d_raw = g * -np.expm1(-d)
    if rgb is None:
        return d_raw, None
    p = f32r(pad)
    s = (f64(rgb) + p) / (1 + 2 * p)
    return d_raw, f64(g_rgb) * (1 + 2 * p) * s * (1 - s)


def _bf16_flush(want):
    """a result below the smallest normal bfloat16 (2^-126) may come back as 0: its own magnitude"""
    return np.where(np.abs(want) < TINY, np.abs(want), 0.0)


def head_backward_bounds(density, g_density, rgb=None, g_rgb=None, pad=0.001):
    """density head: float32 forms 1 - expf(-d) -- expf (1 U next to 1), the subtraction (exact or 1 U), the product: 3 U |g| in absolute
      terms, because for d < 1e-5 the difference cancels and a relative bound would not hold -- then rounds to bfloat16: half a spacing,
      2^-8 of the binade's base, which is at most the value (1 + 2^-7: the float32 value may sit just above the float64 one's binade).
                                                                                   |g| (2^-8 (1 - e^-d) (1 + 2^-7) + 3 U)
    colour head: s from 3 roundings (rgb + p, 1 + 2p, the division), 1 - s cancels next to s = 1 (absolute: 3 U s + U), three products
      and 1 + 2p again: 8 U |g| covers them for s in [0, 1]; then the bfloat16 rounding as above.
                                                                                   |g| (2^-8 |s (1 - s)| (1 + 2p) (1 + 2^-7) + 8 U)
    Either result below 2^-126 may be flushed to 0 (_bf16_flush)."""
    d, g = f64(density), np.abs(f64(g_density))
    want_raw, want_pre = head_backward_reference(density, g_density, rgb, g_rgb, pad)
    b_raw = g * (BF16_HALF_ULP * -np.expm1(-d) * (1 + 2.0 ** -7) + 3 * U) + _bf16_flush(want_raw)
    if rgb is None:
        return b_raw, None
    p = f32r(pad)
    s = (f64(rgb) + p) / (1 + 2 * p)
    b_pre = np.abs(f64(g_rgb)) * (BF16_HALF_ULP * np.abs(s * (1 - s)) * (1 + 2 * p) * (1 + 2.0 ** -7) + 8 * U) + _bf16_flush(want_pre)
    return b_raw, b_pre


# ------------------------------------------------------------------------------------------------------------ packing
def fm_index(r, c, ld):
    """element index of (r, c) in a fragment-major tensor with ld columns (include/mip360_hip.h; pinned against mip360_to_fm by
    tests/test_gpu_mip360_fm.py::test_to_fm_from_fm_follow_the_documented_formula)"""
    r, c = np.asarray(r), np.asarray(c)
    row, f = r % 32, c % 16
    hi, t = (f // 4) % 2, 4 * (f // 8) + f % 4
    unit = 8 * (row >> 2) + 4 * (hi ^ (row >> 4)) + (row & 3)
    return ((r // 32) * (ld // 16) + c // 16) * 512 + unit * 8 + t


def pack_reference(kernel, fwd=None, ld_fwd=0, bwd=None, ld_bwd=0, fwd_fm=None, ld_fwd_fm=0, bwd_fm=None, ld_bwd_fm=0, bwd_rows=0,
                   bwd_col0=0):
    """pack_weight_kernel on host arrays.  kernel [n_in, n_out] float32; every destination is a flat float32 array holding bfloat16
    values (whatever it held before stays outside the written window) or None.  fwd[o, i], bwd[i, o], fwd_fm (o, i), bwd_fm
    (i, bwd_col0 + o) for i < bwd_rows.  Exact: round to nearest even, nothing else.  Returns the destinations."""
    n_in, n_out = kernel.shape
    q = round_bf16(kernel)
    ii, oo = np.meshgrid(np.arange(n_in), np.arange(n_out), indexing='ij')
    if fwd is not None:
        fwd[oo * ld_fwd + ii] = q
    if bwd is not None:
        bwd[ii * ld_bwd + oo] = q
    if fwd_fm is not None:
        fwd_fm[fm_index(oo, ii, ld_fwd_fm)] = q
    if bwd_fm is not None:
        keep = ii < bwd_rows
        bwd_fm[fm_index(ii[keep], bwd_col0 + oo[keep], ld_bwd_fm)] = q[keep]
    return fwd, bwd, fwd_fm, bwd_fm


# ------------------------------------------------------------------------------------------------------------ input families
NORM_SIZES = (1, 3, 4, 1023, 4097, 1000003)
NORM_BLOCKS = (1, 7, 256)
NORM_SCALES = (1e-20, 1e-7, 1.0, 1e15)
ADAM_SIZES = (1, 255, 256, 257, 70001)
ADAM_STEPS = (1, 2, 10, 513, 100000)
ADAM_SCALES = (1e-12, 3e-7, 1e-3, 1.0)
SLAB_KSPLITS = (1, 2, 3, 4, 5, 12, 13, 16, 17, 29, 32, 33, 256)
SLAB_SHAPES = ((5, 5, 3, 3), (504, 512, 8, 8), (16, 16, 1, 1), (7, 8, 4, 6), (64, 64, 256, 256))          # rows, n_in, n_out, ldg
SLAB_SCALES = (1.0, 0.25, -3.0)
HEAD_DENSITIES = (0.0, 1e-9, 1e-8, 1e-7, 1e-6, 1e-5, 1.0, 20.0, 88.0, 160.0)


def adam_case(rs, n, step, scale, lr=2e-3):
    """p, g, m, v (float32).  Every 7th gradient is exactly 0.  Above step 1 the moments are those of a history whose gradients had
    the magnitude of g and, on every other element, the opposite sign, so that b1 m and (1 - b1) g cancel there; a tenth of the
    elements sit within 1e-3 of complete cancellation b1 m = -(1 - b1) g."""
    g = (rs.randn(n) * scale).astype(np.float32)
    g[::7] = 0
    p = rs.randn(n).astype(np.float32) * np.float32(0.1)
    if step == 1:
        return p, g, np.zeros(n, np.float32), np.zeros(n, np.float32)
    sign = np.where(np.arange(n) % 2 == 0, -1.0, 1.0)
    m = sign * np.abs(rs.randn(n) * scale) * (1 - 0.9 ** (step - 1))
    near = rs.rand(n) < 0.1
    m = np.where(near, -f64(g) / 9 * (1 + 1e-3 * rs.randn(n)), m)
    v = (rs.randn(n) * scale) ** 2 * (1 - 0.999 ** (step - 1))
    return p, g, m.astype(np.float32), v.astype(np.float32)


def slab_case(rs, family, ksplit, n):
    """[ksplit, n] float32.  'random': normals over six decades.  'cancelling': slabs 2j and 2j + 1 are equal and opposite up to 1e-4
    of their size, so that the sum is 1e-4 of the sum of magnitudes (an odd last slab stands alone)."""
    x = rs.randn(ksplit, n) * 10.0 ** rs.uniform(-3, 3, (ksplit, 1))
    if family == 'cancelling':
        for j in range(0, ksplit - 1, 2):
            x[j + 1] = -x[j] * (1 + 1e-4 * rs.randn(n))
    return x.astype(np.float32)


def head_case(rs, rows, pad=0.001):
    """density, g_density [rows], rgb, g_rgb [rows, 3] (float32): the densities of HEAD_DENSITIES and the five colours -p, 0, 0.5, 1,
    1 + p in turn (every pairing, the two lists' lengths being coprime with the 3 channels), a third of the rows with a random density
    in [0, 160) and colour in [-p, 1 + p] instead.  Gradients are normals over six decades."""
    r = np.arange(rows)
    density = np.asarray(HEAD_DENSITIES)[r % len(HEAD_DENSITIES)]
    colours = np.array([-pad, 0.0, 0.5, 1.0, 1 + pad])
    rgb = colours[(r[:, None] * 3 + np.arange(3)) % 5]
    free = rs.rand(rows) < 1.0 / 3
    density = np.where(free, rs.uniform(0, 160, rows) * rs.rand(rows) ** 4, density)
    rgb = np.where(free[:, None], rs.uniform(-pad, 1 + pad, (rows, 3)), rgb)
    g_d = rs.randn(rows) * 10.0 ** rs.uniform(-3, 3, rows)
    g_c = rs.randn(rows, 3) * 10.0 ** rs.uniform(-3, 3, (rows, 1))
    return density.astype(np.float32), g_d.astype(np.float32), rgb.astype(np.float32), g_c.astype(np.float32)


def pack_case(rs, n_in, n_out):
    """[n_in, n_out] float32 whose bfloat16 rounding is decided by the rule: a quarter of the elements sit exactly on a tie with an even
    kept mantissa, a quarter on a tie with an odd one, an eighth one float32 spacing to either side of a tie, a sixteenth below the
    normal range of bfloat16 (2^-126), the rest random."""
    x = rs.randn(n_in, n_out).astype(np.float32)
    u = x.view(np.uint32).copy()
    kind = rs.randint(0, 16, x.shape)
    tie = kind < 8
    u[tie] = (u[tie] & np.uint32(0xFFFF0000)) | np.uint32(0x8000)
    u[kind < 4] &= np.uint32(0xFFFEFFFF)                                   # even kept mantissa: the tie rounds down
    odd = (kind >= 4) & (kind < 8)
    u[odd] |= np.uint32(0x00010000)                                        # odd: it rounds up
    u[kind == 8] = (u[kind == 8] & np.uint32(0xFFFF0000)) | np.uint32(0x8001)
    u[kind == 9] = (u[kind == 9] & np.uint32(0xFFFF0000)) | np.uint32(0x7FFF)
    u[kind == 10] &= np.uint32(0x807FFFFF)                                 # exponent 0: subnormal in both formats
    return u.view(np.float32).copy()

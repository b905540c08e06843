"""Float64 restatements and per-element bounds for the ray side of the MipNeRF-360 path (csrc/mip360_kernels.hip: resample_kernel,
cast_encode_kernel, dir_encode_kernel; csrc/mip360_rays.hip: percentiles_kernel), for tests/test_mip360_rays_reference.py (CPU) and
tests/test_gpu_mip360_ray_edges.py (GPU).  Plain numpy on top of oracle/mip360_oracle.py (O), which is dtype-generic; nothing here
touches the code under test, and no constant below was fitted to what a GPU gave: the count of operations stands beside each.

E = 2^-23 is the float32 machine epsilon (one ulp of a number in [1, 2)), U = E / 2 the unit roundoff.

Resampling.  A sample that falls into a bin of density rho moves by (cdf error) / rho, and densities reach 1e-5 (the resampling
padding) and 1e4 (a narrow input bin dilated), so no tolerance stated in sample space holds for every correct float32 implementation.
The reference therefore (a) forms the dilated edges as the kernel does, in float32 with one rounding each -- sorting and clipping are
exact, so the edges of the step function carry no ambiguity -- and does everything after that in float64, and (b) states the tolerance
in cdf space: the inverse cdf F^-1 is monotone, so a kernel whose cdf is off by at most delta anywhere puts centre k inside
[F^-1(u_k - delta), F^-1(u_k + delta)].  delta = E (nb + 16) for nb bins:
    nb - 1   roundings of the running sum, half an ulp of a value <= 1 each      -> (nb - 1) E / 2
    nb - 1   the same for the sum of the softmax's exponentials (any order)       -> (nb - 1) E / 2
    16       log, exp (2 ulp each), + padding, * anneal, - max, the division, and the pdf / pool / renormalisation behind the
             weight (subtraction, division, product, sum, division: 5), in ulps of the term; the terms sum to 1, so 16 E in all
A centre is accepted in [lo - 4 E, hi + 4 E]: the kernel's own interpolation t0 + off (t1 - t0) in float32 is a subtraction, a
division, a product, a sum (4 roundings of values <= 1) and the same again for the float32 `off` entering a width <= 1.
The rule covers a `u` within delta of a cdf edge (the bracket may switch: both brackets are inside the envelope) and excludes nothing.

cast_encode.  feature = damp sin(2^k lm [+ pi/2]), damp = exp(-4^k lv / 2).  With d_lm / d_lv the float32 error of the lifted mean /
variance, |error| <= A + damp (2^k d_lm + 4^k d_lv / 2 + argument terms): see encode_bound()."""
import numpy as np

from oracle import mip360_oracle as O

E = 2.0 ** -23                       # float32 epsilon
U = 2.0 ** -24                       # unit roundoff
f32, f64 = np.float32, np.float64
CENTRE_SLACK = 4 * E                 # see the module docstring
DELTA_TERMS = 16                     # see the module docstring
EDGE_ULPS = 2                        # an interval edge: one sum and one difference of centres in float32


def F64(a):
    return np.asarray(a, f64)


def envelope_ratio(got, lo, want, hi):
    """position of `got` in the envelope [lo, hi] around the float64 value `want` (lo <= want <= hi): (got - want) / (hi - want) above,
    (want - got) / (want - lo) below, so <= 1 exactly when inside; a value that is not finite counts as inf"""
    got, lo, want, hi = F64(got), F64(lo), F64(want), F64(hi)
    with np.errstate(divide='ignore', invalid='ignore'):
        r = np.where(got >= want, (got - want) / (hi - want), (want - got) / (want - lo))
    r = np.where(got == want, 0.0, r)
    return np.where(np.isfinite(got), np.nan_to_num(r, nan=np.inf), np.inf)


def excess(got, lo, hi):
    """distance outside [lo, hi] (0 inside), for a failure's message"""
    got = F64(got)
    return np.maximum(0, np.maximum(F64(lo) - got, got - F64(hi)))


def err_ratio(got, want, bound):
    """|got - want| / bound per element; not finite or off where the bound is 0 counts as inf"""
    got, want = F64(got), F64(want)
    bound = F64(bound) + np.zeros_like(want)
    err = np.abs(got - want)
    with np.errstate(divide='ignore', invalid='ignore'):
        r = np.where(err == 0, 0.0, err / bound)
    return np.where(np.isfinite(got), np.nan_to_num(r, nan=np.inf), np.inf)


# ------------------------------------------------------------------------------------------------------------ resampling
def dilated_edges(sd, dilation, domain=(0.0, 1.0)):
    """float32, as the kernel forms them: t[:-1] - d and t[1:] + d with one rounding each, concatenated, sorted, clipped.  Returns
    (td, t0, t1) with t0 / t1 unclipped."""
    sd, d = np.asarray(sd, f32), f32(dilation)
    t0, t1 = sd[..., :-1] - d, sd[..., 1:] + d
    td = np.clip(np.sort(np.concatenate([sd, t0, t1], -1), -1), f32(domain[0]), f32(domain[1]))
    assert td.dtype == f32 and t0.dtype == f32
    return td, t0, t1


def step_function(sd, w, dilation, anneal, padding, domain=(0.0, 1.0)):
    """models.py:158-183 for one level: (edges, logits) of the step function that is sampled, float64 from float32 edges and
    float32 weights.  dilation / anneal / padding are rounded to float32 first (the C ABI takes floats)."""
    sd, w = np.asarray(sd, f32), np.asarray(w, f32)
    if f32(dilation) > 0:
        td, t0, t1 = dilated_edges(sd, dilation, domain)
        p = F64(w) / np.maximum(O.EPS32 ** 2, np.diff(F64(sd), axis=-1))                    # pdf with the eps^2 floor
        cover = (t0[..., None, :] <= td[..., None]) & (t1[..., None, :] > td[..., None])    # unclipped float32 t0, t1
        pd = np.max(np.where(cover, p[..., None, :], 0.0), -1)[..., :-1]
        wd = pd * np.diff(F64(td), axis=-1)
        wd = wd / np.maximum(O.EPS32 ** 2, wd.sum(-1, keepdims=True))
        t, w64 = F64(td)[..., 1:-1], wd[..., 1:-1]
    else:
        t, w64 = F64(sd), F64(w)
    with np.errstate(divide='ignore'):
        logits = np.where(t[..., 1:] > t[..., :-1], F64(f32(anneal)) * np.log(w64 + F64(f32(padding))), -np.inf)
    return t, logits


def uniform_positions(shape_prefix, ns, jitter01):
    """stepfun.py:195-213 in double, rounded to float32 as the kernel does (`uf`), returned as float64"""
    return F64(O.sample_u(shape_prefix, ns, jitter01, True, True, f32))


def delta_cdf(nb):
    return E * (nb + DELTA_TERMS)


def centre_envelope(t, logits, u):
    """(lo, hi, centre): F^-1(u -+ delta) without the slack, and the float64 centres themselves"""
    with np.errstate(invalid='ignore'):
        cw = O.integrate_weights(O.softmax(logits))
    d = delta_cdf(logits.shape[-1])
    inv = lambda x: O.sorted_interp(np.clip(x, 0.0, 1.0), cw, t)
    return inv(u - d), inv(u + d), inv(u)


def interval_bounds(lo, hi, domain=(0.0, 1.0)):
    """bounds of the ns + 1 interval edges of sample_intervals (stepfun.py:253-270) from the bounds of the ns centres, slack included:
    interior edges are means of neighbours; the first is 1.5 c0 - 0.5 c1 (so it mixes lo and hi), the last likewise; both are then
    clipped as the kernel clips them; EDGE_ULPS ulps of the value on top (E |v| >= one ulp of v)."""
    lo, hi = lo - CENTRE_SLACK, hi + CENTRE_SLACK
    mid_lo, mid_hi = (lo[..., 1:] + lo[..., :-1]) / 2, (hi[..., 1:] + hi[..., :-1]) / 2
    first_lo, first_hi = 1.5 * lo[..., :1] - 0.5 * hi[..., 1:2], 1.5 * hi[..., :1] - 0.5 * lo[..., 1:2]
    last_lo, last_hi = 1.5 * lo[..., -1:] - 0.5 * hi[..., -2:-1], 1.5 * hi[..., -1:] - 0.5 * lo[..., -2:-1]
    a, b = F64(f32(domain[0])), F64(f32(domain[1]))
    e_lo = np.concatenate([np.maximum(a, first_lo), mid_lo, np.minimum(b, last_lo)], -1)
    e_hi = np.concatenate([np.maximum(a, first_hi), mid_hi, np.minimum(b, last_hi)], -1)
    return e_lo - EDGE_ULPS * E * np.abs(e_lo), e_hi + EDGE_ULPS * E * np.abs(e_hi)


def intervals_of(centres, domain=(0.0, 1.0)):
    """sample_intervals (stepfun.py:253-270) from the centres on"""
    mid = (centres[..., 1:] + centres[..., :-1]) / 2
    first = np.maximum(centres.dtype.type(domain[0]), 2 * centres[..., :1] - mid[..., :1])
    last = np.minimum(centres.dtype.type(domain[1]), 2 * centres[..., -1:] - mid[..., -1:])
    return np.concatenate([first, mid, last], -1)


def resample_bounds(sd, w, dilation, anneal, padding, ns, jitter01, domain=(0.0, 1.0)):
    """everything the tests need for one call: dict(lo, hi) of the sdist edges [n, ns + 1], the centre envelope and nb"""
    t, logits = step_function(sd, w, dilation, anneal, padding, domain)
    u = uniform_positions(t.shape[:-1], ns, jitter01)
    c_lo, c_hi, c = centre_envelope(t, logits, u)
    e_lo, e_hi = interval_bounds(c_lo, c_hi, domain)
    want = intervals_of(c, domain)
    return dict(lo=e_lo, hi=e_hi, want=want, c_lo=c_lo - CENTRE_SLACK, c_hi=c_hi + CENTRE_SLACK, centres=c, nb=logits.shape[-1], t=t, logits=logits)


# ------------------------------------------------------------------------------------------------------------ percentiles
PERCENTILES = (5, 50, 95)


def percentile_reference(tdist, weights, t_far):
    """render.py:204-214.  np.cumsum of float32 is the sequential float32 sum, the bits of the kernel's prefix; np.interp runs in
    double; the result is rounded to float32.  (The background weight max(0, 1 - acc) is the last bin, which integrate_weights drops.)"""
    tdist, weights = np.asarray(tdist, f32), np.asarray(weights, f32)
    t_aug = np.concatenate([tdist, np.asarray(t_far, f32).reshape(-1, 1)], -1)
    w_aug = np.concatenate([weights, np.zeros_like(weights[..., :1])], -1)
    assert O.integrate_weights(w_aug).dtype == f32
    return O.weighted_percentile(t_aug, w_aug, list(PERCENTILES)).astype(f32)


def ulp32(x):
    """one float32 ulp at |x| (float64)"""
    x = np.abs(np.asarray(x, f32))
    return F64(np.nextafter(x, f32(np.inf))) - F64(x)


def percentile_bound(want):
    return ulp32(want)                                   # 1 float32 ulp


# ------------------------------------------------------------------------------------------------------------ cast_encode
N_DEG, N_BASIS = 12, 21
T_REDUCE32 = float(f32(100 * np.pi))                     # safe_sin's period as float32 arithmetic sees it
T_REDUCE_ERR = abs(T_REDUCE32 - 100 * np.pi)             # 5.9e-6: what each subtracted period adds to the phase (upstream's float32 too)
A_FLOOR = 8 * U                                          # sinf 2 ulp (4 U of a value <= 1), expf 1 ulp (2 U), the product (1 U): 7 -> 8
C_TMEAN = 6                                              # mu 1; c = 2 mu hw^2 / denom 5 + 5 + 1 = 11 at c <= t_mean / 3; the sum 1
C_MEAN = C_TMEAN + 1                                     # ... and the product d t_mean
C_CONTRACT = 14                                          # m2 3, sqrt 2.5, 2r - 1 -> 6, / m2 -> 10, s x 11, the dot with the basis 3
C_V = 30                                                 # v = J^T b relative to ||J||: J's entries 8 (the mean's error) + 10 (s) or 5 (the
                                                         # rank-one term, whose 1 - r cancels: absolute 2.5 U r), the products 4, the dot 3
C_TVAR = (5, 28)                                         # hw^2 / 3: 1 + 2 + 1 + 1;  (4/15) hw^4 (12 mu^2 - hw^2) / denom^2: 1 + 7 + 1 + 5 + 1 + 11 + 1, + the sum
C_RVAR = 19                                              # (4/15) hw^4 / denom: 1 + 7 + 1 + 5 + 1 = 15, the two sums 2, br br and the product 2
C_OUTER = 3                                              # d_a d_b, the product with t_var, the sum of the two parts
C_NULL = 8                                               # I - d (d / dms): dms 3, the quotient 1, the product 1, the difference 1 -> 6; x r_var and the sum 2
C_DOTS = 6                                               # cov v (3 products, 2 sums -> 3) and v . (cov v) (3)


def encode_chain(tdist, origins, directions, radii, basis, dtype=f64, floor=True, diag=False, rank_one=True, full=False):
    """cast_rays(cone) -> contract with its Jacobian -> lift -> (lm, lv) in `dtype`, written out so that the three mutants of the CPU
    test can be switched on: floor=False drops the eps floor of denom, diag=True takes the diagonal covariance, rank_one=False drops
    the Jacobian's rank-one term.  With the defaults and float64 it is the chain of O (asserted by the CPU test)."""
    c = lambda a: np.asarray(a, dtype)
    td, o, d, br = c(tdist), c(origins), c(directions), c(radii).reshape(-1, 1)
    t0, t1 = td[..., :-1], td[..., 1:]
    mu, hw = (t0 + t1) / 2, (t1 - t0) / 2
    eps = dtype(np.finfo(f32).eps)
    with np.errstate(divide='ignore', invalid='ignore'):
        denom = 3 * mu ** 2 + hw ** 2
        if floor:
            denom = np.maximum(eps, denom)
        t_mean = mu + (2 * mu * hw ** 2) / denom
        t_var = (hw ** 2) / 3 - dtype(4 / 15) * hw ** 4 * (12 * mu ** 2 - hw ** 2) / denom ** 2
        r_var = ((mu ** 2) / 4 + dtype(5 / 12) * hw ** 2 - dtype(4 / 15) * (hw ** 4) / denom) * br ** 2
    mean = d[..., None, :] * t_mean[..., None] + o[..., None, :]
    dms = np.maximum(dtype(1e-10), np.sum(d ** 2, -1, keepdims=True))
    eye = np.eye(3, dtype=dtype)
    if diag:
        cov = (t_var[..., None] * (d ** 2)[..., None, :] + r_var[..., None] * (1 - d ** 2 / dms)[..., None, :])[..., None] * eye
    else:
        d_outer = d[..., :, None] * d[..., None, :]
        null_outer = eye - d[..., :, None] * (d / dms)[..., None, :]
        cov = t_var[..., None, None] * d_outer[..., None, :, :] + r_var[..., None, None] * null_outer[..., None, :, :]
    m2 = np.maximum(eps, np.sum(mean ** 2, -1, keepdims=True))
    r = np.sqrt(m2)
    s = (2 * r - 1) / m2
    ds = (1 - r) / (m2 * m2)
    cm = np.where(m2 <= 1, mean, s * mean)
    outer = mean[..., :, None] * mean[..., None, :] if rank_one else np.zeros(mean.shape + (3,), dtype)
    J = np.where(m2[..., None] <= 1, eye, s[..., None] * eye + 2 * ds[..., None] * outer)
    ccov = J @ cov @ np.swapaxes(J, -1, -2)
    b = c(basis)
    if full:
        return dict(J=J, cov=cov, mean=mean, cm=cm, t_mean=t_mean, t_var=t_var)
    return cm @ b, np.sum(b * (ccov @ b), -2)


def encode_features(lm, lv, dtype=f64):
    """integrated_pos_enc(0, 12) in `dtype` -> [..., 504]; float32 reproduces safe_sin's float32 period"""
    out = O.integrated_pos_enc(np.asarray(lm, dtype), np.asarray(lv, dtype), 0, N_DEG)
    assert out.dtype == dtype
    return out


def encode_reference(tdist, origins, directions, radii, basis):
    """the float64 chain of tests/test_gpu_mip360.py -> dict(want [rows, 504], lm, lv [rows, 21])"""
    means, covs = O.cast_rays(F64(tdist), F64(origins), F64(directions), F64(radii).reshape(-1, 1), 'cone', diag=False)
    m, cv = O.track_linearize_contract(means, covs)
    lm, lv = O.lift_and_diagonalize(m, cv, F64(basis))
    rows = lm.shape[0] * lm.shape[1]
    return dict(want=O.integrated_pos_enc(lm, lv, 0, N_DEG).reshape(rows, 2 * N_DEG * N_BASIS), lm=lm.reshape(rows, N_BASIS),
                lv=lv.reshape(rows, N_BASIS))


def encode_deltas(tdist, origins, directions, radii, basis):
    """(d_lm [rows, 1], d_lv [rows, 21]): absolute float32 error bounds of the lifted mean (for any unit basis vector) and of the lifted
    variance of each basis vector, from the input magnitudes and the counts above (all first order in U; (1 + 1e-3) holds the rest):
      t_mean        C_TMEAN U t_mean                                   (c = 2 mu hw^2 / denom >= 0 and <= t_mean / 3)
      mean          U (C_MEAN |d| t_mean + |mean|)                     (the product and the sum with the origin)
      contraction   ||J||_2 times that (||J||_2 = 1 inside the unit ball, s = (2 r - 1) / r^2 outside: the radial gain 1 / r^2 is smaller)
      evaluation    C_CONTRACT U |contract(mean)|
      lv = v^T cov v, v = J^T b:
        from v      2 |cov v| C_V U ||J||  +  (C_V U ||J||)^2 ||cov||   -- |cov v| is taken after ITS cancellation (d . v is small for a
                    far sample although |d| |v| is not), which is what makes a wide far interval testable at all
        from cov    |v|^2 (|d|^2 (U (5 A1 + 28 A2) + C_OUTER U |t_var|) + 2 C_RVAR U R + 3 C_NULL U R), A1 / A2 the magnitudes of
                    the two terms of t_var (they cancel), R the sum of magnitudes of r_var's terms
        the dots    C_DOTS U |v|^2 (|d|^2 |t_var| + 2 R)"""
    td, d, br = F64(tdist), F64(directions), F64(radii).reshape(-1, 1)
    q = encode_chain(tdist, origins, directions, radii, basis, full=True)
    t0, t1 = td[..., :-1], td[..., 1:]
    mu, hw = (t0 + t1) / 2, (t1 - t0) / 2
    denom = np.maximum(E, 3 * mu ** 2 + hw ** 2)
    A1, A2 = hw ** 2 / 3, (4 / 15) * hw ** 4 * (12 * mu ** 2 + hw ** 2) / denom ** 2
    R = (mu ** 2 / 4 + (5 / 12) * hw ** 2 + (4 / 15) * hw ** 4 / denom) * br ** 2
    dn = np.sqrt(np.sum(d ** 2, -1, keepdims=True))
    r = np.sqrt(np.maximum(E, np.sum(q['mean'] ** 2, -1)))
    d_mean = U * (C_MEAN * dn * np.abs(q['t_mean']) + r)
    gain = np.where(r <= 1, 1.0, (2 * r - 1) / r ** 2)
    # a mean within its own error of the unit sphere may take either branch: the map and its Jacobian are continuous there
    # (s = 1 + O(e^2), the rank-one term O(e) for r = 1 + e), which C_V and C_CONTRACT already hold
    cnorm = np.where(r <= 1, r, 2 - 1 / r)
    d_lm = (gain * d_mean + C_CONTRACT * U * cnorm) * (1 + 1e-3)
    b = F64(basis)
    v = np.swapaxes(q['J'], -1, -2) @ b                                  # [n, S, 3, 21]
    cv = q['cov'] @ v
    v2 = np.sum(v ** 2, -2)
    d_v = C_V * U * gain[..., None]
    cov_norm = (dn ** 2 * np.abs(q['t_var']) + 2 * R)[..., None]
    from_v = 2 * np.sqrt(np.sum(cv ** 2, -2)) * d_v + d_v ** 2 * cov_norm
    from_cov = v2 * (dn ** 2 * U * (C_TVAR[0] * A1 + C_TVAR[1] * A2 + C_OUTER * np.abs(q['t_var'])) + (2 * C_RVAR + 3 * C_NULL) * U * R)[..., None]
    dots = C_DOTS * U * v2 * cov_norm
    d_lv = (from_v + from_cov + dots) * (1 + 1e-3)
    return d_lm.reshape(-1, 1), d_lv.reshape(-1, N_BASIS)


def in_todays_domain(tdist, origins, directions, radii):
    """per row: inside the domain tests/test_gpu_mip360.py::test_cast_encode_matches_oracle has always covered -- unit directions,
    origins within 1.5 of the centre (its origins are 0.3 N(0, I)), 0.2 <= t <= 50, radii up to 2e-3 -- where its tolerance
    2e-6 + 3e-6 2^k max(1, |lm|) is the accepted contract and the bound below is capped by it.  A worst-case count cannot get under
    that tolerance everywhere there: for a wide far interval it allows the lifted variance 15 % (sums of magnitudes that cancel), and
    x e^-x times that is 30 times the tolerance at the middle degrees, while float32 arithmetic stays at a tenth of the count."""
    td, o, d, br = F64(tdist), F64(origins), F64(directions), F64(radii).reshape(-1, 1)
    ray = (np.abs(np.sqrt(np.sum(d ** 2, -1, keepdims=True)) - 1) <= 1e-6) & (np.sqrt(np.sum(o ** 2, -1, keepdims=True)) <= 1.5) & \
        (br <= F64(f32(2e-3)))
    row = ray & (td[..., :-1] >= F64(f32(0.2)) * (1 - 1e-6)) & (td[..., 1:] <= 50 * (1 + 1e-6))
    return row.reshape(-1, 1)


def encode_bound(ref, d_lm, d_lv, today=None):
    """per element [rows, 504]:  A + damp (2^k d_lm + 4^k d_lv / 2 + U (|x| + 2) + reduction), x = 2^k lm:
      U (|x| + 2)   the rounding of x + pi / 2 (x = 2^k lm itself is exact), and pi / 2 as a float
      reduction     for |x| >= 100 pi only: x - floor(x / t) t in float32 (2 U |x|) with the float32 period (q T_REDUCE_ERR, q periods)
    damp is taken at lv - d_lv (the bound must hold for the kernel's own damping too).  today: in_todays_domain(), the rows on which
    the tolerance this bound replaces caps it."""
    lm, lv = ref['lm'], ref['lv']
    k = np.arange(N_DEG)[None, :, None]
    x = np.abs(lm[:, None, :]) * 2.0 ** k
    damp = np.exp(-0.5 * 4.0 ** k * np.maximum(0, lv[:, None, :] - d_lv[:, None, :]))
    q = np.floor((x + 2) / T_REDUCE32) + 1
    reduce_ = np.where(x + 2 >= T_REDUCE32 * (1 - E), 2 * U * x + q * T_REDUCE_ERR, 0.0)
    b = A_FLOOR + damp * (2.0 ** k * d_lm[:, None, :] + 0.5 * 4.0 ** k * d_lv[:, None, :] + U * (x + 2) + reduce_)
    b = b.reshape(lm.shape[0], N_DEG * N_BASIS)
    b = np.concatenate([b, b], -1)
    return b if today is None else np.where(today, np.minimum(b, existing_encode_bound(ref)), b)


# bf16 rows: the kernel evaluates the degrees 0, 2, 5, 8 directly (hardware sine / cosine / exp2) and the others by angle doubling.  Its
# comment states the absolute budget 4e-6 at degree 1, 1e-5 at 4 and 7, 1e-4 at 11, and <= 2.8 per doubling; the degrees between follow
# by dividing by 2.8 per doubling back to the directly evaluated one (tests/test_layout_emulation.py holds the numpy twin to them).
DOUBLING = np.array([4e-6 / 2.8, 4e-6, 1e-5 / 2.8 ** 2, 1e-5 / 2.8, 1e-5, 1e-5 / 2.8 ** 2, 1e-5 / 2.8, 1e-5,
                     1e-4 / 2.8 ** 3, 1e-4 / 2.8 ** 2, 1e-4 / 2.8, 1e-4])


def encode_bound_bf16(ref, bound32):
    """the float32 bound, half a bf16 ulp of the reference (bf16_half_ulp: exactly, i.e. 2^-9 |want| at the top of a binade and
    2^-8 |want| at its base), and the doubling budget of the degree"""
    per_col = np.tile(np.repeat(DOUBLING, N_BASIS), 2)
    return bound32 + bf16_half_ulp(ref['want']) + per_col[None, :]


def existing_encode_bound(ref):
    """the tolerance of tests/test_gpu_mip360.py::test_cast_encode_matches_oracle, which encode_bound must not exceed on its inputs"""
    scale = np.tile(np.repeat(2.0 ** np.arange(N_DEG), N_BASIS), 2)
    lm = np.tile(np.repeat(ref['lm'][:, None, :], N_DEG, 1).reshape(-1, N_DEG * N_BASIS), 2)
    return 2e-6 + 3e-6 * scale[None, :] * np.maximum(1.0, np.abs(lm))


# ------------------------------------------------------------------------------------------------------------ dir_encode
def dir_reference(viewdirs):
    return O.pos_enc(F64(np.asarray(viewdirs, f32)), 0, 4, append_identity=True)          # [n, 27]


def bf16_half_ulp(x):
    """half a bfloat16 ulp at |x|: 2^(e - 8) for |x| in [2^e, 2^(e + 1)) (8 significand bits), between 2^-9 |x| and 2^-8 |x|"""
    _, e = np.frexp(np.abs(F64(x)))                      # |x| = m 2^e, m in [0.5, 1)
    return np.where(F64(x) == 0, 0.0, np.ldexp(1.0, np.maximum(e - 1, -126) - 8))


def dir_bound(want):
    """half a bf16 ulp of the value plus 4 float32 ulp of 1 (the sine's range), absolute: the product with 2^k is exact, x + pi / 2 rounds
    once, pi / 2 is a float, sinf is good to 2 ulp of a value <= 1"""
    return bf16_half_ulp(want) + 4 * E


def round_bf16(x):
    """float32 -> nearest bfloat16, ties to even, as float32"""
    u = np.ascontiguousarray(x, f32).view(np.uint32)
    r = ((u >> np.uint32(16)) & np.uint32(1)) + np.uint32(0x7FFF)
    return ((u + r) & np.uint32(0xFFFF0000)).view(f32)


# ------------------------------------------------------------------------------------------------------------ the inputs of both tests
# The families of tests/test_gpu_mip360_ray_edges.py, generated here so that the CPU test runs the float32 twins over the very same
# inputs.  Everything is seeded by the case's own parameters.
RESAMPLE_M = (1, 2, 63, 64, 65, 127, 128)                 # 65: the lane-strided loops' second round; 128: 3 m + 1 = 385 edges fill LDS
RESAMPLE_NS = (2, 3, 63, 64)
RESAMPLE_N = (1, 3, 4, 5, 37)                             # four rays per block, a whole wave exits together
RESAMPLE_DILATION = (0.0, 0.0025 + 0.5 / 64, 1 / 64.0, 0.5025)
RESAMPLE_PADDING = (0.0, 1e-5)
RESAMPLE_JITTER = ('none', 'zero', 'one', 'random')       # one: 1 - 2^-24, the largest float32 below 1
RESAMPLE_FAMILIES = ('random', 'third_zero', 'dyadic', 'runs', 'single_bin', 'random')
ANNEAL = 10 * 0.3 / (9 * 0.3 + 1)                         # models.py:176-178 at train_frac 0.3
NEAR_FAR = ((0.05, 50.0), (0.2, 1e6))


def resample_rays(m, n, seed, first_family=0):
    """n rays of m bins, ray i of family RESAMPLE_FAMILIES[(first_family + i) % 6]: (sdist [n, m + 1], weights [n, m], families)"""
    rs = np.random.RandomState(seed)
    sd, w, fams = np.zeros((n, m + 1), f32), np.zeros((n, m), f32), []
    for i in range(n):
        fam = RESAMPLE_FAMILIES[(first_family + i) % len(RESAMPLE_FAMILIES)]
        e = np.sort(rs.rand(m + 1))
        wi = np.exp(rs.randn(m) * 3)
        if fam == 'third_zero' and m > 1:
            wi[::3] = 0
        elif fam == 'dyadic':                              # edges k / 64: massive ties within and across the three lists
            e = np.sort(rs.randint(0, 65, m + 1)) / 64.0
            e[0], e[-1] = 0.0, 1.0
            if m >= 63:
                wi[::3] = 0
        elif fam == 'runs':                                # runs of equal edges: zero-width bins inside the ray
            idx = np.sort(rs.randint(0, m + 1, m + 1))
            idx[0], idx[-1] = 0, m
            e = e[idx]
        elif fam == 'single_bin':
            wi[:] = 0
            wi[rs.randint(m)] = 1
        wi = wi / wi.sum()
        sd[i], w[i] = e, wi
        fams.append(fam)
    live = (np.diff(sd, axis=-1) > 0) & (w > 0)
    assert live.any(-1).all(), 'every ray keeps a bin of positive width and weight'
    return sd, w, fams


def jitter_of(mode, n, seed):
    if mode == 'none':
        return None
    if mode == 'zero':
        return np.zeros((n, 1), f32)
    if mode == 'one':
        return np.full((n, 1), 1 - 2.0 ** -24, f32)
    return np.random.RandomState(seed).rand(n, 1).astype(f32)


def near_far(n):
    nf = np.array([NEAR_FAR[i % 2] for i in range(n)], f32)
    return nf[:, :1].copy(), nf[:, 1:].copy()


def resample_cases(m):
    """the cases of one m_in: every ns x dilation x padding at n = 37 (all families in each, the jitter mode and the first family
    rotating), and the small ray counts at both ends of ns and of the dilation"""
    cases = []
    for a, ns in enumerate(RESAMPLE_NS):
        for b, dil in enumerate(RESAMPLE_DILATION):
            for c, pad in enumerate(RESAMPLE_PADDING):
                cases.append(dict(m=m, ns=ns, n=37, dilation=dil, padding=pad, jitter=RESAMPLE_JITTER[(a + b + 2 * c + m) % 4], first=a + b))
    for a, n in enumerate(RESAMPLE_N[:-1]):
        for b, (ns, dil) in enumerate(((2, 0.5025), (64, 0.0025 + 0.5 / 64), (63, 0.0), (3, 1 / 64.0))):
            cases.append(dict(m=m, ns=ns, n=n, dilation=dil, padding=RESAMPLE_PADDING[(a + b) % 2], jitter=RESAMPLE_JITTER[(a + b) % 4],
                              first=2 * a + b))
    for i, c in enumerate(cases):
        c['seed'] = 1000 * m + i
        c['sd'], c['w'], c['families'] = resample_rays(m, c['n'], c['seed'], c['first'])
        c['jit'] = jitter_of(c['jitter'], c['n'], c['seed'] + 1)
        c['near'], c['far'] = near_far(c['n'])
    return cases


PCT_S = (1, 2, 31, 32, 61, 62)
PCT_N = (1, 3, 4, 5, 257)
PCT_FAMILIES = ('below_one', 'exactly_one', 'above_one', 'all_zero', 'half_then_zeros', 'sparse')


def percentile_case(S, n, t_far_value, first_family=0):
    """ray i of family PCT_FAMILIES[(first_family + i) % 6]: weights summing to < 1, to exactly 1 (dyadic), to > 1 (the min(1, .)
    clamp), all zero, a dyadic prefix that hits 0.5 exactly followed by zero weights (tied cdf values: the last edge with cw <= p),
    and every third weight zero"""
    rs = np.random.RandomState(100 * S + n + first_family)
    tdist = np.sort(rs.uniform(0.2, 30, (n, S + 1)), -1).astype(f32)
    w = np.zeros((n, S), f32)
    for i in range(n):
        fam = PCT_FAMILIES[(first_family + i) % len(PCT_FAMILIES)]
        r = rs.rand(S)
        if fam == 'below_one':
            wi = r / r.sum() / rs.uniform(1.05, 1.6)
        elif fam == 'exactly_one':
            wi = np.zeros(S)
            head = {1: [1.0], 2: [.5, .5], 3: [.5, .25, .25]}.get(S, [.5, .25, .125, .125])
            wi[:len(head)] = head
        elif fam == 'above_one':
            wi = r / r.sum() * rs.uniform(1.1, 1.5)
        elif fam == 'all_zero':
            wi = np.zeros(S)
        elif fam == 'half_then_zeros':
            wi = np.zeros(S)
            head = [.5] if S == 1 else [.25, .25]
            wi[:len(head)] = head
            if S > 6:
                wi[6:] = r[6:] / max(r[6:].sum(), 1e-9) * 0.4
        else:
            wi = r / r.sum() * 0.9
            wi[::3] = 0
        w[i] = wi
    return tdist, w, np.full((n, 1), t_far_value, f32)


ENCODE_ROWS = ((1, 1), (2, 1), (3, 1), (4, 1), (11, 1), (12, 1), (13, 1), (191, 1), (193, 1), (6, 32), (3, 64))     # n, S: n S = 1 ... 193
ENCODE_FM_ROWS = ((1, 32), (1, 64), (3, 32))               # 32, 64, 96 rows of the fragment-major layout


def encode_case(n, S, seed=0):
    """tdist [n, S + 1], origins, directions [n, 3], radii [n, 1].  Ray i: direction unit or scaled up to 1.3 (as frame_rays emits them);
    origin inside the unit ball, on it, at |o| = 50; radius 1e-5, 2e-3, 0.1; zero-width intervals; a last interval that ends at 1e6;
    every seventh ray (and the last one of a multi-sample case) starts at the centre with a unit direction and has its edges one ulp apart around
    t = 1: means within a few ulp of |x| = 1, where the contraction switches branch."""
    rs = np.random.RandomState(7000 + 100 * n + S + seed)
    d = rs.randn(n, 3)
    d /= np.linalg.norm(d, axis=-1, keepdims=True)
    o = rs.randn(n, 3)
    o /= np.linalg.norm(o, axis=-1, keepdims=True)
    tdist = np.zeros((n, S + 1), f32)
    radii = np.zeros((n, 1), f32)
    _, s_to_t = O.construct_ray_warps('reciprocal', np.float64(0.2), np.float64(50.0))
    for i in range(n):
        d[i] *= (1.0, 1.3, 0.8 + 0.5 * rs.rand())[i % 3]
        o[i] *= (0.3 * rs.rand(), 1.0, 50.0)[(i // 3) % 3]
        radii[i] = (1e-5, 2e-3, 0.1)[(i // 2) % 3]
        t = s_to_t(np.sort(rs.rand(S + 1)))
        if S > 4:
            t[3] = t[2]                                    # zero-width intervals
            t[S // 2 + 1] = t[S // 2]
        if i % 2 == 1:
            t[-1] = 1e6                                    # every training ray's last interval
        if i % 5 == 4:
            t[0] = t[1] if S > 1 else t[0]
        tdist[i] = t
        if i % 7 == 6 or (S > 1 and i == n - 1):
            o[i] = 0
            d[i] /= np.linalg.norm(d[i])
            one = np.full(S + 1, 1.0, f32)
            steps = np.arange(S + 1) - (S + 1) // 2         # ... 1 - 2 ulp, 1 - 1 ulp, 1, 1 + 1 ulp, ...
            for k in range(S + 1):
                for _ in range(abs(int(steps[k]))):
                    one[k] = np.nextafter(one[k], f32(2.0 if steps[k] > 0 else 0.0))
            tdist[i] = one
    return tdist, o.astype(f32), d.astype(f32), radii


def existing_encode_case():
    """the inputs of tests/test_gpu_mip360.py::test_cast_encode_matches_oracle"""
    rs = np.random.RandomState(1)
    n, S = 29, 32
    d = rs.randn(n, 3).astype(f32)
    d /= np.linalg.norm(d, axis=-1, keepdims=True)
    o = (rs.randn(n, 3) * 0.3).astype(f32)
    s = np.sort(rs.rand(n, S + 1), -1).astype(f32)
    _, s_to_t = O.construct_ray_warps('reciprocal', np.full((n, 1), 0.2, f32), np.full((n, 1), 50., f32))
    return s_to_t(s).astype(f32), o, d, np.full((n, 1), 2e-3, f32)


DIR_SHAPES = ((1, 1), (5, 3), (9, 64))                     # n, S
DIR_WIDTH = (27, 32)
DIR_COL0 = (0, 8, 5)


def dir_case(n):
    """viewdirs [n, 3]: the components +-1 and 0 first, then random unit vectors"""
    fixed = np.array([[1, 0, 0], [0, -1, 0], [0, 0, 1], [-1, 0, 0], [0, 1, -1], [-1, 1, 0]], f64)
    v = np.random.RandomState(n).randn(n, 3)
    v /= np.linalg.norm(v, axis=-1, keepdims=True)
    k = min(n, len(fixed)) if n > 1 else 0
    v[:k] = fixed[:k]
    return v.astype(f32)

"""Edge-case inputs and float64 error bounds for the MipNeRF-360 loss head (mip360_losses) and compositing
(mip360_render_level / mip360_render_level_backward), for tests/test_mip360_loss_reference.py (CPU) and
tests/test_gpu_mip360_loss_edges.py (GPU).  The reference itself is oracle/mip360_oracle.py evaluated in float64 on the same
float32 inputs; this module only makes inputs and says how far a float32 evaluation may be from that reference.

Inputs (float32 arrays from a np.random.RandomState):
  grid_edges / dyadic_weights   the tie-laden family.  Edges are k/q, so equal neighbours (zero-width intervals) and NeRF edges
                                that sit exactly on a proposal edge are frequent -- where `>=` against `>` in the two-sided
                                searchsorted, or an off-by-one in the scatter j in [lo_i, hi_{i+1}), shows.  Weights are multiples
                                of 2^-bits with a row sum <= 1: every float32 cumulative sum is exact, so w_outer, the hinge
                                max(0, w - w_outer), its square (24 bits) and w + eps are exact, and so is every midpoint
                                difference of the distortion term.  A float32 evaluation then differs from float64 by the rounding
                                of one division and of sums of at most 64 same-signed terms: DYADIC_RTOL.
  general_edges / general_weights   continuous sorted edges, weights 0 or >= 2^-10.  Bounds per element, from the helpers below.

Bounds (float64, from the inputs only; u = 2^-24 is the unit roundoff of float32, K = 64 the length of a wave's float32 sum):
  interlevel_grad_bound, interlevel_loss_bound, distortion_grad_bound, compositing_grad_bound, rendering_grad_error, and
  rendering_backward_ratio, which applies the last two to an output of mip360_render_level_backward.
tests/test_mip360_loss_reference.py checks that the oracle evaluated in float32 stays inside every one of them."""
import numpy as np

from oracle import mip360_oracle as O

U = 2.0 ** -24                      # unit roundoff of float32
K = 64                              # length of the wave's float32 sums
TINY = 2.0 ** -126                  # smallest normal float32: what a flushed product can lose
DYADIC_RTOL = K * U                 # 3.8e-6
EPS = O.EPS32


def f64(a):
    return np.asarray(a, np.float64)


# ------------------------------------------------------------------------------------------------------------ inputs
def grid_edges(rs, n, S, q=64):
    """[n, S+1] sorted edges k/q.  Neighbours are tied on purpose (20 % of them below 16 intervals, where a draw of S+1 values out
    of q+1 seldom repeats; 10 % above) on top of the draw's own repeats; three rows of four run from 0 to 1, as a level's intervals do (rows 1, 5, 9, ... are
    left where they fell, partly or wholly outside the other level's range); row 0 starts with three edges at 0 and ends with three
    at 1 when S >= 6; row 1 (when there is one) has all its edges equal."""
    k = np.sort(rs.randint(0, q + 1, (n, S + 1)), -1)
    span = np.arange(n) % 4 != 1
    k[span, 0], k[span, -1] = 0, q
    tie = rs.rand(n, S + 1) < (0.2 if S < 16 else 0.1)
    tie[:, 0] = False
    first = np.maximum.accumulate(np.where(tie, 0, np.arange(S + 1)), -1)       # index of the first edge of every tied run
    k = np.take_along_axis(k, first, -1)
    if S >= 6:
        k[0, :3], k[0, -3:] = 0, q
    if n >= 2:
        k[1] = rs.randint(0, q + 1)
    return (k / float(q)).astype(np.float32)


def dyadic_weights(rs, n, S, bits=12, total=1.0):
    """[n, S] non-negative multiples of 2^-bits, row sum <= total <= 1 (and at least half of it, up to the flooring), about a third
    of the entries exactly 0, rows 2, 9, 16, ... all zero."""
    one = 1 << bits
    raw = rs.randint(1, one, (n, S)).astype(np.int64)
    raw[rs.rand(n, S) < 1.0 / 3] = 0
    target = rs.randint(int(one * total) // 2, int(one * total) + 1, (n, 1))
    m = raw * target // np.maximum(raw.sum(-1, keepdims=True), 1)
    m[2::7] = 0
    assert (m.sum(-1) <= one).all()
    return (m / float(one)).astype(np.float32)


def general_edges(rs, n, S):
    return np.sort(rs.rand(n, S + 1), -1).astype(np.float32)


def general_weights(rs, n, S):
    """[n, S] weights of a spiky softmax scaled to a row sum in [0.5, 1], a quarter of them set to 0, the rest 0 or >= 2^-10."""
    w = O.softmax(rs.randn(n, S) * 2) * rs.uniform(0.5, 1.0, (n, 1))
    w[rs.rand(n, S) < 0.25] = 0
    w = w.astype(np.float32)
    w[w < 2.0 ** -10] = 0
    return w


# ------------------------------------------------------------------------------------------------------------ loss head
def interlevel_grad_bound(t, w, t_env, w_env, eps=EPS):
    """How far a float32 evaluation of lossfun_outer (per interval: 'term') and of lossfun_outer_grad_w_env (per proposal bin:
    'grad') may be from float64.
      w_outer_i = cy[hi_{i+1}] - cy[lo_i], cy the sequential float32 cumulative sum: the roundings between the two indices, at most
        Sp of them of at most u cy_max each, and the subtraction's:             |D w_outer_i| <= (Sp + 1) u cy_max
        (0 where every covered weight is 0: the weights are 0 or >= 2^-10, so w_outer_i = 0 means a sum of zeros, which is exact)
      ex_i = max(0, w_i - w_outer_i): the hinge is 1-Lipschitz, and stays shut in every precision while w_outer_i - w_i is above
        its error:                                        |D ex_i| <= |D w_outer_i| if w_i - w_outer_i > -|D w_outer_i|, else 0
      go_i = -2 ex_i / (w_i + eps): then its own rounding, w + eps, the division and the factor 2 (exact):
                                                                               |D go_i| <= 2 |D ex_i| / (w_i + eps) + 4 u |go_i|
      term_i = ex_i^2 / (w_i + eps):                        |D term_i| <= (2 ex_i + D ex_i) D ex_i / (w_i + eps) + 4 u term_i
      grad_j = sum of go_i over the cover lo_i <= j < hi_{i+1}: D go_i scattered exactly as the gradient is, plus the roundings of
        a sum of at most Sn same-signed terms and of the scale factor:         + (Sn + 3) u sum_cover |go_i|
    The searchsorted decisions compare float32 inputs and are the same in every precision."""
    t, w, t_env, w_env = f64(t), f64(w), f64(t_env), f64(w_env)
    Sn, Sp = w.shape[-1], w_env.shape[-1]
    lo, hi = O.searchsorted(t_env, t)
    _, w_outer = O.inner_outer(t, t_env, w_env)
    ex = np.maximum(0, w - w_outer)
    go = 2 * ex / (w + eps)
    term = ex ** 2 / (w + eps)
    d_outer = np.where(w_outer == 0, 0.0, (Sp + 1) * U * w_env.sum(-1, keepdims=True))
    d_ex = np.where(w - w_outer > -d_outer, d_outer, 0.0)
    d_go = 2 * d_ex / (w + eps) + 4 * U * go
    d_term = (2 * ex + d_ex) * d_ex / (w + eps) + 4 * U * term
    j = np.arange(Sp)
    cover = (j >= lo[..., :-1, None]) & (j < hi[..., 1:, None])
    grad = np.sum((d_go + (Sn + 3) * U * go)[..., None] * cover, -2)
    return dict(term=d_term, grad=grad, term_value=term)


def interlevel_loss_bound(t, w, envs, eps=EPS):
    """Bound of interlevel_loss (mult 1) over the proposal levels `envs` = [(t_env, w_env), ...]: the terms' own bounds, the
    wave's sum of Sn <= K non-negative terms, the float32 accumulation over the levels and the scalar's final rounding."""
    n, Sn = np.shape(w)
    total = 0.0
    for t_env, w_env in envs:
        b = interlevel_grad_bound(t, w, t_env, w_env, eps)
        total += (b['term'].sum() + (K + len(envs) + 4) * U * b['term_value'].sum()) / (n * Sn)
    return total


def distortion_grad_bound(t, w):
    """How far a float32 evaluation of lossfun_distortion_grad_w ('grad', per interval) and of lossfun_distortion ('loss', per ray)
    may be from float64.  A midpoint ut = (t_i + t_{i+1}) / 2 carries u ut, so |ut_i - ut_j| carries u (ut_i + ut_j) + u |ut_i - ut_j|
    -- an absolute error: the difference cancels -- the product with w_j one more u, and the sum of Sn non-negative terms Sn u inner:
      |D inner_i| <= u (sum_j w_j (ut_i + ut_j) + (Sn + 2) inner_i);   grad_i = 2 inner_i + 2 w_i dt_i / 3: 2 D inner_i, four roundings
      in the second term, three in the scale;   loss = sum_i w_i inner_i + w_i^2 dt_i / 3: w_i D inner_i, then K + 8 roundings."""
    t, w = f64(t), f64(w)
    Sn = w.shape[-1]
    ut = (t[..., 1:] + t[..., :-1]) / 2
    dt = t[..., 1:] - t[..., :-1]
    inner = np.sum(w[..., None, :] * np.abs(ut[..., :, None] - ut[..., None, :]), -1)
    d_inner = U * (np.sum(w[..., None, :] * (ut[..., :, None] + ut[..., None, :]), -1) + (Sn + 2) * inner)
    intra = 2 * w * dt / 3
    grad = 2 * d_inner + 4 * U * intra + 3 * U * (2 * inner + intra)
    loss = np.sum(w * d_inner, -1) + (K + 8) * U * np.sum(w * inner + w ** 2 * dt / 3, -1)
    return dict(grad=grad, loss=loss)


# ------------------------------------------------------------------------------------------------------------ compositing
def _compositing_terms(density, tdist, dirs, opaque):
    density, tdist, dirs = f64(density), f64(tdist), f64(dirs)
    delta = (tdist[..., 1:] - tdist[..., :-1]) * np.linalg.norm(dirs[..., None, :], axis=-1)
    w, alpha, trans = O.compute_alpha_weights(density, tdist, dirs, opaque)
    dd = density * delta
    if opaque:
        dd = np.concatenate([dd[..., :-1], np.zeros_like(dd[..., -1:])], -1)     # the last sample's own exponent is not summed
    return delta, w, alpha, trans, np.cumsum(dd, -1)


def _suffix(a):
    """sum_{k>i} a_k"""
    return np.cumsum(a[..., ::-1], -1)[..., ::-1] - a


def compositing_grad_bound(density, tdist, dirs, gw, opaque, gw_err=None):
    """How far a float32 evaluation of g_density_i = (gw_i (1 - alpha_i) T_i - sum_{k>i} gw_k w_k) delta_i
    (alpha_weights_backward) may be from float64, with X_i = sum_{j<=i} density_j delta_j:
      the exponent of T_i and of 1 - alpha_i is a float32 sum of at most K terms, K u X_i off, which exp turns into a relative
        error; with the roundings of exp, the products and the suffix sum:    K u (1 + X_i) on gw_i (1 - alpha_i) T_i
      1 - alpha_i is taken from the stored alpha_i = 1 - exp(-x_i), which is rounded next to 1:   + u |gw_i| T_i
      a suffix sum taken as an inclusive sum less its own term (numpy's; the kernel's scan is shifted):   + K u |gw_i| w_i
      w_k = alpha_k T_k carries T_k's relative error and, from alpha_k = 1 - exp(-x_k) (exp rounds to u next to 1), u T_k in
        absolute terms -- which is what counts where x_k << 1:                 |gw_k| (K u (1 + X_k) w_k + u T_k) in the suffix sum
      gw_err (optional): an absolute error already on gw (rendering_grad_error), carried through the same linear map
      a product below the smallest normal float32 may be flushed:              2^-126 (|gw_i| + sum_{k>i} |gw_k| + S + 2)
    all times delta_i."""
    delta, w, alpha, trans, X = _compositing_terms(density, tdist, dirs, opaque)
    a = np.abs(f64(gw))
    S = a.shape[-1]
    own = a * (1 - alpha) * trans
    rel = K * U * (1 + X)
    b = rel * own + U * a * trans + K * U * a * w + _suffix(a * (rel * w + U * trans))
    if gw_err is not None:
        b = b + gw_err * (1 - alpha) * trans + _suffix(gw_err * w)
    b = b + TINY * (a + _suffix(a) + S + 2)
    if opaque:
        b[..., -1] = 0                                                           # x_last = inf: the gradient is exactly 0
    return b * delta + TINY


def rendering_grad_error(density, rgbs, tdist, dirs, bg, opaque, g_rgb=None, g_distance_mean=None):
    """Absolute float32 error of the gradient volumetric_rendering_backward hands to the weights (before compositing), from the
    inputs.  rgb part sum_c g_c (c_c - bg): seven roundings of a three-term sum of products.  distance_mean part
    g e (log t_i - E dB) / B, B = max(eps, acc), E = A / B, A = sum_k w_k log t_k:
      D A <= u sum_k (K (1 + X_k) w_k + T_k) |log t_k| (the weights' errors, compositing_grad_bound) + (K + 2) u sum_k w_k |log t_k|
      D E <= D A / B + K u |E| (B is a wave sum when it is acc, exactly eps below it) =: u eE;  e = exp(E) carries (eE + 2) u
      relative;  the difference log t_i - E cancels, so its error counts against |log t_i| + |E|:
      |D gw_i| <= u |g| e / B ((eE + K + 4) (|log t_i| + |E|) + eE)."""
    delta, w, alpha, trans, X = _compositing_terms(density, tdist, dirs, opaque)
    err = np.zeros_like(w)
    if g_rgb is not None:
        err = err + 7 * U * np.sum(np.abs(f64(g_rgb))[..., None, :] * (np.abs(f64(rgbs)) + abs(bg)), -1)
    if g_distance_mean is not None:
        t = f64(tdist)
        logt = np.log(0.5 * (t[..., :-1] + t[..., 1:]))
        acc = w.sum(-1, keepdims=True)
        B = np.maximum(EPS, acc)
        A = (w * logt).sum(-1, keepdims=True)
        E = A / B
        eE = (np.sum((K * (1 + X) * w + trans) * np.abs(logt), -1, keepdims=True)
              + (K + 2) * np.sum(w * np.abs(logt), -1, keepdims=True)) / B + K * np.abs(E)
        e = np.exp(E)
        inside = (e > t[..., :1]) & (e < t[..., -1:])
        g = np.abs(f64(g_distance_mean))[..., None]
        err = err + U * g * inside * e / B * ((eE + K + 4) * (np.abs(logt) + np.abs(E)) + eE)
    return err


def rendering_backward(density, rgbs, tdist, dirs, bg, opaque, g_weights=None, g_rgb=None, g_distance_mean=None):
    """The float64 closed forms chained as mip360_render_level_backward chains them: volumetric_rendering_backward's gradient to the
    weights, plus g_weights, through alpha_weights_backward.  Inputs in any precision (float32 inputs give the float32 evaluation).
    Returns (g_density, g_rgb_samples or None, the gradient handed to the weights)."""
    w = O.compute_alpha_weights(density, tdist, dirs, opaque)[0]
    gw, g_rgbs = O.volumetric_rendering_backward(rgbs, w, tdist, bg, g_rgb=g_rgb, g_distance_mean=g_distance_mean)
    if g_weights is not None:
        gw = gw + g_weights
    return O.alpha_weights_backward(density, tdist, dirs, gw, opaque), g_rgbs, gw


def rendering_backward_ratio(got, density, rgbs, tdist, dirs, bg, opaque, g_weights=None, g_rgb=None, g_distance_mean=None):
    """|got - float64 g_density| / bound per element (<= 1 everywhere is the check), the float64 g_density and the bound.
    One decision of the closed form is not continuous: the background's share of rgb, max(0, 1 - acc) bg, hands -bg sum_c g_c to
    every weight of a ray while 1 - acc > 0.  A float32 acc within its own error of 1 -- every opaque ray -- may decide either way
    (on an opaque ray the two differ by the constant times T_end = 0, in exact arithmetic), so on such a ray the output may be
    within the bound of either branch, the same one for the whole ray.
      |D acc| <= u sum_k (K (1 + X_k) w_k + T_k) + K u acc   (the weights' errors, then the wave's sum)"""
    d64, t64, r64 = f64(density), f64(tdist), f64(dirs)
    g64 = lambda a: None if a is None else f64(a)
    want, _, gw = rendering_backward(d64, None if rgbs is None else f64(rgbs), t64, r64, float(bg), opaque, g64(g_weights), g64(g_rgb),
                                     g64(g_distance_mean))
    err = rendering_grad_error(density, rgbs, tdist, dirs, bg, opaque, g_rgb=g_rgb, g_distance_mean=g_distance_mean)
    bound = compositing_grad_bound(density, tdist, dirs, gw, opaque, err)
    ratio = np.abs(got - want) / bound
    if g_rgb is not None and bg != 0:
        _, w, _, trans, X = _compositing_terms(density, tdist, dirs, opaque)
        acc = w.sum(-1)
        ambiguous = np.abs(1 - acc) <= U * np.sum(K * (1 + X) * w + trans, -1) + K * U * acc
        shift = np.where(1 - acc > 0, 1.0, -1.0) * float(bg) * f64(g_rgb).sum(-1)       # to the other branch
        gw_alt = gw + shift[..., None]
        want_alt = O.alpha_weights_backward(d64, t64, r64, gw_alt, opaque)
        bound_alt = compositing_grad_bound(density, tdist, dirs, gw_alt, opaque, err)
        ratio_alt = np.abs(got - want_alt) / bound_alt
        use = (ambiguous & (ratio_alt.max(-1) < ratio.max(-1)))[..., None]
        ratio, want, bound = np.where(use, ratio_alt, ratio), np.where(use, want_alt, want), np.where(use, bound_alt, bound)
    return ratio, want, bound


# ------------------------------------------------------------------------------------------------------------ cases
LOSS_SIZES = [(1, 1), (2, 63), (33, 7), (63, 2), (64, 64), (32, 64), (64, 1)]          # (Sn, Sp): 1, the wave's 64, 63, ragged
COMPOSITING_FAMILIES = ('plain', 'zero_width', 'zero_density', 'saturating', 'wide')


def loss_case(rs, family, n, Sn, Sp, n_prop):
    """Edges and weights of the NeRF level and of n_prop proposal levels: family 'dyadic' or 'general'.  The dyadic proposal rows
    sum to at most Sp / (2 Sn), between 1/64 and 1/2, so that the hinge w - w_outer > 0 is active on a good part of the intervals
    whatever the two levels' sizes."""
    edges, weights = (grid_edges, dyadic_weights) if family == 'dyadic' else (general_edges, general_weights)
    kw = dict(total=min(0.5, max(1.0 / 64, 0.5 * Sp / Sn))) if family == 'dyadic' else {}
    return dict(sd_n=edges(rs, n, Sn), w_n=weights(rs, n, Sn), sd_p=[edges(rs, n, Sp) for _ in range(n_prop)],
                w_p=[weights(rs, n, Sp, **kw) for _ in range(n_prop)])


def compositing_case(rs, family, n, S):
    """density [n,S], rgbs [n,S,3], tdist [n,S+1], dirs [n,3] (float32).  'plain': the family of tests/test_gpu_mip360.py;
    'zero_width': a third of the intervals have equal ends; 'zero_density'; 'saturating': sample S // 3 has density * delta = 60,
    ordinary ones follow; 'wide': the reciprocal warp of sorted s in [0, 1] between near 0.2 and far 1e6, both ends included."""
    density = np.exp(rs.randn(n, S)).astype(np.float32)
    rgbs = rs.rand(n, S, 3).astype(np.float32)
    steps = np.exp(rs.randn(n, S + 1) * 0.5) * 0.1
    dirs = rs.randn(n, 3).astype(np.float32)
    if family == 'zero_width':
        steps[:, 1:][rs.rand(n, S) < 0.35] = 0
    tdist = (0.2 + np.cumsum(steps, -1)).astype(np.float32)
    if family == 'wide':
        s = np.sort(rs.rand(n, S + 1), -1)
        s[:, 0], s[:, -1] = 0, 1
        tdist = (1 / (s / 1e6 + (1 - s) / 0.2)).astype(np.float32)
    if family == 'zero_density':
        density[:] = 0
    if family == 'saturating':
        j = S // 3
        delta = (f64(tdist[:, j + 1]) - f64(tdist[:, j])) * np.linalg.norm(f64(dirs), axis=-1)
        density[:, j] = (60 / delta).astype(np.float32)
    assert family in COMPOSITING_FAMILIES
    return density, rgbs, tdist, dirs

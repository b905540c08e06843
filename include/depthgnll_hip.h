/* depthgnll_hip.h -- C ABI of libdepthgnll_hip.so: the uncertainty-aware Gaussian negative-log-likelihood depth loss ('gnll') of
 * both training paths on the MI355X (gfx950).  The loss of Dense Depth Priors for NeRF (Roessle et al.): the prior is a per-pixel
 * mean p and standard deviation sigma, the rendered depth is a Gaussian whose variance is the spread of the ray's weights, and a
 * ray is penalised only while its rendering lies outside what the prior expects.  The definition is DESIGN.md 9.9 and, as
 * executable code, tests/depth_gnll_reference.py.
 *
 *   per ray r and level l, with samples x_s, weights w_s (s < S_l), the rendered depth D, the prior p, sigma and the bound lim:
 *   m    = p > 0 and sigma > 0 and (lim is null or p < lim)                     supervised
 *   M0   = sum w_s,  M1 = sum w_s x_s
 *   V    = sum w_s (x_s - D)^2 + 1e-5                                           rendered variance
 *   gate = m and (|D - p| - sigma > 0 or sigma^2 < V)                           outside the expected distribution
 *   Vc   = max(V, 1e-3)
 *   l_r  = 0.5 (log Vc + (D - p)^2 / Vc)
 *   value_l = (1 / n) sum over gated rays of l_r                                (n = all rays of the batch; may be negative)
 *   gV   = 0.5 (1 / Vc - (D - p)^2 / Vc^2)       (the clamp changes the value only: the gradient passes through it to V)
 *   d value / d D   = gate [ (D - p) / Vc - 2 gV (M1 - D M0) ] / n
 *   d value / d w_s = gate gV (x_s - D)^2 / n
 * The gate is a constant for the gradient and positions receive none.  D is an input, not recomputed as M1.
 *
 * Conventions as in depthssi_hip.h: plain C, raw DEVICE pointers, a `void* stream` (hipStream_t), return DEPTHGNLL_OK or an
 * error code with depthgnll_last_error(); the library is stateless and the caller owns every buffer.  The `*_bytes` query and
 * every argument check touch no HIP call and work on a host without a GPU.  Every call only enqueues.
 *
 * Arithmetic: every sum, V, the gate, l_r and both gradients in float64 from the float32 inputs, no implicit fma; one rounding
 * to float32 on the way out (a gradient entry is float32(float64(entry) + scale * gradient)).  No atomics: a ray's sums are
 * per-lane partials added by a fixed tree, a gradient entry is owned by one thread, the rays are summed in a fixed order, and
 * every tree depends on the shapes alone, so equal inputs give equal bits.
 */
#ifndef DEPTHGNLL_HIP_H
#define DEPTHGNLL_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DEPTHGNLL_ABI_VERSION 1
#define DEPTHGNLL_OK 0
#define DEPTHGNLL_ERR_ARG 1
#define DEPTHGNLL_ERR_HIP 2

#define DEPTHGNLL_MAX_RAYS (1 << 20)  /* a training batch */
#define DEPTHGNLL_MAX_LEVELS 8
#define DEPTHGNLL_MAX_SAMPLES 1024    /* per ray and level */

#define DEPTHGNLL_STATS_ROW 3         /* stats [n_levels, 3] float32: supervised rays, gated rays, gated rays with V < 1e-3 */

const char* depthgnll_last_error(void);
int depthgnll_abi_version(void);

/* Bytes of the workspace of depthgnll_levels (aligned to 256 by the caller).  -1 with a message for n_levels outside 1 .. 8 or n
 * outside 1 .. 2^20. */
int64_t depthgnll_workspace_bytes(int n_levels, int n);

/* The loss of n_levels renderings against one prior (p, sigma) [n], all levels of a step in one call (two launches).
 *   n_samples   : HOST array [n_levels], S_l in 1 .. 1024 (may differ per level)
 *   w           : HOST array [n_levels] of device pointers, w[l] [n, S_l]
 *   x           : HOST array [n_levels] of device pointers; x_is_edges 0: x[l] [n, S_l] sample positions; 1: x[l] [n, S_l + 1]
 *                 interval edges t, the position is 0.5f * (t[s] + t[s + 1]) formed in float32 as written
 *   d           : HOST array [n_levels] of device pointers, d[l] [n] the rendered depth
 *   p, sigma    : [n] the prior's mean and standard deviation; limit: [n] or null
 *   scale       : HOST array [n_levels], the levels' weights, or null: 1 each
 *   g_w, g_d    : HOST arrays [n_levels] of device pointers [n, S_l] / [n] (the arrays or single entries may be null).
 *                 scale[l] * gradient is ACCUMULATED; entries of rays that are not gated keep their bits (g_d[l][r] and the
 *                 whole row g_w[l][r, :])
 *   values      : [n_levels] float32, written
 *   stats       : [n_levels, 3] float32 as above, written
 *   fold_*      : each null or one float32 the second launch updates on the same stream:
 *                 *fold_total  += sum_l scale[l] * values[l]   (float32, level order, summed from 0 and then added)
 *                 *fold_last    = values[n_levels - 1]
 *                 *fold_others  = sum of the other levels' values (float32, level order)
 *                 *fold_n_sup   = the number of supervised rays
 * n outside 1 .. 2^20, n_levels outside 1 .. 8, a sample count outside 1 .. 1024 and x_is_edges other than 0 / 1 are errors. */
int depthgnll_levels(void* stream, int n, int n_levels, const int* n_samples, int x_is_edges, const float* const* w,
                     const float* const* x, const float* const* d, const float* p, const float* sigma, const float* limit,
                     const float* scale, float* const* g_w, float* const* g_d, void* workspace, float* values, float* stats,
                     float* fold_total, float* fold_last, float* fold_others, float* fold_n_sup);

#ifdef __cplusplus
}
#endif
#endif

/* depthguide_hip.h -- C ABI of libdepthguide_hip.so: depth-guided fine sampling of the NeRF++ path on the MI355X (gfx950).  G of a
 * cascade level's new foreground depths are drawn from a truncated Gaussian around the depth prior (Roessle et al., Dense Depth
 * Priors for NeRF) -- or, where a ray has no prior, around the depth and spread the previous level rendered -- and merged into the
 * ascending depths the existing fine sampling produced.  The definition is DESIGN.md 9.12 and, as executable code,
 * tests/depth_guide_reference.py.
 *
 *   per ray r: zp[S_prev], wp[S_prev] the previous level's foreground depths and weights; zin[S_in] the output of the existing fine
 *   sampling; lo_r, hi_r the ray's near and far bound; p_r the prior (0 = none), s_r its standard deviation (prior_std[r], or the
 *   constant std_const where prior_std is null); v[G] uniforms in [0, 1).  max(a, b) below is  a < b ? b : a  (a NaN a stays).
 *   s_eff  = max(s_r, min_std)
 *   guided = p_r > 0 and p_r < hi_r and s_eff > 0 and s_eff < inf                                  (a NaN compares false)
 *   mode 0 (guided):  mu = p_r, sd = s_eff
 *   else  W = sum wp
 *         mode 1 (W > 1e-10):  mu = sum(wp zp) / W,  sd = max(sqrt(sum(wp (zp - mu)^2) / W), min_std)
 *         mode 2 (otherwise):  no Gaussian
 *   q_j = (j + v_j) / G                                          j = 0 .. G-1
 *   modes 0, 1:  t = q_j K;  i = min(int(t), K - 1);  f = t - i;  x = T[i] + f (T[i+1] - T[i]);  g_j = min(max(mu + sd x, lo_r), hi_r)
 *   mode 2:      g_j = lo_r + (hi_r - lo_r) q_j
 *   z_merged[r] = sort(cat(zin[r], float32(g)))                  values only, [S_in + G]; NaNs last
 * T [K + 1] (K = DEPTHGUIDE_TABLE_K) is the caller's table of the standard normal's inverse CDF truncated at +-3 sigma,
 * T[i] = Phi^-1(Phi(-3) + (Phi(3) - Phi(-3)) i / K), float64 on the device; the kernel multiplies, adds and compares on it.
 *
 * The uniforms: use_rng != 0: v_j = the Philox4x32-10 uniform of (seed, step), stream 5, element r G + j (the generator of
 * libnerfpp_hip.so, csrc/nerfpp_common.h); else v [n, G] where it is not null; else 0.5 (deterministic, for rendering).
 *
 * Conventions as in rayreg_hip.h: plain C, raw DEVICE pointers, a `void* stream` (hipStream_t), return DEPTHGUIDE_OK or an error
 * code with depthguide_last_error(); the library is stateless and the caller owns every buffer.  Every argument check touches no
 * HIP call and works on a host without a GPU.  The call only enqueues (one launch).
 *
 * Arithmetic: float64 from the float32 inputs on, no implicit fma, one rounding to float32 on the way out.  No atomics; the sums over
 * the previous level's samples are fixed trees of S_prev alone (lane l adds samples l, l + 64, ... in ascending order, the 64 lanes
 * by the xor butterfly), so equal inputs give equal bits.
 */
#ifndef DEPTHGUIDE_HIP_H
#define DEPTHGUIDE_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DEPTHGUIDE_ABI_VERSION 1
#define DEPTHGUIDE_OK 0
#define DEPTHGUIDE_ERR_ARG 1
#define DEPTHGUIDE_ERR_HIP 2

#define DEPTHGUIDE_MAX_RAYS (1 << 20)  /* a training batch or a render chunk */
#define DEPTHGUIDE_MAX_PREV 1024       /* S_prev */
#define DEPTHGUIDE_MAX_MERGED 512      /* S_in + G */
#define DEPTHGUIDE_TABLE_K 1024        /* the table has K + 1 entries */
#define DEPTHGUIDE_RNG_STREAM 5        /* Philox stream id of the uniforms */

const char* depthguide_last_error(void);
int depthguide_abi_version(void);

/* The G guided depths of every ray, merged into zin.
 *   n                : rays, 1 .. 2^20
 *   S_prev           : samples of the previous level, 1 .. 1024
 *   S_in, G          : at least 1 each, S_in + G <= 512
 *   zp, wp           : [n, S_prev]
 *   zin              : [n, S_in]; ascending rows are merged, any other row is sorted with the new depths
 *   lo, hi           : [n]
 *   prior            : [n] or null (no ray has a prior)
 *   prior_std        : [n] or null (every ray has std_const)
 *   std_const        : read where prior_std is null; any value (one that is not positive and finite guides no ray)
 *   min_std          : finite, not negative
 *   table            : [DEPTHGUIDE_TABLE_K + 1] float64, aligned to 8 bytes
 *   v                : [n, G] or null
 *   use_rng, seed, step : as above; use_rng != 0 with a non-null v is refused
 *   z_merged         : [n, S_in + G], written; apart from zin
 *   mode             : [n] int32, written: 0, 1 or 2
 *   guide            : [n, G] or null; written: float32(g) in the order of j */
int depthguide_merge(void* stream, int n, int S_prev, int S_in, int G, const float* zp, const float* wp, const float* zin,
                     const float* lo, const float* hi, const float* prior, const float* prior_std, double std_const, double min_std,
                     const double* table, const float* v, int use_rng, uint64_t seed, uint64_t step, float* z_merged, int32_t* mode,
                     float* guide);

#ifdef __cplusplus
}
#endif
#endif

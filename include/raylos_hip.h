/* raylos_hip.h -- C ABI of libraylos_hip.so: Urban Radiance Fields' line-of-sight term on the foreground weights of one cascade
 * level of the NeRF++ training path, on the MI355X (gfx950).  It empties the space in front of a measured surface and concentrates
 * the weight in a band around it; the expected-depth losses see one number per ray and cannot do either.  The definition is
 * DESIGN.md 9.13 and, as executable code, tests/ray_los_reference.py.
 *
 *   per ray r with S samples: ascending positions z_s, weights w_s (s < S), far bound hi_r, prior p_r (scene units, 0 = none),
 *   half-width sigma_r (scene units); all float32
 *   e_s      = z_s  s < S,   e_S = hi_r                            a weight is the mass of the interval [e_s, e_{s+1}]
 *   m_r      = p_r > 0  and  p_r < hi_r  and  sigma_r > 0          supervised (kl's and gnll's mask, plus sigma)
 *   lo_b     = float32(p_r - sigma_r),  hi_b = float32(p_r + sigma_r)      one float32 rounding each, as written
 *   empty_s  = e_{s+1} <= lo_b                                     the whole interval lies in front of the band
 *   near_s   = not empty_s  and  e_s < hi_b                        the interval touches the band
 *                                                                  (otherwise behind the band: no term)
 *   k_s      = Phi((e_{s+1} - p_r) / (sigma_r / 3)) - Phi((e_s - p_r) / (sigma_r / 3))
 *              Phi(x) = 0.5 (1 + erf(x / sqrt 2)), float64: URF's kernel N(p, (sigma/3)^2), integrated over the interval
 *   L_r      = sum_s near_s (w_s - k_s)^2 + sum_s empty_s w_s^2
 *   value    = (1/n) sum_r m_r L_r                                 n = all rays of the batch
 *   d value / d w_s = m_r (near_s 2 (w_s - k_s) + empty_s 2 w_s) / n
 *   front_r  = sum_s empty_s w_s                                   the mass in front of the band (reported, not trained)
 *   stats    = [ number of supervised rays,  sum_r m_r front_r ]
 *   g_w[r,s] = float32( float64(g_w[r,s]) + lambda * d value / d w_s )     where the sample has a term
 *   *fold_total += float32(lambda * value)
 * The comparisons are float32, as written.  Positions, p and sigma receive no gradient.  k_s is evaluated only for near intervals.
 * The row of g_w of an unsupervised ray, and an entry behind the band, keep their bits.
 *
 * Conventions as in rayreg_hip.h: plain C, raw DEVICE pointers, a `void* stream` (hipStream_t), return RAYLOS_OK or an error code
 * with raylos_last_error(); the library is stateless and the caller owns every buffer.  The `*_bytes` query and every argument
 * check touch no HIP call and work on a host without a GPU.  Every call only enqueues.
 *
 * Arithmetic: float64 from the float32 inputs on (the comparisons and the band's two bounds excepted), no implicit fma; one rounding
 * to float32 on the way out.  No atomics: a gradient entry is owned by one lane, a ray's sums are fixed shuffle trees, the rays are
 * summed in a fixed order, and every tree depends on n and S alone, so equal inputs give equal bits.
 */
#ifndef RAYLOS_HIP_H
#define RAYLOS_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RAYLOS_ABI_VERSION 1
#define RAYLOS_OK 0
#define RAYLOS_ERR_ARG 1
#define RAYLOS_ERR_HIP 2

#define RAYLOS_MAX_RAYS (1 << 20)  /* a training batch */
#define RAYLOS_MAX_SAMPLES 1024    /* per ray */

const char* raylos_last_error(void);
int raylos_abi_version(void);

/* Bytes of the workspace of raylos_level (a multiple of 256).  -1 with a message for n outside 1 .. 2^20. */
int64_t raylos_workspace_bytes(int n);

/* The line-of-sight term of one level (two launches).
 *   n, S        : rays (1 .. 2^20) and samples per ray (1 .. 1024)
 *   w, z        : [n, S] the weights and the ascending sample positions
 *   hi, p, sigma: [n] the rays' far bounds, priors and half-widths of the band
 *   lambda      : finite and positive
 *   g_w         : [n, S] or null (values only); the scaled gradient is ACCUMULATED as above
 *   workspace   : raylos_workspace_bytes(n) bytes aligned to 256
 *   values      : [1] float32, written: the mean line-of-sight term
 *   stats       : [2] float32, written: the number of supervised rays and their summed mass in front of the band
 *   fold_total  : null or one float32 the second launch updates on the same stream as above */
int raylos_level(void* stream, int n, int S, const float* w, const float* z, const float* hi, const float* p,
                 const float* sigma, double lambda, float* g_w, void* workspace, float* values, float* stats,
                 float* fold_total);

#ifdef __cplusplus
}
#endif
#endif

/* rayreg_hip.h -- C ABI of librayreg_hip.so: the two regularisers of the NeRF++ training path on the weights along a ray, on the
 * MI355X (gfx950).  A distortion loss (MipNeRF-360's, in prefix-sum form, on interval edges normalised to [lo, hi]) and an opacity
 * entropy -o log o, both on the foreground weights of one cascade level.  They constrain where weight sits on a ray on which no
 * depth prior speaks.  The definition is DESIGN.md 9.11 and, as executable code, tests/ray_reg_reference.py.
 *
 *   per ray r with S samples: ascending positions z_s, weights w_s (s < S), the ray's near bound lo_r and far bound hi_r
 *   valid_r = hi_r > lo_r                                                       (else the ray gets no distortion term)
 *   e_s     = (z_s - lo_r) / (hi_r - lo_r)  s < S,   e_S = (hi_r - lo_r) / (hi_r - lo_r)        normalised interval edges
 *   u_s     = (e_s + e_{s+1}) / 2,   d_s = e_{s+1} - e_s
 *   A_s = sum_{j<s} w_j,  B_s = sum_{j<s} w_j u_j,   A'_s, B'_s: the same over j > s
 *   dist_r  = 2 sum_s w_s (u_s A_s - B_s) + (1/3) sum_s w_s^2 d_s               (= sum_ij w_i w_j |u_i - u_j| + (1/3) sum w^2 d)
 *   d dist_r / d w_s = 2 [u_s (A_s - A'_s) - (B_s - B'_s)] + (2/3) w_s d_s
 *   o_r     = sum_s w_s + 1e-10,   opac_r = -o_r log o_r,   d opac_r / d w_s = -(log o_r + 1)
 *   values  = [ (1/n) sum_{valid r} dist_r ,  (1/n) sum_r opac_r ]              (n = all rays of the batch)
 *   g_w[r,s] = float32( float64(g_w[r,s]) + (lambda_dist * valid_r * d dist_r/d w_s + lambda_opac * d opac_r/d w_s) / n )
 *   *fold_total += float32(lambda_dist * values[0] + lambda_opac * values[1])
 *   stats   = [ number of valid rays ]
 * Positions receive no gradient.  A lambda of 0 removes its term: its value is written as 0 and nothing of it is evaluated.  A row
 * of g_w that receives no term (an invalid ray while lambda_opac = 0) keeps its bits.
 *
 * Conventions as in depthgnll_hip.h: plain C, raw DEVICE pointers, a `void* stream` (hipStream_t), return RAYREG_OK or an error code
 * with rayreg_last_error(); the library is stateless and the caller owns every buffer.  The `*_bytes` query and every argument
 * check touch no HIP call and work on a host without a GPU.  Every call only enqueues.
 *
 * Arithmetic: float64 from the float32 inputs on, no implicit fma; one rounding to float32 on the way out.  No atomics: a lane owns
 * a contiguous run of a ray's samples, the lanes' totals are scanned by fixed shuffle trees, a gradient entry is owned by one lane,
 * the rays are summed in a fixed order, and every tree depends on n and S alone, so equal inputs give equal bits.
 */
#ifndef RAYREG_HIP_H
#define RAYREG_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RAYREG_ABI_VERSION 1
#define RAYREG_OK 0
#define RAYREG_ERR_ARG 1
#define RAYREG_ERR_HIP 2

#define RAYREG_MAX_RAYS (1 << 20)  /* a training batch */
#define RAYREG_MAX_SAMPLES 1024    /* per ray */

const char* rayreg_last_error(void);
int rayreg_abi_version(void);

/* Bytes of the workspace of rayreg_level (a multiple of 256).  -1 with a message for n outside 1 .. 2^20. */
int64_t rayreg_workspace_bytes(int n);

/* Both regularisers of one level (two launches).
 *   n, S        : rays (1 .. 2^20) and samples per ray (1 .. 1024)
 *   w, z        : [n, S] the weights and the ascending sample positions
 *   lo, hi      : [n] the rays' bounds
 *   lambda_*    : finite and not negative, at least one positive
 *   g_w         : [n, S] or null (values only); the scaled gradient is ACCUMULATED as above
 *   workspace   : rayreg_workspace_bytes(n) bytes aligned to 256
 *   values      : [2] float32, written: the mean distortion and the mean opacity entropy (0 for a lambda of 0)
 *   stats       : [1] float32, written: the number of valid rays
 *   fold_total  : null or one float32 the second launch updates on the same stream as above */
int rayreg_level(void* stream, int n, int S, const float* w, const float* z, const float* lo, const float* hi, double lambda_dist,
                 double lambda_opac, float* g_w, void* workspace, float* values, float* stats, float* fold_total);

#ifdef __cplusplus
}
#endif
#endif

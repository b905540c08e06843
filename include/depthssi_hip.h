/* depthssi_hip.h -- C ABI of libdepthssi_hip.so: the scale-and-shift-invariant depth loss ('ssi') of both training paths on the
 * MI355X (gfx950).  A relative-depth prior (monocular depth) is known up to one scale and one shift per image; per group of rays
 * (= image) the loss fits the scale w and shift q that best map the rendered depth onto the prior in the least-squares sense and
 * penalises what is left.  The definition is DESIGN.md 9.8 and, as executable code, tests/depth_ssi_reference.py.
 *
 *   m_i = p_i > 0 and 0 <= g_i < n_groups                         (a ray outside the groups counts as unsupervised)
 *   per group k over its supervised rays:  N = sum 1, Sd = sum d, Sdd = sum d^2, Sp = sum p, Sdp = sum d p
 *   fitted  iff  N >= min_rays  and  N Sdd - Sd^2 > 1e-8 N Sdd   (the rendered depth is not constant in the group)
 *   w = (N Sdp - Sd Sp) / (N Sdd - Sd^2),  q = (Sp - w Sd) / N,  r_i = w d_i + q - p_i
 *   L = (1 / D) sum over fitted groups, over their supervised rays, of r_i^2;   dL/dd_i = 2 w r_i / D   (w and q minimise the
 *   sum, so their derivatives drop out).  D = n (DEPTHSSI_NORM_ALL) or max(N_sup, 1) (DEPTHSSI_NORM_SUPERVISED), N_sup = sum m.
 *
 * Conventions as in depthmetrics_hip.h: plain C, raw DEVICE pointers, a `void* stream` (hipStream_t), return DEPTHSSI_OK or an
 * error code with depthssi_last_error(); the library is stateless and the caller owns every buffer.  The `*_bytes` query and
 * every argument check touch no HIP call and work on a host without a GPU.  Every call only enqueues.
 *
 * Arithmetic: every sum, the solve, the residual and the gradient in float64 from the float32 inputs, no implicit fma; one
 * rounding to float32 on the way out (a gradient entry is float32(float64(entry) + scale * gradient)).  No atomics: a group's
 * sums are per-thread partials added by fixed trees, a gradient entry is owned by one thread of one workgroup, and both trees
 * depend on the shapes alone, so equal inputs give equal bits.
 */
#ifndef DEPTHSSI_HIP_H
#define DEPTHSSI_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DEPTHSSI_ABI_VERSION 1
#define DEPTHSSI_OK 0
#define DEPTHSSI_ERR_ARG 1
#define DEPTHSSI_ERR_HIP 2

#define DEPTHSSI_MAX_RAYS (1 << 20)   /* a training batch: every group's workgroup reads all n rays */
#define DEPTHSSI_MAX_GROUPS 65535
#define DEPTHSSI_MAX_LEVELS 8

#define DEPTHSSI_NORM_ALL 0           /* D = n */
#define DEPTHSSI_NORM_SUPERVISED 1    /* D = max(N_sup, 1) */

#define DEPTHSSI_FIT_ROW 4            /* fit [n_levels, n_groups, 4] float32: w, q, N, fitted (0 / 1); w = q = 0 when not fitted */
#define DEPTHSSI_STATS_ROW 2          /* stats [n_levels, 2] float32: supervised rays, supervised rays in fitted groups */

const char* depthssi_last_error(void);
int depthssi_abi_version(void);

/* Bytes of the workspace of depthssi_levels (aligned to 256 by the caller).  -1 with a message for n_levels outside 1 .. 8 or
 * n_groups outside 1 .. 65535. */
int64_t depthssi_workspace_bytes(int n_levels, int n_groups);

/* The loss of n_levels rendered depths d[l] [n] against one prior p [n], all levels of a step in one call (two launches).
 *   g, g_stride : group id of ray i at g[i * g_stride] (int32; g_stride 3 reads the frame column of a [n, 3] pixel table in
 *                 place), or null: one group (n_groups must be 1 then)
 *   scale       : HOST array [n_levels], the levels' weights
 *   grads       : HOST array [n_levels] of device pointers [n] (entries may be null), or null.  scale[l] * dL/dd is ACCUMULATED;
 *                 entries of rays that are unsupervised or in a group that is not fitted are not touched
 *   values      : [n_levels] float32, written
 *   fit, stats  : as above, written
 *   fold_*      : each null or one float32 the second launch updates on the same stream:
 *                 *fold_total  += sum_l scale[l] * values[l]   (float32, level order, summed from 0 and then added)
 *                 *fold_last    = values[n_levels - 1]
 *                 *fold_others  = sum of the other levels' values (float32, level order)
 *                 *fold_n_sup   = N_sup
 * n outside 1 .. 2^20, n_groups outside 1 .. 65535, n_levels outside 1 .. 8, min_rays < 1 and an unknown norm are errors. */
int depthssi_levels(void* stream, int n, int n_levels, const float* const* d, const float* p, const int32_t* g, int g_stride,
                    int n_groups, int min_rays, int norm, const float* scale, float* const* grads, void* workspace, float* values,
                    float* fit, float* stats, float* fold_total, float* fold_last, float* fold_others, float* fold_n_sup);

#ifdef __cplusplus
}
#endif
#endif

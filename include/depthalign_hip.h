/* depthalign_hip.h -- C ABI of libdepthalign_hip.so: aligning relative depth priors to sparse metric depth on the MI355X (gfx950).
 * A monocular prior is known up to one scale and one shift per image; each frame's (s, b) is fitted once, robustly, against the few
 * metric measurements the frame has (the anchor), and applied to every pixel of the prior.  The definition is DESIGN.md 8.9 and, as
 * executable code, tests/depth_align_reference.py.
 *
 * Conventions as in depthacc_hip.h: plain C, raw DEVICE pointers, a `void* stream` (hipStream_t), return DEPTHALIGN_OK or an error
 * code with depthalign_last_error(); the library is stateless and the caller owns every buffer.  The `*_bytes` query and every
 * argument check touch no HIP call and work on a host without a GPU.  Every call only enqueues.
 *
 * The definition.  prior p and anchor a are float32 [n_frames, height, width]; a value is valid iff > 0 (0, negatives and NaN are
 * not).  space DEPTH: target t = a, model z = s p + b.  space DISPARITY: the prior is relative inverse depth, t = 1.0 / a in float64,
 * model 1 / z = s p + b.  Everything inside is IEEE float64 on the exactly widened inputs, no implicit fma.  Per frame, over the pairs
 * (x_i = p_i, t_i) of the pixels with p > 0 and a > 0, starting from w_i = 1, for k = 0 .. iters:
 *     Sw = sum w, Sx = sum w x, St = sum w t, Sxx = sum (w x) x, Sxt = sum (w x) t;   den = Sw Sxx - Sx Sx
 *     degenerate unless den > (1e-8 Sw) Sxx;   s = (Sw Sxt - Sx St) / den, b = (St - s Sx) / Sw;   r_i = (s x_i + b) - t_i
 *     sigma = 1.2533141373155001 (sum w |r|) / Sw;   if k < iters and sigma > 0: q_i = |r_i| / (c sigma), w_i = 1 / (1 + q_i q_i),
 *     else the loop ends (sigma == 0 is an exact fit).
 * Status: 1 n_pairs < min_points; 2 degenerate at any iteration; 3 the final s <= 0 or a non-finite result; 0 fitted.  A frame that is
 * not fitted reports s = b = sigma = rms = 0 and n_inliers = 0.  n_inliers counts |r_i| <= 3 sigma after the last solve; rms =
 * sqrt(sum r^2 / n_pairs), unweighted.  Apply, for every pixel of a fitted frame with p > 0: v = s p + b, z = v (DEPTH) or 1 / v
 * (DISPARITY), valid iff v > 0 and z <= max_depth; depth_out = float32(z), to nearest, else 0; std_out = float32(max(std, std_floor))
 * with std = sigma (DEPTH) or (sigma z) z (DISPARITY) where depth_out came from the fit, else 0.  With keep_anchor a pixel with a > 0
 * takes the anchor's bits and std_floor.
 *
 * No atomics.  Every float64 sum is a fixed tree of (height, width) and the frame's pair count alone: the pairs are compacted in pixel
 * order, thread j of the frame's one workgroup adds pairs j, j + 1024, ... in that order, and the 1024 partial sums meet in the LDS halving
 * tree.  A frame's row and pixels are the same bits from call to call and for every batch the frame is passed in.
 */
#ifndef DEPTHALIGN_HIP_H
#define DEPTHALIGN_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DEPTHALIGN_ABI_VERSION 1
#define DEPTHALIGN_OK 0
#define DEPTHALIGN_ERR_ARG 1
#define DEPTHALIGN_ERR_HIP 2

#define DEPTHALIGN_MAX_FRAMES 65535
#define DEPTHALIGN_MAX_PIXELS (1ll << 28)    /* H * W of a frame */
#define DEPTHALIGN_MAX_ITERS 32              /* iters: reweighted solves after the first, 0 .. 32 */
#define DEPTHALIGN_TILE 2048                 /* a compaction workgroup takes 2048 consecutive pixels of one frame */

#define DEPTHALIGN_SPACE_DEPTH 0
#define DEPTHALIGN_SPACE_DISPARITY 1

#define DEPTHALIGN_STATUS_FITTED 0
#define DEPTHALIGN_STATUS_FEW 1              /* n_pairs < min_points */
#define DEPTHALIGN_STATUS_DEGENERATE 2       /* den <= 1e-8 Sw Sxx at some iteration: the prior is constant over the pairs */
#define DEPTHALIGN_STATUS_INVERTED 3         /* the final s <= 0, or a non-finite result: an inverted prior, or the wrong space */

/* the row of a frame: rows [n_frames, DEPTHALIGN_ROW] float64 */
#define DEPTHALIGN_ROW 8
#define DEPTHALIGN_ROW_S 0
#define DEPTHALIGN_ROW_B 1
#define DEPTHALIGN_ROW_SIGMA 2
#define DEPTHALIGN_ROW_N_PAIRS 3
#define DEPTHALIGN_ROW_N_INLIERS 4
#define DEPTHALIGN_ROW_STATUS 5
#define DEPTHALIGN_ROW_ITERATIONS 6          /* solves done */
#define DEPTHALIGN_ROW_RMS 7

const char* depthalign_last_error(void);
int depthalign_abi_version(void);

/* Bytes of the workspace of depthalign_fit_apply (aligned to 256 by the caller): the 12-byte pair (x float32, t float64) of every pixel, the
 * tiles' counts and offsets and the frames' pair counts.  -1 with a message for n_frames outside 1 .. 65535, height or width below 1, or
 * height * width above 2^28. */
int64_t depthalign_workspace_bytes(int n_frames, int height, int width);

/* The fit of every frame of prior against anchor and its application:
 *   space 0 / 1; iters 0 .. 32; c > 0 and finite; min_points >= 2; max_depth > 0 (+inf allowed); keep_anchor 0 / 1;
 *   std_floor >= 0 and finite
 *   depth_out [n_frames, height, width] float32
 *   std_out   [n_frames, height, width] float32, or null
 *   rows      [n_frames, 8] float64
 * No output and no part of the workspace may overlap prior or anchor, or another output. */
int depthalign_fit_apply(void* stream, int n_frames, int height, int width, const float* prior, const float* anchor, int space,
                         int iters, double c, int min_points, double max_depth, int keep_anchor, double std_floor, void* workspace,
                         float* depth_out, float* std_out, double* rows);

#ifdef __cplusplus
}
#endif
#endif

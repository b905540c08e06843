/* depthmetrics_hip.h -- C ABI of libdepthmetrics_hip.so: the depth-error columns of the evaluators on the MI355X (gfx950).  The
 * standard KITTI depth metrics of a split of rendered depth frames against their ground truth: RMSE, AbsRel, SqRel, the mean
 * absolute difference, RMSE of the logarithms and the three threshold ratios, plus the absolute-error map the MipNeRF-360
 * evaluators write as absrel_{idx}.npy.  The definition is DESIGN.md 8.5 and, as executable code, tests/depth_metrics_reference.py.
 *
 * Conventions as in depthvis_hip.h: plain C, raw DEVICE pointers, a `void* stream` (hipStream_t), return DEPTHMETRICS_OK or an
 * error code with depthmetrics_last_error(); the library is stateless and the caller owns every buffer.  The `*_bytes` query and
 * every argument check touch no HIP call and work on a host without a GPU.  Every call only enqueues.
 *
 * Arithmetic: the division by the scale, the valid mask, the clip and the error map in float32 (what numpy does with float32
 * frames and a Python-float scale); everything summed in float64 from those float32 values, no implicit fma.  No atomics: a
 * frame's sums are per-workgroup partials added in workgroup order, the number of workgroups of a frame and the pixels of every
 * thread depend on the frame's size alone, so a frame's nine numbers depend on that frame's values alone and are the same bits
 * from call to call and for any batch the frame is part of.
 */
#ifndef DEPTHMETRICS_HIP_H
#define DEPTHMETRICS_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DEPTHMETRICS_ABI_VERSION 1
#define DEPTHMETRICS_OK 0
#define DEPTHMETRICS_ERR_ARG 1
#define DEPTHMETRICS_ERR_HIP 2

#define DEPTHMETRICS_MAX_FRAMES 65535
#define DEPTHMETRICS_MAX_PIXELS (1ll << 28)  /* H * W of a frame */
#define DEPTHMETRICS_WG_PIXELS 2048          /* a frame of n pixels has min(ceil(n / 2048), 128) workgroups */

/* the row of a frame: out [n_frames, DEPTHMETRICS_ROW] float64 */
#define DEPTHMETRICS_ROW 9
#define DEPTHMETRICS_N_VALID 0   /* n: pixels with 1e-3 < gt / scale < 80 */
#define DEPTHMETRICS_RMSE 1      /* sqrt(sum d^2 / n),  d = g - clip(p, 1e-3, 80) */
#define DEPTHMETRICS_ABSREL 2    /* sum(|d| / g) / n */
#define DEPTHMETRICS_SQREL 3     /* sum(d^2 / g) / n */
#define DEPTHMETRICS_ABSDIFF 4   /* sum |d| / n */
#define DEPTHMETRICS_RMSE_LOG 5  /* sqrt(sum (log g - log vp)^2 / n) */
#define DEPTHMETRICS_A1 6        /* #(max(g / vp, vp / g) < 1.25) / n */
#define DEPTHMETRICS_A2 7        /* ... < 1.25^2 */
#define DEPTHMETRICS_A3 8        /* ... < 1.25^3 */

const char* depthmetrics_last_error(void);
int depthmetrics_abi_version(void);

/* Bytes of the workspace of depthmetrics_frames (aligned to 256 by the caller).  -1 with a message for n_frames outside
 * 1 .. 65535 or n_pixels outside 1 .. 2^28. */
int64_t depthmetrics_workspace_bytes(int n_frames, int64_t n_pixels);

/* out [n_frames, 9] float64 of pred, gt [n_frames, n_pixels] float32 in scene units; g = gt / float32(scale),
 * p = pred / float32(scale).  A frame without a valid pixel has n_valid 0 and NaN in the other eight; a NaN prediction on a
 * valid pixel makes that frame's sums NaN and counts in no threshold.  scale: finite and positive.
 * err_map [n_frames, n_pixels] float32 or null: |g - vp| in float32 on the valid pixels, 0 elsewhere. */
int depthmetrics_frames(void* stream, int n_frames, int64_t n_pixels, const float* pred, const float* gt, double scale,
                        void* workspace, double* out, float* err_map);

#ifdef __cplusplus
}
#endif
#endif

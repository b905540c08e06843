/* depthvis_hip.h -- C ABI of libdepthvis_hip.so: the depth pictures of the three evaluators on the MI355X (gfx950).  Weighted
 * percentiles of a frame (upstream's vis.weighted_percentile), a frame's min / max, and the colourised bytes of
 * vis.visualize_cmap / vis.matte / vis.visualize_coord_mod (MipNeRF-360) and utils.colorize_np (NeRF++).  The definition is
 * DESIGN.md 8.4 and, as executable code, tests/depth_vis_reference.py.
 *
 * Conventions as in colorcc_hip.h: plain C, raw DEVICE pointers, a `void* stream` (hipStream_t), return DEPTHVIS_OK or an
 * error code with depthvis_last_error(); the library is stateless and the caller owns every buffer.  The `*_bytes` query and
 * every argument check touch no HIP call and work on a host without a GPU.  Every call only enqueues.
 *
 * Arithmetic: float64 from float32 inputs, no implicit fma.  No floating-point atomics: a frame's sums are per-workgroup
 * partials added in workgroup order, and the number of workgroups of a frame depends on its size alone, so a frame's results
 * depend on that frame's values alone and are the same bits from call to call and for any batch the frame is part of.
 */
#ifndef DEPTHVIS_HIP_H
#define DEPTHVIS_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DEPTHVIS_ABI_VERSION 1
#define DEPTHVIS_OK 0
#define DEPTHVIS_ERR_ARG 1
#define DEPTHVIS_ERR_HIP 2

#define DEPTHVIS_MAX_N (1 << 22)        /* values of one frame in depthvis_percentiles */
#define DEPTHVIS_MAX_PIXELS (1ll << 28) /* H * W of the other calls */
#define DEPTHVIS_MAX_PS 4               /* percentiles of one call */

/* depthvis_colorize modes */
#define DEPTHVIS_MODE_CMAP 0            /* visualize_cmap with a colour table and the matte */
#define DEPTHVIS_MODE_CMAP3 1           /* visualize_cmap without a table on a 3-channel value (depth_triplet), matte */
#define DEPTHVIS_MODE_MINMAX 2          /* colorize_np without a mask: min-max, table, no matte */
#define DEPTHVIS_MODE_MATTE_RGB 3       /* matte(rgb, acc) (color_matte) */
#define DEPTHVIS_MODE_COORDS_MOD 4      /* matte(((origins + directions * distance + 1) % 2) / 2, acc) */
/* colour tables (matplotlib's 256-entry tables) */
#define DEPTHVIS_CMAP_TURBO 0
#define DEPTHVIS_CMAP_JET 1
/* curves of the two cmap modes, applied to value, lo and hi; eps = 2^-23 */
#define DEPTHVIS_CURVE_IDENTITY 0
#define DEPTHVIS_CURVE_NEG_LOG 1        /* -log(x + eps) */
#define DEPTHVIS_CURVE_LOG 2            /* log(x + eps) */

const char* depthvis_last_error(void);
int depthvis_abi_version(void);

/* Bytes of the workspace of depthvis_percentiles and depthvis_minmax for frames of n values (aligned to 256 by the caller).
 * -1 with a message for n_frames < 1 or > 65535, n < 1 or n > DEPTHVIS_MAX_N. */
int64_t depthvis_workspace_bytes(int n_frames, int64_t n);

/* out [n_frames, n_ps] float64: np.interp(ps * (cw[-1] / 100), cw, sorted value) with cw the running sum of the weights in
 * the order of (value ascending, NaN last, equal values by index).  value, weight [n_frames, n] float32; ps: n_ps HOST
 * doubles, 1 <= n_ps <= DEPTHVIS_MAX_PS.  A radix select over the 56-bit (order-preserving float image, index) key. */
int depthvis_percentiles(void* stream, int n_frames, int64_t n, const float* value, const float* weight, int n_ps,
                         const double* ps, void* workspace, double* out);

/* out [n_frames, 4] float32: min, max (NaN if the frame holds one, as numpy's), nanmin, nanmax (NaN for an all-NaN frame). */
int depthvis_minmax(void* stream, int n_frames, int64_t n, const float* value, void* workspace, float* out);

/* What the MipNeRF-360 suite derives per pixel before any picture, all [n_frames, n_pixels] float32:
 *   acc_eff = isnan(distance_mean) ? 0 : acc
 *   and, unless triplet_value is null, triplet_value [.., 3] = (2 * median - p5, median, p95) in float32 and
 *   triplet_weight [.., 3] = acc_eff three times (every channel entry of a pixel carries the pixel's weight). */
int depthvis_prepare(void* stream, int n_frames, int64_t n_pixels, const float* acc, const float* distance_mean,
                     const float* distance_median, const float* p5, const float* p95, float* acc_eff, float* triplet_value,
                     float* triplet_weight);

/* out [n_frames, H, W, 3] uint8 = clip(nan_to_num(v), 0, 1) * 255, truncated.  By mode:
 *   CMAP        value [F, H, W], acc [F, H, W], lohi [F, 2] float64 (lo_auto, hi_auto), cmap, curve
 *   CMAP3       value [F, H, W, 3], acc, lohi, curve
 *   MINMAX      value [F, H, W], minmax [F, 4] float32 (depthvis_minmax's rows), cmap
 *   MATTE_RGB   value [F, H, W, 3] (the colour), acc
 *   COORDS_MOD  value [F, H, W] (distance_mean), origins, directions [F, H, W, 3], acc
 * Pointers a mode does not name are ignored. */
int depthvis_colorize(void* stream, int n_frames, int H, int W, int mode, int cmap, int curve, const float* value,
                      const float* acc, const float* origins, const float* directions, const double* lohi,
                      const float* minmax, uint8_t* out);

#ifdef __cplusplus
}
#endif
#endif

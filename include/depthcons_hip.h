/* depthcons_hip.h -- C ABI of libdepthcons_hip.so: the multi-view geometric consistency check of depth priors on the MI355X
 * (gfx950).  Every valid prior pixel of every posed frame is taken into its neighbouring frames and back (the depth-map filter of
 * multi-view stereo); it is kept when enough neighbours agree, and the spread of what they say is its standard deviation.  The
 * definition is DESIGN.md 8.7 and, as executable code, tests/depth_consistency_reference.py.
 *
 * Conventions as in depthmetrics_hip.h: plain C, raw DEVICE pointers, a `void* stream` (hipStream_t), return DEPTHCONS_OK or an
 * error code with depthcons_last_error(); the library is stateless and the caller owns every buffer.  The `*_bytes` query and
 * every argument check touch no HIP call and work on a host without a GPU.  Every call only enqueues.
 *
 * Arithmetic: the geometry in IEEE float64 in the reference's written order, no implicit fma; the depth maps are float32 and are
 * widened exactly.  No atomics: a frame's row is the sum of per-workgroup integer partials, added by a second launch.  A pixel's
 * outputs depend on its frame, its neighbours' frames and cameras alone, so they are the same bits from call to call and for any
 * batch that holds them.
 */
#ifndef DEPTHCONS_HIP_H
#define DEPTHCONS_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DEPTHCONS_ABI_VERSION 1
#define DEPTHCONS_OK 0
#define DEPTHCONS_ERR_ARG 1
#define DEPTHCONS_ERR_HIP 2

#define DEPTHCONS_MAX_FRAMES 65535
#define DEPTHCONS_MAX_VIEWS 16               /* K: neighbours per frame */
#define DEPTHCONS_MAX_PIXELS (1ll << 28)     /* H * W of a frame */
#define DEPTHCONS_TILE_W 32                  /* a workgroup is a tile of 32 x 8 pixels of one frame */
#define DEPTHCONS_TILE_H 8

/* a camera: cams [n_frames, DEPTHCONS_CAM] float64 = fx fy cx cy, then the 3 x 4 camera-to-world [R | t] row-major, in the OpenCV
 * convention (x right, y down, z forward); depth is z-depth, pixel centres sit at +0.5 */
#define DEPTHCONS_CAM 16

/* the row of a frame: rows [n_frames, DEPTHCONS_ROW] int64 */
#define DEPTHCONS_ROW 4
#define DEPTHCONS_N_VALID 0        /* pixels with depth > 0 */
#define DEPTHCONS_N_VERIFIABLE 1   /* of those: n_seen >= min_views */
#define DEPTHCONS_N_KEPT 2         /* of the valid: kept */
#define DEPTHCONS_N_DROPPED 3      /* n_valid - n_kept */

const char* depthcons_last_error(void);
int depthcons_abi_version(void);

/* Bytes of the workspace of depthcons_check (aligned to 256 by the caller).  -1 with a message for n_frames outside 1 .. 65535,
 * height or width below 1, or height * width above 2^28. */
int64_t depthcons_workspace_bytes(int n_frames, int height, int width);

/* The check of depth [n_frames, height, width] float32 (valid iff > 0: 0, negatives and NaN pass through) with cams
 * [n_frames, 16] float64 and nbr [n_frames, n_views] int32, n_views 0 .. 16: the frames every frame is checked against, in list
 * order; an entry < 0 or >= n_frames is skipped.  pix_tol >= 0 pixels, rel_tol >= 0, min_views >= 1, keep_unverified 0 / 1,
 * std_floor >= 0 scene units; all finite.
 *   depth_out [n_frames, height, width] float32: the input where kept (and where invalid), 0 where dropped
 *   std_out   the same shape, or null: max(n_ok > 0 ? sqrt(s / n_ok) : rel_tol * d, std_floor) where kept and valid, else 0
 *   counts    [n_frames, height, width, 2] uint8, or null: n_seen, n_ok
 *   rows      [n_frames, 4] int64, or null
 * No output may overlap depth: the neighbours of a pixel read it. */
int depthcons_check(void* stream, int n_frames, int height, int width, int n_views, const float* depth, const double* cams,
                    const int32_t* nbr, double pix_tol, double rel_tol, int min_views, int keep_unverified, double std_floor,
                    void* workspace, float* depth_out, float* std_out, uint8_t* counts, int64_t* rows);

#ifdef __cplusplus
}
#endif
#endif

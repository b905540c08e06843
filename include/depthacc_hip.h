/* depthacc_hip.h -- C ABI of libdepthacc_hip.so: densifying sparse depth priors from neighbouring frames on the MI355X (gfx950).
 * Every valid prior pixel of a frame's neighbours is taken into the frame (multi-sweep accumulation, as KITTI's annotated depth is
 * built); where the frame has no measurement of its own, the nearest of what arrived is added unless a nearer surface in a small
 * window around it hides it.  The definition is DESIGN.md 8.8 and, as executable code, tests/depth_accumulate_reference.py.
 *
 * Conventions as in depthcons_hip.h: plain C, raw DEVICE pointers, a `void* stream` (hipStream_t), return DEPTHACC_OK or an error
 * code with depthacc_last_error(); the library is stateless and the caller owns every buffer.  The `*_bytes` query and every
 * argument check touch no HIP call and work on a host without a GPU.  Every call only enqueues.
 *
 * Arithmetic: the geometry in IEEE float64 in the reference's written order, no implicit fma; the depth maps are float32 and are
 * widened exactly; the one rounding is z -> float32, to nearest.  The scatter is a minimum over 64-bit integer keys (depth bits,
 * slot, source pixel), which does not depend on the order of arrival, and a frame's row is the sum of per-workgroup integer
 * partials, added by a second launch: the outputs are the same bits from call to call and for any batch that holds a frame and its
 * neighbours in the same slots.
 */
#ifndef DEPTHACC_HIP_H
#define DEPTHACC_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DEPTHACC_ABI_VERSION 1
#define DEPTHACC_OK 0
#define DEPTHACC_ERR_ARG 1
#define DEPTHACC_ERR_HIP 2

#define DEPTHACC_MAX_FRAMES 65535
#define DEPTHACC_MAX_VIEWS 16                /* V: neighbours per frame; the slot takes 4 bits of the key */
#define DEPTHACC_MAX_PIXELS (1ll << 28)      /* H * W of a frame; the source pixel takes 28 bits of the key */
#define DEPTHACC_MAX_RADIUS 8                /* occl_radius: the visibility window is (2 r + 1)^2 pixels */
#define DEPTHACC_TILE_W 32                   /* a resolve workgroup is a tile of 32 x 8 pixels of one frame */
#define DEPTHACC_TILE_H 8
#define DEPTHACC_SCATTER_TILE 2048           /* a scatter workgroup takes 2048 consecutive pixels of one source frame */

/* a camera: cams [n_frames, DEPTHACC_CAM] float64 = fx fy cx cy, then the 3 x 4 camera-to-world [R | t] row-major, in the OpenCV
 * convention (x right, y down, z forward); depth is z-depth, pixel centres sit at +0.5 */
#define DEPTHACC_CAM 16

/* origin of a pixel of depth_out */
#define DEPTHACC_ORIGIN_NONE 0      /* no measurement of its own and none arrived: the input passes through */
#define DEPTHACC_ORIGIN_OWN 1       /* the frame's own measurement */
#define DEPTHACC_ORIGIN_ADDED 2     /* a neighbour's measurement */
#define DEPTHACC_ORIGIN_HIDDEN 3    /* a neighbour's measurement arrived but a nearer surface hides it: the input passes through */

/* the row of a frame: rows [n_frames, DEPTHACC_ROW] int64 */
#define DEPTHACC_ROW 4
#define DEPTHACC_N_OWN 0            /* pixels with depth > 0 */
#define DEPTHACC_N_CANDIDATES 1     /* pixels without one that a neighbour's measurement reached: n_added + n_hidden */
#define DEPTHACC_N_ADDED 2
#define DEPTHACC_N_HIDDEN 3

const char* depthacc_last_error(void);
int depthacc_abi_version(void);

/* Bytes of the workspace of depthacc_accumulate (aligned to 256 by the caller): the 8-byte z-buffer of every pixel and the row
 * partials.  -1 with a message for n_frames outside 1 .. 65535, height or width below 1, or height * width above 2^28. */
int64_t depthacc_workspace_bytes(int n_frames, int height, int width);

/* The accumulation of depth [n_frames, height, width] float32 (valid iff > 0: 0, negatives and NaN are not) with cams
 * [n_frames, 16] float64 and nbr [n_frames, n_views] int32, n_views 0 .. 16: the frames whose measurements are taken into every
 * frame, slot by slot; an entry < 0 or >= n_frames is skipped.  occl_radius 0 .. 8 pixels, occl_tol >= 0 and finite.
 *   depth_out [n_frames, height, width] float32: the input, and a neighbour's z where origin is 2
 *   origin    [n_frames, height, width] uint8, or null: DEPTHACC_ORIGIN_*
 *   src       [n_frames, height, width] int32, or null: (slot << 28) | (y * width + x) of the source pixel where origin is 2 or 3,
 *             else -1
 *   rows      [n_frames, 4] int64, or null
 * No output and no part of the workspace may overlap depth: the launches read it throughout. */
int depthacc_accumulate(void* stream, int n_frames, int height, int width, int n_views, const float* depth, const double* cams,
                        const int32_t* nbr, int occl_radius, double occl_tol, void* workspace, float* depth_out, uint8_t* origin,
                        int32_t* src, int64_t* rows);

#ifdef __cplusplus
}
#endif
#endif

/* depthmvs_hip.h -- C ABI of libdepthmvs_hip.so: a plane-sweep multi-view stereo depth prior on the MI355X (gfx950), the classical,
 * weight-free stand-in for the paper's stereo prior.  Every frame is swept through fronto-parallel depth planes against its nearest
 * frames with the known poses: a 5 x 5 census of the luma is matched by Hamming distance, the best views of a plane are summed (the
 * occlusion rule), the sums are aggregated over a window, and the winning plane is refined by a parabola through its two
 * neighbours.  A pixel whose winner is not seen by enough views, sits at an end of the table or is not unique is refused.  The
 * definition is DESIGN.md 8.11 and, as executable code, tests/depth_mvs_reference.py.
 *
 * Conventions as in depthcomp_hip.h: plain C, raw DEVICE pointers, a `void* stream` (hipStream_t), return DEPTHMVS_OK or an error
 * code with depthmvs_last_error(); the library is stateless and the caller owns every buffer.  The `*_bytes` query and every
 * argument check touch no HIP call and work on a host without a GPU (the entries of inv_depth, cams and nbr are the caller's to
 * check: they live on the device; a neighbour index outside 0 .. n_frames - 1 counts as no neighbour).  Every call only enqueues.
 *
 * Arithmetic: everything discrete is integer arithmetic; the geometry and the refinement are IEEE float64 in the reference's
 * written order, no implicit fma; depth and std are each rounded to float32 once, to nearest.  No atomics: a frame's row is the sum
 * of per-workgroup integer partials, added by a last launch.  The outputs are the same bits from call to call and for a frame alone
 * with its neighbours or in any batch.
 */
#ifndef DEPTHMVS_HIP_H
#define DEPTHMVS_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DEPTHMVS_ABI_VERSION 1
#define DEPTHMVS_OK 0
#define DEPTHMVS_ERR_ARG 1
#define DEPTHMVS_ERR_HIP 2

#define DEPTHMVS_MAX_FRAMES 65535
#define DEPTHMVS_MAX_PIXELS (1ll << 28)     /* H * W of a frame */
#define DEPTHMVS_MAX_VIEWS 16               /* neighbours of a frame */
#define DEPTHMVS_MIN_PLANES 4
#define DEPTHMVS_MAX_PLANES 256
#define DEPTHMVS_MAX_RADIUS 4               /* the aggregation window is (2 a + 1)^2 taps */
#define DEPTHMVS_CAM 16                     /* fx fy cx cy + the 3 x 4 camera-to-world, row-major (OpenCV axes) */
#define DEPTHMVS_CENSUS_BITS 24             /* 5 x 5 without the centre; also the cost of a view that is out of bounds */
#define DEPTHMVS_TILE_W 32                  /* a workgroup of 256 threads is a tile of 32 x 16 pixels of one frame: two per thread */
#define DEPTHMVS_TILE_H 16

/* status of a pixel; the first rule that applies wins, in the order UNSEEN, END, AMBIGUOUS */
#define DEPTHMVS_ACCEPTED 0      /* depth and std are set */
#define DEPTHMVS_END 1           /* the winner is plane 0 or the last plane */
#define DEPTHMVS_AMBIGUOUS 2     /* not C* <= uniqueness * second */
#define DEPTHMVS_UNSEEN 3        /* fewer than best_views views are in bounds at the winner */

/* the row of a frame: rows [n_frames, DEPTHMVS_ROW] int64; the four add up to height * width */
#define DEPTHMVS_ROW 4
#define DEPTHMVS_N_ACCEPTED 0
#define DEPTHMVS_N_END 1
#define DEPTHMVS_N_AMBIGUOUS 2
#define DEPTHMVS_N_UNSEEN 3

const char* depthmvs_last_error(void);
int depthmvs_abi_version(void);

/* Bytes of the workspace of depthmvs_sweep (aligned to 256 by the caller): the census [n_frames, height, width] uint32 and the row
 * partials.  It does not grow with the number of planes.  -1 with a message for n_frames outside 1 .. 65535, height or width below
 * 1, or height * width above 2^28. */
int64_t depthmvs_workspace_bytes(int n_frames, int height, int width);

/* The sweep of rgb [n_frames, height, width, 3] uint8 with cams [n_frames, 16] float64, nbr [n_frames, n_views] int32 (-1: no
 * neighbour) and the planes inv_depth [n_planes] float64: inverse depths, strictly increasing, finite, >= 0 (entry 0 may be 0, the
 * plane at infinity).  n_views 1 .. 16, n_planes 4 .. 256, best_views 1 .. n_views, agg_radius 0 .. 4, uniqueness in (0, 1],
 * std_planes finite and > 0.
 *   depth   [n_frames, height, width] float32: 1 / w at accepted pixels, else 0
 *   std     [n_frames, height, width] float32: std_planes * z * z * step at accepted pixels, else 0
 *   status  [n_frames, height, width] uint8: DEPTHMVS_ACCEPTED .. DEPTHMVS_UNSEEN
 *   plane   [n_frames, height, width] uint8, or null: k*, the lowest plane of minimal aggregated cost
 *   cost    [n_frames, height, width] uint16, or null: C* = C(k*)
 *   second  [n_frames, height, width] uint16, or null: the minimum of C over |k - k*| > 1
 *   census  [n_frames, height, width] uint32, or null: the 24-bit census word of every pixel
 *   rows    [n_frames, 4] int64, or null
 * No output and no part of the workspace may overlap rgb, cams, nbr or inv_depth: the launches read them throughout. */
int depthmvs_sweep(void* stream, int n_frames, int height, int width, int n_views, int n_planes, const uint8_t* rgb,
                   const double* cams, const int32_t* nbr, const double* inv_depth, int best_views, int agg_radius, double uniqueness,
                   double std_planes, void* workspace, float* depth, float* std, uint8_t* status, uint8_t* plane, uint16_t* cost,
                   uint16_t* second, uint32_t* census, int64_t* rows);

#ifdef __cplusplus
}
#endif
#endif

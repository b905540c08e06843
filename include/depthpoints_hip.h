/* depthpoints_hip.h -- C ABI of libdepthpoints_hip.so: a sparse depth prior from a 3D point cloud with tracks (the points of the
 * scene's own reconstruction) on the MI355X (gfx950).  Every point is taken into the frames that observed it (or into every frame
 * whose frustum holds it), the nearest point of a pixel wins, and a point that a nearer one in a small window hides is left out.
 * Besides the depth the call writes a per-pixel standard deviation and the index of the winning point.  The definition is DESIGN.md
 * 8.12 and, as executable code, tests/depth_points_reference.py.
 *
 * Conventions as in depthacc_hip.h: plain C, raw DEVICE pointers, a `void* stream` (hipStream_t), return DEPTHPOINTS_OK or an error
 * code with depthpoints_last_error(); the library is stateless and the caller owns every buffer.  The `*_bytes` query and every
 * argument check touch no HIP call and work on a host without a GPU.  Every call only enqueues.
 *
 * Arithmetic: the geometry in IEEE float64 in the reference's written order, no implicit fma; the one rounding of a depth is
 * z -> float32, to nearest.  The scatter is a minimum over 64-bit integer keys (depth bits, point index), which does not depend on
 * the order of arrival; the counts are integers (per-workgroup partials summed by a last launch, and integer atomic adds): the
 * outputs are the same bits from call to call, for any order of the observations and for any batch of frames.
 */
#ifndef DEPTHPOINTS_HIP_H
#define DEPTHPOINTS_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DEPTHPOINTS_ABI_VERSION 1
#define DEPTHPOINTS_OK 0
#define DEPTHPOINTS_ERR_ARG 1
#define DEPTHPOINTS_ERR_HIP 2

#define DEPTHPOINTS_MAX_FRAMES 65535
#define DEPTHPOINTS_MAX_PIXELS (1ll << 28)     /* H * W of a frame */
#define DEPTHPOINTS_MAX_POINTS 2147483647ll    /* the point index takes the low 32 bits of the key and is written as an int32 */
#define DEPTHPOINTS_MAX_OBS (1ll << 40)
#define DEPTHPOINTS_MAX_RADIUS 8               /* occl_radius: the visibility window is (2 r + 1)^2 pixels */
#define DEPTHPOINTS_TILE_W 32                  /* a resolve workgroup is a tile of 32 x 8 pixels of one frame */
#define DEPTHPOINTS_TILE_H 8
#define DEPTHPOINTS_POINT_TILE 1024            /* in the `all` mode a scatter workgroup takes 1024 consecutive points into one frame */

/* a camera: cams [n_frames, DEPTHPOINTS_CAM] float64 = fx fy cx cy, then the 3 x 4 camera-to-world [R | t] row-major, in the OpenCV
 * convention (x right, y down, z forward); depth is z-depth, pixel centres sit at +0.5 (depthacc_hip.h's) */
#define DEPTHPOINTS_CAM 16
/* a point: points [n_points, DEPTHPOINTS_POINT] float64 = x y z in the cameras' world, then coef: the standard deviation of a pixel
 * that shows the point at depth z is max(std_floor, std_scale * coef * z * z / fx) */
#define DEPTHPOINTS_POINT 4
/* an observation: obs [n_obs, DEPTHPOINTS_OBS] int32 = (point, frame) */
#define DEPTHPOINTS_OBS 2

/* origin of a pixel of depth_out */
#define DEPTHPOINTS_ORIGIN_NONE 0     /* no point reached the pixel: depth 0 */
#define DEPTHPOINTS_ORIGIN_POINT 1    /* the nearest point that reached it */
#define DEPTHPOINTS_ORIGIN_HIDDEN 2   /* a point reached it, but a nearer one in its window hides it: depth 0 */

/* the row of a frame: rows [n_frames, DEPTHPOINTS_ROW] int64 */
#define DEPTHPOINTS_ROW 4
#define DEPTHPOINTS_N_OBS 0           /* observations presented to the frame: its rows of obs with a point inside the table, or n_points */
#define DEPTHPOINTS_N_PROJECTED 1     /* those inside the frame and the depth range */
#define DEPTHPOINTS_N_KEPT 2          /* pixels with origin POINT */
#define DEPTHPOINTS_N_HIDDEN 3        /* pixels with origin HIDDEN */

const char* depthpoints_last_error(void);
int depthpoints_abi_version(void);

/* Bytes of the workspace of depthpoints_splat (aligned to 256 by the caller): the 8-byte z-buffer of every pixel, the row partials
 * and the per-frame counters.  -1 with a message for n_frames outside 1 .. 65535, height or width below 1, or height * width above
 * 2^28. */
int64_t depthpoints_workspace_bytes(int n_frames, int height, int width);

/* The splat of points [n_points, 4] float64 (aligned to 16 bytes) into n_frames frames of height x width pixels with cams
 * [n_frames, 16] float64.
 *   obs given (the `track` mode): obs [n_obs, 2] int32 = (point, frame); a point goes into the frames that observed it.  A row whose
 *       point is outside [0, n_points) or whose frame is outside [0, n_frames) is skipped.  The order of the rows changes no output;
 *       rows sorted by frame keep a wave on one camera.
 *   obs null (the `all` mode; n_obs must be 0): every point goes into every frame.
 * A point at camera coordinates (x, y, z) of a frame is projected there iff z is finite, near <= z <= far and
 * (floor(fx * x / z + cx), floor(fy * y / z + cy)) lies inside the frame.  0 < near < far, both finite; occl_radius 0 .. 8 pixels;
 * occl_tol >= 0 and finite; std_scale > 0 and finite; std_floor >= 0 and finite; n_points 0 .. 2^31 - 1; n_obs 0 .. 2^40.
 *   depth_out [n_frames, height, width] float32: z where origin is POINT, else 0
 *   std_out   [n_frames, height, width] float32, or null: the standard deviation where origin is POINT, else 0
 *   point     [n_frames, height, width] int32, or null: the winning point where origin is POINT, else -1
 *   origin    [n_frames, height, width] uint8, or null: DEPTHPOINTS_ORIGIN_*
 *   rows      [n_frames, 4] int64, or null */
int depthpoints_splat(void* stream, int n_frames, int height, int width, const double* cams, int64_t n_points, const double* points,
                      int64_t n_obs, const int32_t* obs, double near, double far, int occl_radius, double occl_tol, double std_scale,
                      double std_floor, void* workspace, float* depth_out, float* std_out, int32_t* point, uint8_t* origin,
                      int64_t* rows);

#ifdef __cplusplus
}
#endif
#endif

/* depthcomp_hip.h -- C ABI of libdepthcomp_hip.so: completing sparse depth priors by image-guided filtering on the MI355X (gfx950).
 * Joint-bilateral normalised convolution: a pixel without a measurement takes the confidence-weighted mean of the measured depths in
 * a window around it, each weighted by its distance in the image and by how much its colour differs from the pixel's, so that the
 * fill stops at object boundaries; a window that straddles two surfaces is refused.  A few passes carry the fill outwards.  The
 * definition is DESIGN.md 8.10 and, as executable code, tests/depth_complete_reference.py.
 *
 * Conventions as in depthacc_hip.h: plain C, raw DEVICE pointers, a `void* stream` (hipStream_t), return DEPTHCOMP_OK or an error
 * code with depthcomp_last_error(); the library is stateless and the caller owns every buffer.  The `*_bytes` query and every
 * argument check touch no HIP call and work on a host without a GPU (the weight tables' entries are the caller's to check: they
 * live on the device).  Every call only enqueues.
 *
 * Arithmetic: IEEE float64 in the reference's written order, no implicit fma; the float32 planes are widened exactly; z, c, v and
 * std_out are each rounded to float32 once, to nearest.  No atomics: a pass reads the state of the pass before it and writes its
 * own, and a frame's row is the sum of per-workgroup integer partials, added by a last launch.  The outputs are the same bits from
 * call to call and for a frame alone or in any batch.
 */
#ifndef DEPTHCOMP_HIP_H
#define DEPTHCOMP_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DEPTHCOMP_ABI_VERSION 1
#define DEPTHCOMP_OK 0
#define DEPTHCOMP_ERR_ARG 1
#define DEPTHCOMP_ERR_HIP 2

#define DEPTHCOMP_MAX_FRAMES 65535
#define DEPTHCOMP_MAX_PIXELS (1ll << 28)     /* H * W of a frame */
#define DEPTHCOMP_MAX_RADIUS 8               /* the window is (2 r + 1)^2 taps */
#define DEPTHCOMP_MAX_ITERS 16
#define DEPTHCOMP_MAX_POINTS 289             /* min_points: at most every tap of the widest window */
#define DEPTHCOMP_COLOUR_TABLE 766           /* |dR| + |dG| + |dB| = 0 .. 765 */
#define DEPTHCOMP_TILE_W 32                  /* a workgroup of 256 threads is a tile of 32 x 16 pixels of one frame: two per thread */
#define DEPTHCOMP_TILE_H 16

/* origin of a pixel of depth_out */
#define DEPTHCOMP_ORIGIN_NONE 0      /* empty, and the last pass found too little around it: the input passes through */
#define DEPTHCOMP_ORIGIN_OWN 1       /* the frame's own measurement */
#define DEPTHCOMP_ORIGIN_FILLED 2    /* filled by pass `pass` */
#define DEPTHCOMP_ORIGIN_REFUSED 3   /* empty, and the last pass found a window that straddles two surfaces: the input passes through */

/* the row of a frame: rows [n_frames, DEPTHCOMP_ROW] int64; the four add up to height * width */
#define DEPTHCOMP_ROW 4
#define DEPTHCOMP_N_OWN 0
#define DEPTHCOMP_N_FILLED 1
#define DEPTHCOMP_N_REFUSED 2
#define DEPTHCOMP_N_NONE 3

const char* depthcomp_last_error(void);
int depthcomp_abi_version(void);

/* Bytes of the workspace of depthcomp_complete (aligned to 256 by the caller): one more state (z, c, v, pass) for the passes to
 * alternate with the outputs, stand-ins for the outputs the caller leaves out, and the row partials.  -1 with a message for n_frames
 * outside 1 .. 65535, height or width below 1, or height * width above 2^28. */
int64_t depthcomp_workspace_bytes(int n_frames, int height, int width);

/* The completion of depth [n_frames, height, width] float32 (valid iff > 0: 0, negatives and NaN are not) guided by rgb
 * [n_frames, height, width, 3] uint8, with std_in [n_frames, height, width] float32 or null (the standard deviation of the frame's
 * own measurements; a value not > 0 counts as 0), w_space [(2 radius + 1)^2] float64 row-major over (dy, dx) and w_colour [766]
 * float64 indexed by |dR| + |dG| + |dB|, every entry finite and >= 0.  radius 1 .. 8, iters 1 .. 16, min_points 1 .. 289, min_conf
 * in [0, 1], max_rel_spread >= 0 (+inf: no gate), decay in (0, 1].
 *   depth_out [n_frames, height, width] float32: z where conf > 0, elsewhere the input with its bits
 *   std_out   [n_frames, height, width] float32: sqrt(v) where conf > 0, else 0
 *   conf      [n_frames, height, width] float32, or null: 1 at own pixels, below 1 at filled ones, 0 elsewhere
 *   origin    [n_frames, height, width] uint8: DEPTHCOMP_ORIGIN_*
 *   pass      [n_frames, height, width] uint8, or null: the pass that filled the pixel, else 0
 *   rows      [n_frames, 4] int64, or null
 * No output and no part of the workspace may overlap depth, rgb, std_in or a table: the launches read them throughout. */
int depthcomp_complete(void* stream, int n_frames, int height, int width, const float* depth, const uint8_t* rgb, const float* std_in,
                       const double* w_space, const double* w_colour, int radius, int iters, int min_points, double min_conf,
                       double max_rel_spread, double decay, void* workspace, float* depth_out, float* std_out, float* conf,
                       uint8_t* origin, uint8_t* pass, int64_t* rows);

#ifdef __cplusplus
}
#endif
#endif

/* depthsgm_hip.h -- C ABI of libdepthsgm_hip.so: the plane-sweep multi-view stereo depth prior of depthmvs_hip.h with semi-global
 * smoothing on the MI355X (gfx950).  The aggregated cost C(p, k) of the sweep (steps 1 to 4 of DESIGN.md 8.11, the one definition
 * both libraries compile) is summed along 4 or 8 scanline directions with a penalty P1 for a change of one plane and P2 for a
 * jump, and the winner, the uniqueness test and the parabola are taken on the sum S(p, k).  The definition is DESIGN.md 8.11a and,
 * as executable code, tests/depth_mvs_smooth_reference.py.
 *
 * Conventions, limits, the camera layout, the status values and the row of a frame are those of depthmvs_hip.h (the DEPTHMVS_*
 * constants hold here).  The `*_bytes` query and every argument check touch no HIP call and work on a host without a GPU.  Every
 * call only enqueues.
 *
 * Arithmetic: everything new is integer arithmetic.  One path's value L <= 31104 + P2 < 2^16, the sum over the paths S < 2^19.
 * The refinement is step 7 of the sweep on S.  No atomics: within a launch every (pixel, plane) belongs to one path, the launches
 * of the directions are ordered on the stream.  The outputs are the same bits from call to call, for a frame alone with its
 * neighbours or in any batch, and for every slab_frames.
 */
#ifndef DEPTHSGM_HIP_H
#define DEPTHSGM_HIP_H

#include <stdint.h>
#include "depthmvs_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define DEPTHSGM_ABI_VERSION 1
#define DEPTHSGM_OK 0
#define DEPTHSGM_ERR_ARG 1
#define DEPTHSGM_ERR_HIP 2

#define DEPTHSGM_MAX_P2 32767               /* so that one path's value fits 16 bits */
#define DEPTHSGM_MAX_EDGE 255
#define DEPTHSGM_PLANE_ALIGN 8              /* a pixel's curve in the slabs is n_planes rounded up to a multiple of this */
#define DEPTHSGM_SLAB_ENTRY_BYTES 6         /* C uint16 + S uint32 per (pixel, plane) of a slab frame */

const char* depthsgm_last_error(void);
int depthsgm_abi_version(void);

/* Bytes of the workspace of depthsgm_sweep (aligned to 256 by the caller), every part rounded up to 256: the census
 * [n_frames, height, width] uint32, the row partials [n_frames, tiles, 4] int32, and the slabs of s = min(slab_frames, n_frames)
 * frames with d = n_planes rounded up to a multiple of 8: C [s, height, width, d] uint16 and S [s, height, width, d] uint32.
 * -1 with a message for sizes depthmvs_workspace_bytes refuses, n_planes outside 4 .. 256 or slab_frames < 1. */
int64_t depthsgm_workspace_bytes(int n_frames, int height, int width, int n_planes, int slab_frames);

/* depthmvs_sweep with smoothing.  The arguments of depthmvs_sweep mean what they mean there.  smooth_paths 4 or 8; p1, p2: the
 * penalties in the units of C, 1 <= p1 <= p2 <= 32767; smooth_edge 0 .. 255 (0: P2 is constant, else P2' = max(p1, p2 / (1 +
 * |Y(p) - Y(q)| / smooth_edge)) with the census' luma Y); slab_frames >= 1: the frames the slabs hold, the call loops over chunks
 * of that many and the results do not depend on it.
 *   cost    [n_frames, height, width] uint32, or null: S* = S(k*)
 *   second  [n_frames, height, width] uint32, or null: the minimum of S over |k - k*| > 1
 * Every other output as in depthmvs_sweep, taken on S. */
int depthsgm_sweep(void* stream, int n_frames, int height, int width, int n_views, int n_planes, const uint8_t* rgb,
                   const double* cams, const int32_t* nbr, const double* inv_depth, int best_views, int agg_radius, double uniqueness,
                   double std_planes, int smooth_paths, int p1, int p2, int smooth_edge, int slab_frames, void* workspace, float* depth,
                   float* std, uint8_t* status, uint8_t* plane, uint32_t* cost, uint32_t* second, uint32_t* census, int64_t* rows);

#ifdef __cplusplus
}
#endif
#endif

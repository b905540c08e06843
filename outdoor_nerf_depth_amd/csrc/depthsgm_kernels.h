// Launchers of libdepthsgm_hip.so (depthsgm_kernels.hip) and the sizes its workspace follows from.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/depthsgm_hip.h"
#include "depthmvs_kernels.h"

constexpr int DEPTHSGM_PATH_WAVES = 4;                                 // scanlines of a workgroup of the paths kernel, one wave each

inline int depthsgm_dp(int n_planes) { return (n_planes + DEPTHSGM_PLANE_ALIGN - 1) / DEPTHSGM_PLANE_ALIGN * DEPTHSGM_PLANE_ALIGN; }

// the scanlines of one frame along (dx, dy): one per pixel whose predecessor lies outside the frame
inline int64_t depthsgm_lines(int height, int width, int dx, int dy) {
  return dx != 0 && dy != 0 ? (int64_t)width + height - 1 : dx != 0 ? height : width;
}

// One direction over the frames of a chunk.  cslab / sslab: [frames, H, W, dp] uint16 / uint32; rgb: the chunk's first frame.
struct DepthsgmPaths {
  const uint16_t* cslab; uint32_t* sslab; const uint8_t* rgb;
  int frames, height, width, n_planes, dp, dx, dy, p1, p2, edge, first;
  int64_t lines;                                                       // of one frame
};

// The select step over the frames [f0, f0 + frames) of the call, whose curves are frames 0 .. of the slabs
struct DepthsgmSelect {
  const uint16_t* cslab; const uint32_t* sslab; const double* inv_depth;
  float* depth; float* std; uint8_t* status; uint8_t* plane; uint32_t* cost; uint32_t* second; int32_t* partial;
  int height, width, tiles_x, n_planes, dp;
  int64_t tiles, f0;
  double uniqueness, std_planes;
};

void launch_depthsgm_census(hipStream_t st, const uint8_t* rgb, int height, int width, int64_t i0, int64_t n, uint32_t* census);
// Workgroups [wg0, wg0 + n_wg) of the (frame, tile) of the call; a.slab, a.slab_f0 and a.dp say where the curves go
void launch_depthsgm_slab(hipStream_t st, const DepthmvsSweep& a, int64_t wg0, int64_t n_wg);
// Workgroups [wg0, wg0 + n_wg) of the ceil(frames * lines / 4) of one direction
void launch_depthsgm_paths(hipStream_t st, const DepthsgmPaths& a, int64_t wg0, int64_t n_wg);
// Workgroups [wg0, wg0 + n_wg) of the frames * tiles of the chunk, (frame, tile) with the tile fastest
void launch_depthsgm_select(hipStream_t st, const DepthsgmSelect& a, int64_t wg0, int64_t n_wg);
void launch_depthsgm_rows(hipStream_t st, int n_frames, int64_t tiles, int64_t frame_px, const int32_t* partial, int64_t* rows);

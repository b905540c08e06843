// Launchers of libdepthalign_hip.so (depthalign_kernels.hip) and the sizes its workspace follows from.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/depthalign_hip.h"
#include "depth_prior_device.h"

constexpr int DEPTHALIGN_BLOCK = 256;                                  // threads of a tile, scan and apply workgroup
constexpr int DEPTHALIGN_FIT_BLOCK = 1024;                             // threads of a frame's fit workgroup

static_assert(DEPTHALIGN_TILE % DEPTHALIGN_BLOCK == 0, "whole rounds of loads per tile");

inline int64_t depthalign_tiles(int height, int width) { return ((int64_t)height * width + DEPTHALIGN_TILE - 1) / DEPTHALIGN_TILE; }

struct DepthAlignParams {
  int space, iters, min_points, keep_anchor;
  double c, max_depth, std_floor;
};

// Workgroups [wg0, wg0 + n_wg) of the n_frames * tiles of a call, (frame, tile) with the tile fastest.  xs == null: the count of
// every tile's pairs to counts [n_frames, tiles]; else the pairs, in pixel order, from offsets [n_frames, tiles]: x = p to xs and
// t = a (or 1.0 / a with disparity) to ts, both [n_frames, height * width].
void launch_depthalign_tiles(hipStream_t st, int height, int width, int64_t wg0, int64_t n_wg, int disparity, const float* prior,
                             const float* anchor, int32_t* counts, const int32_t* offsets, float* xs, double* ts);
// offsets: the exclusive scan of every frame's counts; n_pairs [n_frames]: their sum
void launch_depthalign_scan(hipStream_t st, int n_frames, int64_t tiles, const int32_t* counts, int32_t* offsets, int32_t* n_pairs);
void launch_depthalign_fit(hipStream_t st, int n_frames, int64_t frame_px, const float* xs, const double* ts, const int32_t* n_pairs,
                           const DepthAlignParams& prm, double* rows);
void launch_depthalign_apply(hipStream_t st, int n_frames, int64_t frame_px, const float* prior, const float* anchor, const double* rows,
                             const DepthAlignParams& prm, float* depth_out, float* std_out);

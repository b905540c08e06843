// Launchers of libdepthacc_hip.so (depthacc_kernels.hip) and the sizes its workspace follows from.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/depthacc_hip.h"
#include "depth_prior_device.h"

constexpr int DEPTHACC_BLOCK = DEPTHACC_TILE_W * DEPTHACC_TILE_H;     // threads of a workgroup of every kernel here

static_assert(DEPTHACC_BLOCK == 256 && DEPTHACC_SCATTER_TILE % DEPTHACC_BLOCK == 0, "four waves; whole rounds of loads per scatter tile");

inline int64_t depthacc_tiles(int height, int width) { return depthprior::tiles(height, width, DEPTHACC_TILE_W, DEPTHACC_TILE_H); }
inline int64_t depthacc_scatter_tiles(int height, int width) {
  return ((int64_t)height * width + DEPTHACC_SCATTER_TILE - 1) / DEPTHACC_SCATTER_TILE;
}

// Workgroups [wg0, wg0 + n_wg) of the n_frames * n_views * scatter_tiles of a call, (frame, slot, tile) with the tile fastest.
void launch_depthacc_scatter(hipStream_t st, int n_frames, int height, int width, int n_views, int64_t wg0, int64_t n_wg,
                             const float* depth, const double* cams, const int32_t* nbr, unsigned long long* zbuf);
// Workgroups [wg0, wg0 + n_wg) of the n_frames * tiles of a call, (frame, tile) with the tile fastest.  one_plus_tol = 1.0 + occl_tol.
// partial [n_frames, tiles, 4] int32 or null: own, candidates, added, 0 of every tile.
void launch_depthacc_resolve(hipStream_t st, int height, int width, int64_t wg0, int64_t n_wg, const float* depth,
                             const unsigned long long* zbuf, int radius, double one_plus_tol, float* depth_out, uint8_t* origin,
                             int32_t* src, int32_t* partial);
void launch_depthacc_rows(hipStream_t st, int n_frames, int64_t tiles, const int32_t* partial, int64_t* rows);

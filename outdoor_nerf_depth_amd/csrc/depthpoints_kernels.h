// Launchers of libdepthpoints_hip.so (depthpoints_kernels.hip) and the sizes its workspace follows from.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/depthpoints_hip.h"
#include "depth_prior_device.h"

constexpr int DEPTHPOINTS_BLOCK = DEPTHPOINTS_TILE_W * DEPTHPOINTS_TILE_H;   // threads of a workgroup of every kernel but the rows'

static_assert(DEPTHPOINTS_BLOCK == 256 && DEPTHPOINTS_POINT_TILE % DEPTHPOINTS_BLOCK == 0, "four waves; whole rounds of loads per point tile");

inline int64_t depthpoints_tiles(int height, int width) {
  return depthprior::tiles(height, width, DEPTHPOINTS_TILE_W, DEPTHPOINTS_TILE_H);
}
inline int64_t depthpoints_point_tiles(int64_t n_points) { return (n_points + DEPTHPOINTS_POINT_TILE - 1) / DEPTHPOINTS_POINT_TILE; }

// The projection's parameters, shared by both scatter kernels
struct DepthPointsRange {
  double near, far;
};

// `track`: workgroups [wg0, wg0 + n_wg) of the ceil(n_obs / 256) of a call, one thread per row of obs.
// counts [n_frames, 2] uint64 or null: n_obs, n_projected of every frame, added to.
void launch_depthpoints_scatter_obs(hipStream_t st, int n_frames, int height, int width, int64_t wg0, int64_t n_wg, const double* cams,
                                    int64_t n_points, const double* points, int64_t n_obs, const int32_t* obs, DepthPointsRange rg,
                                    unsigned long long* zbuf, unsigned long long* counts);
// `all`: workgroups [wg0, wg0 + n_wg) of the n_frames * point_tiles of a call, (frame, tile) with the tile fastest.
void launch_depthpoints_scatter_all(hipStream_t st, int height, int width, int64_t wg0, int64_t n_wg, const double* cams,
                                    int64_t n_points, const double* points, DepthPointsRange rg, unsigned long long* zbuf,
                                    unsigned long long* counts);
// Workgroups [wg0, wg0 + n_wg) of the n_frames * tiles of a call, (frame, tile) with the tile fastest.  one_plus_tol = 1.0 + occl_tol.
// partial [n_frames, tiles, 2] int32 or null: kept, hidden of every tile.
void launch_depthpoints_resolve(hipStream_t st, int height, int width, int64_t wg0, int64_t n_wg, const double* cams,
                                const double* points, const unsigned long long* zbuf, int radius, double one_plus_tol,
                                double std_scale, double std_floor, float* depth_out, float* std_out, int32_t* point, uint8_t* origin,
                                int32_t* partial);
void launch_depthpoints_rows(hipStream_t st, int n_frames, int64_t tiles, const int32_t* partial, const unsigned long long* counts,
                             int64_t* rows);

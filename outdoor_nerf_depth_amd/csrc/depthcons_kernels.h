// Launchers of libdepthcons_hip.so (depthcons_kernels.hip) and the sizes its workspace follows from.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/depthcons_hip.h"
#include "depth_prior_device.h"

constexpr int DEPTHCONS_BLOCK = DEPTHCONS_TILE_W * DEPTHCONS_TILE_H;   // threads of a check workgroup: one per pixel of its tile

static_assert(DEPTHCONS_BLOCK == 256 && DEPTHCONS_TILE_W % 32 == 0, "four waves, each two whole tile rows");

struct DepthconsParams {
  double pix_tol2, rel_tol, std_floor;
  int min_views, keep_unverified;
};

inline int64_t depthcons_tiles(int height, int width) { return depthprior::tiles(height, width, DEPTHCONS_TILE_W, DEPTHCONS_TILE_H); }

// The tiles [tile0, tile0 + n_tiles) of the frames [frame0, frame0 + n_launch_frames): n_tiles * n_launch_frames <= depthprior::MAX_GRID.
// partial [n_frames, tiles, 4] int32 or null: valid, verifiable, kept, 0 of every tile.
void launch_depthcons_check(hipStream_t st, int n_frames, int height, int width, int n_views, int frame0, int n_launch_frames,
                            int64_t tile0, int64_t n_tiles, const float* depth, const double* cams, const int32_t* nbr,
                            DepthconsParams prm, float* depth_out, float* std_out, uint8_t* counts, int32_t* partial);
void launch_depthcons_rows(hipStream_t st, int n_frames, int64_t tiles, const int32_t* partial, int64_t* rows);

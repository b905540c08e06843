// Launchers of libdepthcomp_hip.so (depthcomp_kernels.hip) and the sizes its workspace follows from.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/depthcomp_hip.h"
#include "depth_prior_device.h"

constexpr int DEPTHCOMP_BLOCK = 256;                                   // threads of a workgroup of the pass kernel
constexpr int DEPTHCOMP_PPT = DEPTHCOMP_TILE_W * DEPTHCOMP_TILE_H / DEPTHCOMP_BLOCK;   // pixels of a thread: rows ty, ty + 8

static_assert(DEPTHCOMP_BLOCK % DEPTHCOMP_TILE_W == 0 && DEPTHCOMP_PPT * DEPTHCOMP_BLOCK == DEPTHCOMP_TILE_W * DEPTHCOMP_TILE_H,
              "whole rows of the tile per round of the workgroup");

inline int64_t depthcomp_tiles(int height, int width) { return depthprior::tiles(height, width, DEPTHCOMP_TILE_W, DEPTHCOMP_TILE_H); }

// The state of every pixel between two passes: depth, confidence, variance [F, H, W] float32 and the pass that filled it [F, H, W] uint8
struct DepthcompState {
  float* z; float* c; float* v; uint8_t* pass;
};

// One pass.  The first reads depth (and std_in, nullable) and no state; every later one reads `in`.  A pass that is not the last
// writes `out`, all four planes.  The last writes the call's outputs instead: out.z = depth_out and out.v = std_out in their final
// form, out.c = conf and out.pass = pass (either may be null), origin, and partial [F, tiles, 4] int32 (or null): own, filled,
// refused, 0 of every tile.
struct DepthcompPass {
  const float* depth; const uint8_t* rgb; const float* std_in; const double* w_space; const double* w_colour;
  DepthcompState in, out;
  uint8_t* origin; int32_t* partial;
  int height, width, tiles_x, radius, k, min_points;
  int64_t tiles;
  double min_conf, max_rel_spread, decay;
};

// Workgroups [wg0, wg0 + n_wg) of the n_frames * tiles of a pass, (frame, tile) with the tile fastest.
void launch_depthcomp_pass(hipStream_t st, const DepthcompPass& a, bool first, bool last, int64_t wg0, int64_t n_wg);
void launch_depthcomp_rows(hipStream_t st, int n_frames, int64_t tiles, int64_t frame_px, const int32_t* partial, int64_t* rows);

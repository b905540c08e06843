// Launchers of libdepthmvs_hip.so (depthmvs_kernels.hip) and the sizes its workspace follows from.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/depthmvs_hip.h"
#include "depth_prior_device.h"

constexpr int DEPTHMVS_BLOCK = 256;                                    // threads of a workgroup of the sweep kernel
constexpr int DEPTHMVS_PPT = DEPTHMVS_TILE_W * DEPTHMVS_TILE_H / DEPTHMVS_BLOCK;   // pixels of a thread: rows ty, ty + 8

static_assert(DEPTHMVS_BLOCK % DEPTHMVS_TILE_W == 0 && DEPTHMVS_PPT * DEPTHMVS_BLOCK == DEPTHMVS_TILE_W * DEPTHMVS_TILE_H,
              "whole rows of the tile per round of the workgroup");

inline int64_t depthmvs_tiles(int height, int width) { return depthprior::tiles(height, width, DEPTHMVS_TILE_W, DEPTHMVS_TILE_H); }

// One sweep.  census [F, H, W] uint32 is written by launch_depthmvs_census first and read by the sweep.  plane, cost, second and
// partial ([F, tiles, 4] int32: accepted, end, ambiguous, 0 of every tile) may be null.  The slab instantiation of the sweep
// (depthmvs_sweep.h, libdepthsgm_hip.so) writes none of the outputs but slab [frames of the chunk, H, W, dp] uint16 with dp a
// multiple of 8, frame slab_f0 of the call first; the plain one does not read the three.
struct DepthmvsSweep {
  const double* cams; const int32_t* nbr; const double* inv_depth; const uint32_t* census;
  float* depth; float* std; uint8_t* status; uint8_t* plane; uint16_t* cost; uint16_t* second; int32_t* partial;
  int n_frames, height, width, tiles_x, n_views, n_planes, best_views, radius;
  int64_t tiles;
  double uniqueness, std_planes;
  uint16_t* slab; int64_t slab_f0; int dp;
};

// Pixels [i0, i0 + n) of the n_frames * height * width of the census
void launch_depthmvs_census(hipStream_t st, const uint8_t* rgb, int height, int width, int64_t i0, int64_t n, uint32_t* census);
// Workgroups [wg0, wg0 + n_wg) of the n_frames * tiles of the sweep, (frame, tile) with the tile fastest.
void launch_depthmvs_sweep(hipStream_t st, const DepthmvsSweep& a, int64_t wg0, int64_t n_wg);
void launch_depthmvs_rows(hipStream_t st, int n_frames, int64_t tiles, int64_t frame_px, const int32_t* partial, int64_t* rows);

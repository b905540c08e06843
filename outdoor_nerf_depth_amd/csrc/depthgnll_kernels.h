// Launchers of libdepthgnll_hip.so (depthgnll_kernels.hip) and the layout of its workspace.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/depthgnll_hip.h"
#include "hip_device.h"

constexpr int DEPTHGNLL_RAYS_PER_BLOCK = 4;    // launch 1: one wave per (ray, level), four waves per workgroup
constexpr int DEPTHGNLL_FINISH_BLOCK = 1024;   // launch 2: threads of its one workgroup

// what both launches read; passed by value
struct DepthGnllArgs {
  int n, n_levels, edges;
  int S[DEPTHGNLL_MAX_LEVELS];
  const float* w[DEPTHGNLL_MAX_LEVELS];
  const float* x[DEPTHGNLL_MAX_LEVELS];
  const float* d[DEPTHGNLL_MAX_LEVELS];
  float* g_w[DEPTHGNLL_MAX_LEVELS];            // null entries: no gradient for that level
  float* g_d[DEPTHGNLL_MAX_LEVELS];
  float scale[DEPTHGNLL_MAX_LEVELS];
  const float* p; const float* sigma; const float* limit;   // limit may be null
  double* ws_loss;                             // [n_levels, n] the ray's l_r, 0 when not gated
  int32_t* ws_class;                           // [n_levels, n] bit 0 supervised, bit 1 gated, bit 2 V < 1e-3
  float* values; float* stats;
  hipdev::LevelFolds folds;
};

// the doubles first, so that both parts are aligned
inline int64_t depthgnll_ws_bytes(int n_levels, int n) { return (int64_t)n_levels * n * (int64_t)(sizeof(double) + sizeof(int32_t)); }

void launch_depthgnll_rays(hipStream_t st, const DepthGnllArgs& a);
void launch_depthgnll_finish(hipStream_t st, const DepthGnllArgs& a);

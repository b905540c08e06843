// Launchers of libdepthssi_hip.so (depthssi_kernels.hip) and the layout of its workspace.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/depthssi_hip.h"
#include "hip_device.h"

constexpr int DEPTHSSI_BLOCK = 256;        // threads of both kernels

// what both launches read; passed by value
struct DepthSsiArgs {
  int n, n_levels, n_groups, min_rays, norm, g_stride;
  const float* d[DEPTHSSI_MAX_LEVELS];
  float* grads[DEPTHSSI_MAX_LEVELS];       // null entries: no gradient for that level
  float scale[DEPTHSSI_MAX_LEVELS];
  const float* p;
  const int32_t* g;                        // null: every ray in group 0
  double* ws;                              // [n_levels, n_groups] sum of r^2 (0 when not fitted), then [n_levels] N_sup
  float* values; float* fit; float* stats;
  hipdev::LevelFolds folds;
};

inline int64_t depthssi_ws_doubles(int n_levels, int n_groups) { return (int64_t)n_levels * n_groups + n_levels; }

void launch_depthssi_groups(hipStream_t st, const DepthSsiArgs& a);
void launch_depthssi_finish(hipStream_t st, const DepthSsiArgs& a);

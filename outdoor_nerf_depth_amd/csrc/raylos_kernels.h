// Launchers of libraylos_hip.so (raylos_kernels.hip) and the layout of its workspace.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/raylos_hip.h"

constexpr int RAYLOS_RAYS_PER_BLOCK = 4;    // launch 1: one wave per ray, four waves per workgroup
constexpr int RAYLOS_FINISH_BLOCK = 1024;   // launch 2: threads of its one workgroup

// what both launches read; passed by value
struct RayLosArgs {
  int n, S;
  const float* w; const float* z; const float* hi; const float* p; const float* sigma;
  double lambda;
  float* g_w;                                  // null: values only
  double* ws_los;                              // [n] the ray's L_r, 0 when unsupervised
  double* ws_front;                            // [n] the ray's front_r, 0 when unsupervised
  int32_t* ws_sup;                             // [n] the ray's class: 1 supervised, 0 not
  float* values; float* stats; float* fold_total;
};

// the doubles first, so that every part is aligned
inline int64_t raylos_ws_bytes(int n) { return (int64_t)n * (int64_t)(2 * sizeof(double) + sizeof(int32_t)); }

void launch_raylos_rays(hipStream_t st, const RayLosArgs& a);
void launch_raylos_finish(hipStream_t st, const RayLosArgs& a);

// Launchers of librayreg_hip.so (rayreg_kernels.hip), the layout of its workspace and the float64 wave scans its kernel uses.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/rayreg_hip.h"
#include "hip_device.h"

constexpr int RAYREG_RAYS_PER_BLOCK = 4;    // launch 1: one wave per ray, four waves per workgroup
constexpr int RAYREG_FINISH_BLOCK = 1024;   // launch 2: threads of its one workgroup

// what both launches read; passed by value
struct RayRegArgs {
  int n, S;
  const float* w; const float* z; const float* lo; const float* hi;
  double lambda_dist, lambda_opac;
  float* g_w;                                  // null: values only
  double* ws_dist;                             // [n] the ray's dist_r, 0 when invalid or lambda_dist = 0
  double* ws_opac;                             // [n] the ray's opac_r, 0 when lambda_opac = 0
  int32_t* ws_valid;                           // [n] hi > lo
  float* values; float* stats; float* fold_total;
};

// the doubles first, so that every part is aligned
inline int64_t rayreg_ws_bytes(int n) { return (int64_t)n * (int64_t)(2 * sizeof(double) + sizeof(int32_t)); }

void launch_rayreg_rays(hipStream_t st, const RayRegArgs& a);
void launch_rayreg_finish(hipStream_t st, const RayRegArgs& a);

#ifdef __HIPCC__
namespace rayreg {

// float64 scans over the 64 lanes of a wave, each a fixed shuffle tree (the float ones are hip_device.h's wave_incl_sum and
// wave_excl_suffix_sum):  exclusive prefix  out(lane) = sum_{l < lane} x(l),   exclusive suffix  out(lane) = sum_{l > lane} x(l)
__device__ __forceinline__ double wave_excl_prefix_sum(double x, int lane) {
  double v = x;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const double t = __shfl_up(v, d, 64);
    if (lane >= d) v += t;
  }
  const double e = __shfl_up(v, 1, 64);
  return lane == 0 ? 0.0 : e;
}
__device__ __forceinline__ double wave_excl_suffix_sum(double x, int lane) {
  double v = x;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const double t = __shfl_down(v, d, 64);
    if (lane + d < 64) v += t;
  }
  const double e = __shfl_down(v, 1, 64);
  return lane == 63 ? 0.0 : e;
}

}  // namespace rayreg
#endif

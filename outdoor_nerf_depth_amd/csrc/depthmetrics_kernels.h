// Launchers of libdepthmetrics_hip.so (depthmetrics_kernels.hip) and the sizes its workspace follows from.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/depthmetrics_hip.h"

constexpr int DEPTHMETRICS_BLOCK = 256;    // threads of a reduce workgroup
constexpr int DEPTHMETRICS_QUAD = 4;       // consecutive pixels a thread takes at once: one 16-byte load where the frame is aligned
constexpr int DEPTHMETRICS_MAX_WG = 128;   // workgroups per frame: a function of the frame's size alone
constexpr int DEPTHMETRICS_SUMS = 5;       // d^2, |d| / g, d^2 / g, |d|, L^2
constexpr int DEPTHMETRICS_COUNTS = 4;     // valid, thresh < 1.25, < 1.25^2, < 1.25^3

static_assert(DEPTHMETRICS_SUMS + DEPTHMETRICS_COUNTS == DEPTHMETRICS_ROW, "a partial row is a frame's row before the divisions");
static_assert(DEPTHMETRICS_WG_PIXELS % (DEPTHMETRICS_BLOCK * DEPTHMETRICS_QUAD) == 0, "whole quads per thread");

inline int depthmetrics_workgroups(int64_t n_pixels) {
  const int64_t g = (n_pixels + DEPTHMETRICS_WG_PIXELS - 1) / DEPTHMETRICS_WG_PIXELS;
  return (int)(g < DEPTHMETRICS_MAX_WG ? g : DEPTHMETRICS_MAX_WG);
}

// partial [n_frames, nwg, 9] float64: the five sums, then the four counts (exact in float64)
void launch_depthmetrics_reduce(hipStream_t st, int n_frames, int64_t n_pixels, int nwg, const float* pred, const float* gt,
                                float scale, double* partial, float* err_map);
void launch_depthmetrics_finish(hipStream_t st, int n_frames, int nwg, const double* partial, double* out);

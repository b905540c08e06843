// Launchers of colorcc_kernels.hip and the sizes colorcc_api.hip lays the workspace out with.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/colorcc_hip.h"

constexpr int COLORCC_BLOCK = 256;       // threads of an accumulate / apply workgroup
constexpr int COLORCC_MAX_WG = 64;       // workgroups per frame (and channel): a function of H * W alone

inline int colorcc_workgroups(int64_t n_pixels) {
  const int64_t n = (n_pixels + COLORCC_BLOCK - 1) / COLORCC_BLOCK;
  return (int)(n < COLORCC_MAX_WG ? n : COLORCC_MAX_WG);
}

// weights [n_frames, COLORCC_ITERS, 3, 10]; partials [n_frames, 3, nwg, COLORCC_SUMS]; sse_partials [n_frames, nwg]
void launch_colorcc_accumulate(hipStream_t st, int n_frames, int64_t n_pixels, int nwg, const float* img, const uint8_t* ref,
                               const double* weights, int iteration, double* partials);
// adds a (frame, channel)'s partials in workgroup order; sums != null: writes them [n_frames, 3, COLORCC_SUMS] and stops;
// else solves for weights[.., iteration, c, :] and writes the mask count to out[f, 2 + iteration * 3 + c]
void launch_colorcc_solve(hipStream_t st, int n_frames, int nwg, const double* partials, int iteration, double* weights,
                          double* out, double* sums);
void launch_colorcc_apply(hipStream_t st, int n_frames, int64_t n_pixels, int nwg, const float* img, const uint8_t* ref,
                          const double* weights, int quantize, double* rgb_cc, uint8_t* cc_u8, double* sse_partials);
void launch_colorcc_finish(hipStream_t st, int n_frames, int64_t n_pixels, int nwg, const double* sse_partials, double* out);

// Internal launch interface of liblpips_hip.so (lpips_conv.hip, lpips_tap.hip -> lpips_api.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

constexpr int LPIPS_KC = 16;                      // k rows per staged chunk; Kp is a multiple of it
constexpr int LPIPS_TAP_PIX = 64;                 // pixels per workgroup of the tap kernel = one partial sum

inline int lpips_kp(int Cin) { return (9 * Cin + LPIPS_KC - 1) / LPIPS_KC * LPIPS_KC; }
inline int lpips_tap_blocks(int H, int W) { return (H * W + LPIPS_TAP_PIX - 1) / LPIPS_TAP_PIX; }

// lpips_conv.hip
void launch_lpips_pack_conv(hipStream_t st, int Cin, int Cout, const float* w, float* wp);
void launch_lpips_conv3x3_relu(hipStream_t st, int n_images, int H, int W, int Cin, int Cout, const float* x, const float* wp,
                               const float* bias, float* y);
// lpips_tap.hip
void launch_lpips_prep(hipStream_t st, int n_pairs, int H, int W, const unsigned char* gt, const unsigned char* pred, float* x);
void launch_lpips_pool(hipStream_t st, int n_images, int H, int W, int C, const float* x, float* y);
// f [2 * n_pairs, H, W, C] (images 2p, 2p + 1 = the pair p) -> part[p * part_stride + b], b < lpips_tap_blocks(H, W)
void launch_lpips_tap(hipStream_t st, int n_pairs, int H, int W, int C, const float* f, const float* lin, double* part,
                      int64_t part_stride);
// part [n_pairs, part_stride]: tap l occupies [off[l], off[l] + nblk[l]); out [n_pairs, 6]
struct LpipsFinishArgs { int off[5]; int nblk[5]; double npix[5]; };
void launch_lpips_finish(hipStream_t st, int n_pairs, const double* part, int64_t part_stride, LpipsFinishArgs a, double* out);

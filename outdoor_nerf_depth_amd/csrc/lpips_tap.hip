// The element-wise and reduction kernels of LPIPS (lpips_hip.h): input scaling, 2 x 2 max-pool, the per-tap distance and the
// final sum.  Nothing here is an atomic.  A tap workgroup owns 64 consecutive pixels of ONE pair and writes one float64
// partial; lpips_finish_kernel adds a pair's partials in a fixed order, so a pair's values depend on its own bytes alone.
//
// lpips_tap_kernel: one wave per pixel at a time, the C channels spread over the lanes (C / 64 per lane and image), so both
// feature maps are read once: the two norms by a butterfly sum (every lane ends with the same bits), then
// sum_c w[c] * (f0[c] / (|f0| + 1e-10) - f1[c] / (|f1| + 1e-10))^2 in float64.  Equal features give exactly 0.  The workgroup's
// partial: the butterfly again, then the four waves in wave order (hipdev::wave_deposit / waves_collect).
#include <math.h>
#include "hip_device.h"
#include "lpips_kernels.h"

namespace {

using hipdev::wave_sum;       // every lane ends with the same bits
using hipdev::wave_deposit, hipdev::waves_collect;

// x = byte / 255 * 2 - 1, then (x - shift) / scale, in float32 in this order (the file is built without fma contraction)
__global__ __launch_bounds__(256) void lpips_prep_kernel(int n_pairs, int HW, const unsigned char* __restrict__ gt,
                                                         const unsigned char* __restrict__ pred, float* __restrict__ x) {
  const size_t per = (size_t)HW * 3, total = (size_t)n_pairs * 2 * per;
  const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= total) return;
  const size_t img = idx / per, e = idx - img * per;
  const int c = (int)(e % 3);
  const unsigned char* src = (img & 1) ? pred : gt;
  const float v = (float)src[(img >> 1) * per + e] / 255.f * 2.f - 1.f;
  const float shift = c == 0 ? -.030f : c == 1 ? -.088f : -.188f;
  const float scale = c == 0 ? .458f : c == 1 ? .448f : .450f;
  x[idx] = (v - shift) / scale;
}

// y [n, H / 2, W / 2, C] = max over 2 x 2 of x [n, H, W, C]; an odd trailing row / column is dropped.  C % 4 == 0.
__global__ __launch_bounds__(256) void lpips_pool_kernel(int n_images, int H, int W, int C4, const float4* __restrict__ x,
                                                         float4* __restrict__ y) {
  const int Ho = H / 2, Wo = W / 2;
  const size_t total = (size_t)n_images * Ho * Wo * C4;
  const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= total) return;
  const int c = (int)(idx % C4);
  size_t p = idx / C4;
  const int xo = (int)(p % Wo); p /= Wo;
  const int yo = (int)(p % Ho);
  const size_t img = p / Ho;
  const float4* s = x + ((img * H + 2 * yo) * W + 2 * xo) * C4 + c;
  const float4 a = s[0], b = s[C4], d = s[(size_t)W * C4], e = s[(size_t)W * C4 + C4];
  y[idx] = make_float4(fmaxf(fmaxf(a.x, b.x), fmaxf(d.x, e.x)), fmaxf(fmaxf(a.y, b.y), fmaxf(d.y, e.y)),
                       fmaxf(fmaxf(a.z, b.z), fmaxf(d.z, e.z)), fmaxf(fmaxf(a.w, b.w), fmaxf(d.w, e.w)));
}

template <int CPL>                                // channels per lane: C = 64 * CPL
__global__ __launch_bounds__(256) void lpips_tap_kernel(int HW, const float* __restrict__ f, const float* __restrict__ lin,
                                                        double* __restrict__ part, int64_t part_stride) {
  constexpr int C = 64 * CPL, WAVES = 4, PER_WAVE = LPIPS_TAP_PIX / WAVES;
  __shared__ double red[WAVES][1];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, pair = blockIdx.y;
  const float* f0 = f + (size_t)(2 * pair) * HW * C;
  const float* f1 = f0 + (size_t)HW * C;
  double w[CPL];
#pragma unroll
  for (int j = 0; j < CPL; ++j) w[j] = (double)lin[lane + 64 * j];
  double acc = 0.0;
  for (int t = 0; t < PER_WAVE; ++t) {
    const int p = blockIdx.x * LPIPS_TAP_PIX + wv * PER_WAVE + t;
    if (p >= HW) break;                           // wave-uniform
    double a[CPL], b[CPL], sa = 0.0, sb = 0.0;
#pragma unroll
    for (int j = 0; j < CPL; ++j) {
      a[j] = (double)f0[(size_t)p * C + lane + 64 * j];
      b[j] = (double)f1[(size_t)p * C + lane + 64 * j];
      sa += a[j] * a[j];
      sb += b[j] * b[j];
    }
    const double na = sqrt(wave_sum(sa)) + 1e-10, nb = sqrt(wave_sum(sb)) + 1e-10;
#pragma unroll
    for (int j = 0; j < CPL; ++j) {
      const double d = a[j] / na - b[j] / nb;
      acc += w[j] * (d * d);
    }
  }
  wave_deposit(red, 0, wave_sum(acc));
  __syncthreads();
  if (threadIdx.x == 0) part[(size_t)pair * part_stride + blockIdx.x] = waves_collect<double>(red, 0);
}

// one workgroup per pair, wave l adds tap l: lane j takes partials j, j + 64, ... in order, then the butterfly
__global__ __launch_bounds__(320) void lpips_finish_kernel(const double* __restrict__ part, int64_t part_stride,
                                                           LpipsFinishArgs a, double* __restrict__ out) {
  __shared__ double d[5];
  const int lane = threadIdx.x & 63, l = threadIdx.x >> 6, pair = blockIdx.x;
  const double* p = part + (size_t)pair * part_stride + a.off[l];
  double s = 0.0;
  for (int k = lane; k < a.nblk[l]; k += 64) s += p[k];
  s = wave_sum(s);
  if (lane == 0) d[l] = s / a.npix[l];
  __syncthreads();
  if (threadIdx.x == 0) {
    double t = d[0];
    for (int k = 1; k < 5; ++k) t += d[k];
    for (int k = 0; k < 5; ++k) out[(size_t)pair * 6 + k] = d[k];
    out[(size_t)pair * 6 + 5] = t;
  }
}

}  // namespace

void launch_lpips_prep(hipStream_t st, int n_pairs, int H, int W, const unsigned char* gt, const unsigned char* pred, float* x) {
  const size_t total = (size_t)n_pairs * 2 * H * W * 3;
  lpips_prep_kernel<<<(unsigned)((total + 255) / 256), 256, 0, st>>>(n_pairs, H * W, gt, pred, x);
}

void launch_lpips_pool(hipStream_t st, int n_images, int H, int W, int C, const float* x, float* y) {
  const size_t total = (size_t)n_images * (H / 2) * (W / 2) * (C / 4);
  lpips_pool_kernel<<<(unsigned)((total + 255) / 256), 256, 0, st>>>(n_images, H, W, C / 4, (const float4*)x, (float4*)y);
}

void launch_lpips_tap(hipStream_t st, int n_pairs, int H, int W, int C, const float* f, const float* lin, double* part,
                      int64_t part_stride) {
  const dim3 grid(lpips_tap_blocks(H, W), n_pairs);
  const int HW = H * W;
  switch (C) {
    case 64: lpips_tap_kernel<1><<<grid, 256, 0, st>>>(HW, f, lin, part, part_stride); break;
    case 128: lpips_tap_kernel<2><<<grid, 256, 0, st>>>(HW, f, lin, part, part_stride); break;
    case 256: lpips_tap_kernel<4><<<grid, 256, 0, st>>>(HW, f, lin, part, part_stride); break;
    default: lpips_tap_kernel<8><<<grid, 256, 0, st>>>(HW, f, lin, part, part_stride); break;   // 512
  }
}

void launch_lpips_finish(hipStream_t st, int n_pairs, const double* part, int64_t part_stride, LpipsFinishArgs a, double* out) {
  lpips_finish_kernel<<<n_pairs, 320, 0, st>>>(part, part_stride, a, out);
}

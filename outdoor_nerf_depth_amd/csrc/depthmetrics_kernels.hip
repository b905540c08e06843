// Depth-error metrics of a split.  float32 up to the clipped prediction, float64 from there, no atomics, compiled
// with -ffp-contract=off.
//
//   reduce  grid (nwg, frames), 256 threads.  A frame's pixels are cut into quads of 4 consecutive pixels; quad q belongs to
//           workgroup (q / 256) % nwg, thread q % 256, and a thread takes its quads in ascending order and a quad's pixels in
//           ascending order.  nwg = min(ceil(n / 2048), 128): all of it follows from n alone.  A whole quad is one 16-byte load
//           per input where the frame's base is 16-byte aligned (f * n a multiple of 4) and four 4-byte loads where it is not:
//           the same pixels in the same order either way.  Every thread keeps five float64 sums and four counts; they are
//           added over the wave by a shfl_down tree, then over the four waves in wave order by nine threads (hipdev::wave_deposit /
//           waves_collect), which write the workgroup's partial row.  The error map is written on the way.
//   finish  grid (frames), 64 threads: the frame's partial rows go to LDS, thread k adds column k in workgroup order; thread 0
//           divides.
#include "depthmetrics_kernels.h"
#include "hip_device.h"

namespace {

using hipdev::f32x4;
using hipdev::wave_sum_lane0, hipdev::wave_deposit, hipdev::waves_collect;

constexpr int BLOCK = DEPTHMETRICS_BLOCK, QUAD = DEPTHMETRICS_QUAD, WAVES = BLOCK / 64, ROW = DEPTHMETRICS_ROW;
constexpr float LO = 1e-3f, HI = 80.f;                      // the reference's validity and clip bounds, in metres
constexpr double T1 = 1.25, T2 = 1.5625, T3 = 1.953125;

struct Acc {
  double s[DEPTHMETRICS_SUMS];
  uint32_t c[DEPTHMETRICS_COUNTS];
};

// one pixel: its error-map value; its terms go to `a` when it is valid
__device__ inline float dm_pixel(float pred, float gt, float scale, Acc& a) {
  const float g = gt / scale, p = pred / scale;
  if (!(g < HI && g > LO)) return 0.f;                       // a NaN is never valid
  const float vp = p < LO ? LO : (p > HI ? HI : p);          // numpy's clip: a NaN stays NaN
  const double G = (double)g, V = (double)vp;
  const double d = G - V, ad = fabs(d), d2 = d * d;
  const double L = log(G) - log(V);
  const double r0 = G / V, r1 = V / G;
  const double thresh = r0 > r1 ? r0 : r1;                   // NaN when V is
  a.s[0] += d2;
  a.s[1] += ad / G;
  a.s[2] += d2 / G;
  a.s[3] += ad;
  a.s[4] += L * L;
  a.c[0] += 1u;
  a.c[1] += thresh < T1 ? 1u : 0u;
  a.c[2] += thresh < T2 ? 1u : 0u;
  a.c[3] += thresh < T3 ? 1u : 0u;
  return fabsf(g - vp);
}

__global__ __launch_bounds__(BLOCK) void depthmetrics_reduce_kernel(int64_t n, int nwg, const float* __restrict__ pred,
                                                                   const float* __restrict__ gt, float scale,
                                                                   double* __restrict__ partial, float* __restrict__ err_map) {
  const int f = blockIdx.y, g = blockIdx.x, tid = threadIdx.x;
  const float* fp = pred + (int64_t)f * n;
  const float* fg = gt + (int64_t)f * n;
  float* fe = err_map == nullptr ? nullptr : err_map + (int64_t)f * n;
  const bool vec_in = (((uintptr_t)fp | (uintptr_t)fg) & 15) == 0;
  const bool vec_out = ((uintptr_t)fe & 15) == 0;
  Acc a;
#pragma unroll
  for (int k = 0; k < DEPTHMETRICS_SUMS; ++k) a.s[k] = 0.0;
#pragma unroll
  for (int k = 0; k < DEPTHMETRICS_COUNTS; ++k) a.c[k] = 0u;
  const int64_t n_quads = (n + QUAD - 1) / QUAD;
  for (int64_t q = (int64_t)g * BLOCK + tid; q < n_quads; q += (int64_t)nwg * BLOCK) {
    const int64_t i = q * QUAD;
    if (i + QUAD <= n) {
      float p[QUAD], t[QUAD], e[QUAD];
      if (vec_in) {
        const f32x4 pv = *(const f32x4*)(fp + i), tv = *(const f32x4*)(fg + i);
#pragma unroll
        for (int k = 0; k < QUAD; ++k) { p[k] = pv[k]; t[k] = tv[k]; }
      } else {
#pragma unroll
        for (int k = 0; k < QUAD; ++k) { p[k] = fp[i + k]; t[k] = fg[i + k]; }
      }
#pragma unroll
      for (int k = 0; k < QUAD; ++k) e[k] = dm_pixel(p[k], t[k], scale, a);
      if (fe != nullptr) {
        if (vec_out) {
          f32x4 ev;
#pragma unroll
          for (int k = 0; k < QUAD; ++k) ev[k] = e[k];
          *(f32x4*)(fe + i) = ev;
        } else {
#pragma unroll
          for (int k = 0; k < QUAD; ++k) fe[i + k] = e[k];
        }
      }
    } else {                                                 // the frame's last, partial quad
      for (int64_t j = i; j < n; ++j) {
        const float e = dm_pixel(fp[j], fg[j], scale, a);
        if (fe != nullptr) fe[j] = e;
      }
    }
  }
  __shared__ double red[WAVES][ROW];
#pragma unroll
  for (int k = 0; k < DEPTHMETRICS_SUMS; ++k) wave_deposit(red, k, wave_sum_lane0(a.s[k]));
#pragma unroll
  for (int k = 0; k < DEPTHMETRICS_COUNTS; ++k)              // a workgroup sees at most 2^28 pixels
    wave_deposit(red, DEPTHMETRICS_SUMS + k, (double)wave_sum_lane0(a.c[k]));
  __syncthreads();
  if (tid < ROW) partial[((int64_t)f * nwg + g) * ROW + tid] = waves_collect<double>(red, tid);
}

__global__ __launch_bounds__(64) void depthmetrics_finish_kernel(int nwg, const double* __restrict__ partial,
                                                                double* __restrict__ out) {
  const int f = blockIdx.x, tid = threadIdx.x;
  __shared__ double rows[DEPTHMETRICS_MAX_WG * ROW];         // the frame's partial rows, loaded side by side: the adds wait for no load
  __shared__ double sum[ROW];
  const double* fpart = partial + (int64_t)f * nwg * ROW;
  for (int i = tid; i < nwg * ROW; i += 64) rows[i] = fpart[i];
  __syncthreads();
  if (tid < ROW) {
    double s = rows[tid];
    for (int g = 1; g < nwg; ++g) s += rows[g * ROW + tid];
    sum[tid] = s;
  }
  __syncthreads();
  if (tid != 0) return;
  const double n = sum[DEPTHMETRICS_SUMS];                   // 0 / 0 below is the NaN of numpy's empty mean
  double* o = out + (int64_t)f * ROW;
  o[DEPTHMETRICS_N_VALID] = n;
  o[DEPTHMETRICS_RMSE] = sqrt(sum[0] / n);
  o[DEPTHMETRICS_ABSREL] = sum[1] / n;
  o[DEPTHMETRICS_SQREL] = sum[2] / n;
  o[DEPTHMETRICS_ABSDIFF] = sum[3] / n;
  o[DEPTHMETRICS_RMSE_LOG] = sqrt(sum[4] / n);
  o[DEPTHMETRICS_A1] = sum[DEPTHMETRICS_SUMS + 1] / n;
  o[DEPTHMETRICS_A2] = sum[DEPTHMETRICS_SUMS + 2] / n;
  o[DEPTHMETRICS_A3] = sum[DEPTHMETRICS_SUMS + 3] / n;
}

}  // namespace

void launch_depthmetrics_reduce(hipStream_t st, int n_frames, int64_t n_pixels, int nwg, const float* pred, const float* gt,
                                float scale, double* partial, float* err_map) {
  depthmetrics_reduce_kernel<<<dim3(nwg, n_frames), BLOCK, 0, st>>>(n_pixels, nwg, pred, gt, scale, partial, err_map);
}

void launch_depthmetrics_finish(hipStream_t st, int n_frames, int nwg, const double* partial, double* out) {
  depthmetrics_finish_kernel<<<n_frames, 64, 0, st>>>(nwg, partial, out);
}

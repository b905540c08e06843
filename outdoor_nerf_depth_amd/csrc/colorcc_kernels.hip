// Colour correction of test renders: upstream's image.color_correct as four kernels, float64, no atomics.
//
//   accumulate  grid (nwg, 3, frames): a workgroup walks its share of one frame's pixels for ONE channel's mask, rebuilds the
//               current pixel from the float32 render with the warps already fitted (cc_current, in registers: there is no
//               float64 working image) and keeps the channel's 66 masked sums (55 Gram, 10 right-hand sides, count) per
//               thread; wave shuffle tree (cc_wave_sum), then the four waves in order (hipdev::wave_deposit / waves_collect), one
//               partial per (frame, channel, workgroup).
//   solve       grid (3, frames), one wave: partials added in workgroup order, Gram scaled to unit diagonal, cyclic Jacobi
//               (12 sweeps) in LDS, pseudo-inverse with a relative eigenvalue cut-off.
//   apply       grid (nwg, frames): cc_current with all five warps -> rgb_cc, the truncated bytes, squared-error partials.
//   finish      adds a frame's squared-error partials in workgroup order.
//
// The channels go one after another (a workgroup per channel) rather than three systems at once: 66 float64 sums are 132
// VGPRs, three are 396 and spill.  Compiled with -ffp-contract=off and explicit fma() in cc_warp, so accumulate and apply
// compute the same bits for a pixel and a mask never disagrees with the output.
#include "colorcc_kernels.h"
#include "hip_device.h"

namespace {

using hipdev::wave_deposit, hipdev::waves_collect;

constexpr int NF = COLORCC_FEATURES, NS = COLORCC_SUMS, NW = 3 * NF;      // NW: doubles of one iteration's warp [3][10]
constexpr double EPS = 0.5 / 255;

__device__ inline bool cc_unclipped(double z) { return (z >= EPS) & (z <= 1 - EPS); }

__device__ inline void cc_features(double r, double g, double b, double a[NF]) {
  a[0] = r * r; a[1] = r * g; a[2] = r * b; a[3] = g * g; a[4] = g * b; a[5] = b * b;
  a[6] = r; a[7] = g; a[8] = b; a[9] = 1.0;
}

__device__ inline double cc_clip01(double v) { return fmin(fmax(v, 0.0), 1.0); }

// x <- clip(a(x) . w, 0, 1); w [3][10] (uniform address: scalar loads)
__device__ inline void cc_warp(const double* __restrict__ w, double x[3]) {
  double a[NF];
  cc_features(x[0], x[1], x[2], a);
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    double s = 0.0;
#pragma unroll
    for (int k = 0; k < NF; ++k) s = fma(a[k], w[c * NF + k], s);
    x[c] = cc_clip01(s);
  }
}

// x0: the render's pixel as float64, non-finite -> 0; x: x0 after the first n_warps fitted warps of the frame
__device__ inline void cc_current(const float* __restrict__ px, const double* __restrict__ wf, int n_warps, double x0[3], double x[3]) {
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const float v = px[c];
    x0[c] = isfinite(v) ? (double)v : 0.0;
    x[c] = x0[c];
  }
  for (int i = 0; i < n_warps; ++i) cc_warp(wf + i * NW, x);
}

__device__ inline double cc_wave_sum(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o);
  return v;                                                  // lane 0 holds the wave's sum (a fixed tree)
}

__global__ __launch_bounds__(COLORCC_BLOCK) void colorcc_accumulate_kernel(
    int64_t n_pixels, int nwg, const float* __restrict__ img, const uint8_t* __restrict__ ref, const double* __restrict__ weights,
    int iteration, double* __restrict__ partials) {
  const int c = blockIdx.y, f = blockIdx.z, tid = threadIdx.x;
  const float* fimg = img + (int64_t)f * n_pixels * 3;
  const uint8_t* fref = ref + (int64_t)f * n_pixels * 3;
  const double* wf = weights + (int64_t)f * COLORCC_ITERS * NW;
  double acc[NS];
#pragma unroll
  for (int k = 0; k < NS; ++k) acc[k] = 0.0;
  for (int64_t p = (int64_t)blockIdx.x * COLORCC_BLOCK + tid; p < n_pixels; p += (int64_t)nwg * COLORCC_BLOCK) {
    double x0[3], x[3];
    cc_current(fimg + p * 3, wf, iteration, x0, x);
    const double rc = (double)fref[p * 3 + c] / 255.0;
    const double x0c = c == 0 ? x0[0] : c == 1 ? x0[1] : x0[2];
    const double xc = c == 0 ? x[0] : c == 1 ? x[1] : x[2];
    if (cc_unclipped(x0c) && cc_unclipped(xc) && cc_unclipped(rc)) {
      double a[NF];
      cc_features(x[0], x[1], x[2], a);
      int k = 0;
#pragma unroll
      for (int i = 0; i < NF; ++i)
#pragma unroll
        for (int j = i; j < NF; ++j) acc[k++] += a[i] * a[j];
#pragma unroll
      for (int i = 0; i < NF; ++i) acc[55 + i] += a[i] * rc;
      acc[65] += 1.0;
    }
  }
  __shared__ double red[COLORCC_BLOCK / 64][NS];
#pragma unroll
  for (int k = 0; k < NS; ++k) wave_deposit(red, k, cc_wave_sum(acc[k]));
  __syncthreads();
  if (tid < NS) partials[(((int64_t)f * 3 + c) * nwg + blockIdx.x) * NS + tid] = waves_collect<double>(red, tid);
}

// index of Gram entry (i, j), i <= j, in the upper-triangle row-major order of COLORCC_SUMS
__device__ inline int cc_tri(int i, int j) { return i * NF - i * (i - 1) / 2 + (j - i); }

__global__ __launch_bounds__(64) void colorcc_solve_kernel(int nwg, const double* __restrict__ partials, int iteration,
                                                          double* __restrict__ weights, double* __restrict__ out,
                                                          double* __restrict__ sums) {
  const int c = blockIdx.x, f = blockIdx.y, tid = threadIdx.x;
  __shared__ double S[NS], A[NF][NF], V[NF][NF], d[NF], y[NF];
  const double* part = partials + ((int64_t)f * 3 + c) * nwg * NS;
  for (int k = tid; k < NS; k += 64) {
    double s = 0.0;
    for (int w = 0; w < nwg; ++w) s += part[(int64_t)w * NS + k];
    S[k] = s;
  }
  __syncthreads();
  if (sums != nullptr) {
    for (int k = tid; k < NS; k += 64) sums[((int64_t)f * 3 + c) * NS + k] = S[k];
    return;
  }
  if (tid == 0) out[(int64_t)f * COLORCC_OUT + 2 + iteration * 3 + c] = S[65];
  if (tid < NF) {
    const double g = S[cc_tri(tid, tid)];
    d[tid] = g > 0.0 ? 1.0 / sqrt(g) : 1.0;
  }
  __syncthreads();
  for (int e = tid; e < NF * NF; e += 64) {
    const int i = e / NF, j = e % NF;
    A[i][j] = S[i <= j ? cc_tri(i, j) : cc_tri(j, i)] * d[i] * d[j];
    V[i][j] = i == j ? 1.0 : 0.0;
  }
  __syncthreads();
  for (int sweep = 0; sweep < 12; ++sweep) {
    for (int p = 0; p < NF - 1; ++p) {
      for (int q = p + 1; q < NF; ++q) {
        const double app = A[p][p], aqq = A[q][q], apq = A[p][q];
        double cs = 1.0, sn = 0.0;
        if (apq != 0.0) {
          const double theta = (aqq - app) / (2.0 * apq);
          const double t = copysign(1.0, theta) / (fabs(theta) + sqrt(theta * theta + 1.0));
          cs = 1.0 / sqrt(t * t + 1.0);
          sn = t * cs;
        }
        __syncthreads();                                     // every thread has read the pivot
        if (tid < NF) {                                      // A <- A J, V <- V J (columns p, q)
          const double akp = A[tid][p], akq = A[tid][q];
          A[tid][p] = cs * akp - sn * akq;
          A[tid][q] = sn * akp + cs * akq;
          const double vkp = V[tid][p], vkq = V[tid][q];
          V[tid][p] = cs * vkp - sn * vkq;
          V[tid][q] = sn * vkp + cs * vkq;
        }
        __syncthreads();
        if (tid < NF) {                                      // A <- J^T A (rows p, q)
          const double apk = A[p][tid], aqk = A[q][tid];
          A[p][tid] = cs * apk - sn * aqk;
          A[q][tid] = sn * apk + cs * aqk;
        }
        __syncthreads();
      }
    }
  }
  double lmax = 0.0;
  for (int i = 0; i < NF; ++i) lmax = fmax(lmax, A[i][i]);
  if (tid < NF) {                                            // y_i = v_i . (d * rhs) / lambda_i, or 0 below the cut-off
    const double lam = A[tid][tid];
    double s = 0.0;
    for (int k = 0; k < NF; ++k) s += V[k][tid] * (d[k] * S[55 + k]);
    y[tid] = (lam > COLORCC_RANK_CUTOFF * lmax && lam > 0.0) ? s / lam : 0.0;
  }
  __syncthreads();
  if (tid < NF) {
    double z = 0.0;
    for (int i = 0; i < NF; ++i) z += V[tid][i] * y[i];
    z *= d[tid];
    weights[((int64_t)f * COLORCC_ITERS + iteration) * NW + c * NF + tid] = isfinite(z) ? z : 0.0;
  }
}

__global__ __launch_bounds__(COLORCC_BLOCK) void colorcc_apply_kernel(
    int64_t n_pixels, int nwg, const float* __restrict__ img, const uint8_t* __restrict__ ref, const double* __restrict__ weights,
    int quantize, double* __restrict__ rgb_cc, uint8_t* __restrict__ cc_u8, double* __restrict__ sse_partials) {
  const int f = blockIdx.y, tid = threadIdx.x;
  const int64_t base = (int64_t)f * n_pixels * 3;
  const double* wf = weights + (int64_t)f * COLORCC_ITERS * NW;
  double sse = 0.0;
  for (int64_t p = (int64_t)blockIdx.x * COLORCC_BLOCK + tid; p < n_pixels; p += (int64_t)nwg * COLORCC_BLOCK) {
    double x0[3], x[3];
    cc_current(img + base + p * 3, wf, COLORCC_ITERS, x0, x);
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const int64_t o = base + p * 3 + c;
      if (rgb_cc != nullptr) rgb_cc[o] = x[c];
      if (cc_u8 != nullptr) cc_u8[o] = (uint8_t)(x[c] * 255.0);          // x in [0, 1]: truncation, as the PNG writer's
      const double q = quantize ? rint(x[c] * 255.0) / 255.0 : x[c];
      const double e = q - (double)ref[o] / 255.0;
      sse += e * e;
    }
  }
  __shared__ double red[COLORCC_BLOCK / 64][1];
  wave_deposit(red, 0, cc_wave_sum(sse));
  __syncthreads();
  if (tid == 0) sse_partials[(int64_t)f * nwg + blockIdx.x] = waves_collect<double>(red, 0);
}

__global__ __launch_bounds__(64) void colorcc_finish_kernel(int n_frames, int64_t n_pixels, int nwg,
                                                           const double* __restrict__ sse_partials, double* __restrict__ out) {
  const int f = blockIdx.x * 64 + threadIdx.x;
  if (f >= n_frames) return;
  double s = 0.0;
  for (int w = 0; w < nwg; ++w) s += sse_partials[(int64_t)f * nwg + w];
  out[(int64_t)f * COLORCC_OUT] = s;
  out[(int64_t)f * COLORCC_OUT + 1] = (double)n_pixels * 3.0;
}

}  // namespace

void launch_colorcc_accumulate(hipStream_t st, int n_frames, int64_t n_pixels, int nwg, const float* img, const uint8_t* ref,
                               const double* weights, int iteration, double* partials) {
  colorcc_accumulate_kernel<<<dim3(nwg, 3, n_frames), COLORCC_BLOCK, 0, st>>>(n_pixels, nwg, img, ref, weights, iteration, partials);
}

void launch_colorcc_solve(hipStream_t st, int n_frames, int nwg, const double* partials, int iteration, double* weights,
                          double* out, double* sums) {
  colorcc_solve_kernel<<<dim3(3, n_frames), 64, 0, st>>>(nwg, partials, iteration, weights, out, sums);
}

void launch_colorcc_apply(hipStream_t st, int n_frames, int64_t n_pixels, int nwg, const float* img, const uint8_t* ref,
                          const double* weights, int quantize, double* rgb_cc, uint8_t* cc_u8, double* sse_partials) {
  colorcc_apply_kernel<<<dim3(nwg, n_frames), COLORCC_BLOCK, 0, st>>>(n_pixels, nwg, img, ref, weights, quantize, rgb_cc, cc_u8,
                                                                     sse_partials);
}

void launch_colorcc_finish(hipStream_t st, int n_frames, int64_t n_pixels, int nwg, const double* sse_partials, double* out) {
  colorcc_finish_kernel<<<(n_frames + 63) / 64, 64, 0, st>>>(n_frames, n_pixels, nwg, sse_partials, out);
}

// The line-of-sight term on the weights of one level's rays (include/raylos_hip.h).  float64 from the float32 inputs
// on, the comparisons and the band's bounds in float32 as written, no atomics, compiled with -ffp-contract=off.
//
//   rays    grid ceil(n / 4), 256 threads: one wave per ray.  Lane t takes samples t, t + 64, ...: the loads of the w and z rows are
//           coalesced (the interval's far edge z[s + 1] is the neighbouring lane's load, from the same lines).  A sample's term
//           needs nothing of the rest of the ray, so the lane forms it and its gradient entry g_w[r, s] = float32(float64(entry) +
//           lambda * term / n) in the same pass, a plain load and store; erf is evaluated only for an interval that touches the
//           band.  wave_sum gives L_r and front_r; lane 0 writes them and the ray's class.  An unsupervised ray leaves as a whole
//           wave after lane 0 has written zeros, its row of g_w untouched.
//   finish  one workgroup of 1024 threads: thread t adds rays t, t + 1024, ... in ascending order (L_r, front_r, supervised;
//           float64), hipdev::lds_tree_sum over the workgroup; thread 0 divides by n, writes values and stats and applies the fold.
// Every tree depends on n and S alone, so equal inputs give equal bits.
#include <math.h>
#include "raylos_kernels.h"
#include "hip_device.h"

namespace {

using hipdev::wave_sum, hipdev::lds_tree_sum;

constexpr int RPB = RAYLOS_RAYS_PER_BLOCK, FIN = RAYLOS_FINISH_BLOCK, SUMS = 3;

// Phi(x) = 0.5 (1 + erf(x / sqrt 2))
__device__ __forceinline__ double std_normal_cdf(double x) { return 0.5 * (1.0 + erf(x / sqrt(2.0))); }

__global__ __launch_bounds__(RPB * 64) void raylos_rays_kernel(RayLosArgs a) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int ray = blockIdx.x * RPB + wave;
  if (ray >= a.n) return;                                    // (whole waves leave: no shuffle below is divergent)
  const int S = a.S;
  const float hif = a.hi[ray], pf = a.p[ray], sf = a.sigma[ray];
  const bool sup = pf > 0.f && pf < hif && sf > 0.f;         // a NaN anywhere is no supervised ray; wave-uniform
  if (!sup) {
    if (lane == 0) {
      a.ws_los[ray] = 0.0;
      a.ws_front[ray] = 0.0;
      a.ws_sup[ray] = 0;
    }
    return;
  }
  const float lo_b = pf - sf, hi_b = pf + sf;                // one float32 rounding each
  const double p = (double)pf, sd = (double)sf / 3.0, scale = a.lambda, nd = (double)a.n;
  const float* __restrict__ wrow = a.w + (size_t)ray * S;
  const float* __restrict__ zrow = a.z + (size_t)ray * S;
  float* gw = a.g_w ? a.g_w + (size_t)ray * S : nullptr;
  double los = 0.0, front = 0.0;
  for (int s = lane; s < S; s += 64) {
    const float e0 = zrow[s], e1 = s + 1 < S ? zrow[s + 1] : hif;
    const bool empty = e1 <= lo_b, near = !empty && e0 < hi_b;
    if (!(empty || near)) continue;                          // behind the band: no term, the entry keeps its bits
    const double w = (double)wrow[s];
    double grad;
    if (near) {
      const double k = std_normal_cdf(((double)e1 - p) / sd) - std_normal_cdf(((double)e0 - p) / sd);
      const double d = w - k;
      los += d * d;
      grad = 2.0 * d;
    } else {
      los += w * w;
      front += w;
      grad = 2.0 * w;
    }
    if (gw) gw[s] = (float)((double)gw[s] + scale * grad / nd);
  }
  los = wave_sum(los);
  front = wave_sum(front);
  if (lane == 0) {
    a.ws_los[ray] = los;
    a.ws_front[ray] = front;
    a.ws_sup[ray] = 1;
  }
}

__global__ __launch_bounds__(FIN) void raylos_finish_kernel(RayLosArgs a) {
  __shared__ double sh[SUMS][FIN];
  const int tid = threadIdx.x, n = a.n;
  double s[SUMS] = {0.0, 0.0, 0.0};                          // sum of L_r, of front_r; supervised rays
  for (int r = tid; r < n; r += FIN) {
    s[0] += a.ws_los[r];
    s[1] += a.ws_front[r];
    s[2] += (double)a.ws_sup[r];
  }
  lds_tree_sum<FIN, SUMS>(sh, s);
  if (tid == 0) {
    const float v = (float)(sh[0][0] / (double)n);
    a.values[0] = v;
    a.stats[0] = (float)sh[2][0];
    a.stats[1] = (float)sh[1][0];
    if (a.fold_total) *a.fold_total += (float)(a.lambda * (double)v);
  }
}

}  // namespace

void launch_raylos_rays(hipStream_t st, const RayLosArgs& a) {
  raylos_rays_kernel<<<(a.n + RPB - 1) / RPB, RPB * 64, 0, st>>>(a);
}

void launch_raylos_finish(hipStream_t st, const RayLosArgs& a) {
  raylos_finish_kernel<<<1, FIN, 0, st>>>(a);
}

// The Gaussian negative-log-likelihood depth loss of all levels of a step (include/depthgnll_hip.h).  float64 from
// the float32 inputs on, no atomics, compiled with -ffp-contract=off.
//
//   rays    grid (ceil(n / 4), n_levels), 256 threads: one wave per (ray r, level l), as mip360_depth_rays.hip.
//           pass A  lane t takes samples t, t + 64, ... in ascending order (coalesced loads of the w row and of the x row, or of the
//                   two edges of an interval) and keeps M0, M1 and sum w (x - D)^2 as float64; the three are added over the wave by
//                   the xor butterfly, so every lane holds the same bits and the gate below is wave-uniform.  The ray's class
//                   (supervised, gated, clamped) and its l_r (0 when not gated) go to the workspace's [l, r].
//           pass B  (gated rays) the same samples again: g_w[r, s] is owned by the lane that read sample s, g_d[r] by lane 0:
//                   entry = float32(float64(entry) + scale * gradient), a plain load and store.  A ray that is not gated leaves
//                   before it and touches no gradient entry.
//   finish  one workgroup of 1024 threads, level after level: thread t adds the level's rays t, t + 1024, ... in ascending order
//           (l_r and the three class counts, float64), the wave butterfly, the sixteen waves in wave order through LDS
//           (hipdev::wave_deposit / waves_collect); thread 0 divides by n, writes values and stats and, after the last level, the
//           folds (hipdev::fold_levels).
// Every tree depends on n, the sample counts and n_levels alone, so equal inputs give equal bits.
#include <math.h>
#include "depthgnll_kernels.h"
#include "hip_device.h"

namespace {

using hipdev::wave_sum, hipdev::wave_deposit, hipdev::waves_collect;

constexpr int RPB = DEPTHGNLL_RAYS_PER_BLOCK, FIN = DEPTHGNLL_FINISH_BLOCK, FIN_WAVES = FIN / 64, SUMS = 4;
constexpr double VAR_EPS = 1e-5, VAR_MIN = 1e-3;             // the reference's + 1e-5; GaussianNLLLoss(eps = 0.001)

// sample s of a ray: its position, from the row of positions or from the two edges of its interval
__device__ inline double position(const float* __restrict__ row, int s, bool edges) {
  if (edges) return (double)(0.5f * (row[s] + row[s + 1]));
  return (double)row[s];
}

__global__ __launch_bounds__(RPB * 64) void depthgnll_rays_kernel(DepthGnllArgs a) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int ray = blockIdx.x * RPB + wave, l = blockIdx.y;
  if (ray >= a.n) return;                                    // (whole waves leave: no shuffle below is divergent)
  const int n = a.n, S = a.S[l];
  const bool edges = a.edges != 0;
  const size_t slot = (size_t)l * n + ray;
  const float pf = a.p[ray], sf = a.sigma[ray];
  const bool sup = pf > 0.f && sf > 0.f && (a.limit == nullptr || pf < a.limit[ray]);     // a NaN prior is no supervision
  if (!sup) {                                                // wave-uniform
    if (lane == 0) { a.ws_loss[slot] = 0.0; a.ws_class[slot] = 0; }
    return;
  }
  const float* __restrict__ wrow = a.w[l] + (size_t)ray * S;
  const float* __restrict__ xrow = a.x[l] + (size_t)ray * (edges ? S + 1 : S);
  const double D = (double)a.d[l][ray], P = (double)pf, sg = (double)sf;
  // ---- pass A: the ray's three sums ----
  double m0 = 0.0, m1 = 0.0, var = 0.0;
  for (int s = lane; s < S; s += 64) {
    const double w = (double)wrow[s], x = position(xrow, s, edges), dx = x - D;
    m0 += w;
    m1 += w * x;
    var += w * (dx * dx);
  }
  m0 = wave_sum(m0); m1 = wave_sum(m1); var = wave_sum(var);
  const double V = var + VAR_EPS;
  const double diff = D - P;
  const bool gated = fabs(diff) - sg > 0.0 || sg * sg < V;   // a NaN rendering fails both comparisons: not gated
  if (!gated) {                                              // wave-uniform: every lane holds the same V
    if (lane == 0) { a.ws_loss[slot] = 0.0; a.ws_class[slot] = 1; }
    return;
  }
  const bool clamped = V < VAR_MIN;
  const double Vc = clamped ? VAR_MIN : V;
  const double gV = 0.5 * (1.0 / Vc - diff * diff / (Vc * Vc));
  const double sc = (double)a.scale[l], nd = (double)n;
  if (lane == 0) {
    a.ws_loss[slot] = 0.5 * (log(Vc) + diff * diff / Vc);
    a.ws_class[slot] = clamped ? 7 : 3;
    float* gd = a.g_d[l];
    if (gd) gd[ray] = (float)((double)gd[ray] + sc * ((diff / Vc - 2.0 * gV * (m1 - D * m0)) / nd));
  }
  // ---- pass B: the gradient entries of the ray's weights ----
  float* gw = a.g_w[l];
  if (gw == nullptr) return;
  gw += (size_t)ray * S;
  for (int s = lane; s < S; s += 64) {
    const double dx = position(xrow, s, edges) - D;
    gw[s] = (float)((double)gw[s] + sc * (gV * (dx * dx) / nd));
  }
}

__global__ __launch_bounds__(FIN) void depthgnll_finish_kernel(DepthGnllArgs a) {
  __shared__ double red[FIN_WAVES][SUMS];
  const int tid = threadIdx.x, n = a.n, L = a.n_levels;
  float n_sup_f = 0.f;
  for (int l = 0; l < L; ++l) {
    double s[SUMS] = {0.0, 0.0, 0.0, 0.0};                   // sum of l_r; supervised, gated, clamped rays
    for (int r = tid; r < n; r += FIN) {
      const size_t slot = (size_t)l * n + r;
      const int c = a.ws_class[slot];
      s[0] += a.ws_loss[slot];
      s[1] += (double)(c & 1);
      s[2] += (double)((c >> 1) & 1);
      s[3] += (double)((c >> 2) & 1);
    }
#pragma unroll
    for (int k = 0; k < SUMS; ++k) wave_deposit(red, k, wave_sum(s[k]));
    __syncthreads();
    if (tid == 0) {
#pragma unroll
      for (int k = 0; k < SUMS; ++k) s[k] = waves_collect<double>(red, k);
      const float v = (float)(s[0] / (double)n);
      a.values[l] = v;
      a.stats[l * DEPTHGNLL_STATS_ROW] = (float)s[1];
      a.stats[l * DEPTHGNLL_STATS_ROW + 1] = (float)s[2];
      a.stats[l * DEPTHGNLL_STATS_ROW + 2] = (float)s[3];
      n_sup_f = (float)s[1];
    }
    __syncthreads();                                         // red is free for the next level
  }
  if (tid == 0) hipdev::fold_levels(a.folds, a.values, a.scale, L, n_sup_f);
}

}  // namespace

void launch_depthgnll_rays(hipStream_t st, const DepthGnllArgs& a) {
  depthgnll_rays_kernel<<<dim3((a.n + RPB - 1) / RPB, a.n_levels), RPB * 64, 0, st>>>(a);
}

void launch_depthgnll_finish(hipStream_t st, const DepthGnllArgs& a) {
  depthgnll_finish_kernel<<<1, FIN, 0, st>>>(a);
}

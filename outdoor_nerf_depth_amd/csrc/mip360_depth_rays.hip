// Per-ray DS-NeRF ('kl_ray') and Urban-Radiance-Fields ('urf_ray') depth losses of ALL sampling levels of a step.
// The per-element expressions are the ones depth_klurf_kernel evaluates (internal/depth_loss.py:24, 44-60); the reduction is the
// one the two losses are defined with -- sum over a ray's samples, times that ray's mask, mean over the rays -- instead of
// upstream's `.sum(-2)` over the ray axis, so every batch size and every per-level sample count works:
//   steps = 0.5f * (t[s] + t[s+1]), len = (t[s+1] - t[s]) * |dir|, m_r = sup_r > 0, gt = sup_r
//   kl_ray  = (1/n) sum_r m_r sum_s -log(w + 1e-7) * exp(-(steps - gt)^2 / (2 sigma)) * len
//   urf_ray = (1/n) sum_r m_r [ (gt - dm_r)^2 + sum_s near (w - N(steps - gt; 0, sigma / 3))^2 + sum_s empty w^2 ]
//     near = steps <= gt + sigma && steps >= gt - sigma, empty = steps < gt - sigma: float32 comparisons of singly rounded
//     operands (this file is built with -ffp-contract=off), so a float32 reference forms the same booleans.
//
//   depth_rays_kernel       : grid (ceil(n / 4), n_levels), one wave per (ray, level), lane = sample.  Coalesced loads of w and
//       of the two edges, accurate expf / logf, the lane's term; every gradient element is owned by one lane (g_w[r,s] by lane
//       s, g_dm[r] by lane 0) and is ACCUMULATED with a plain load + store.  The ray's sum is a fixed xor butterfly; lane 0
//       writes workspace[level * n + ray].  An unsupervised ray writes 0 there and touches no gradient entry.
//   depth_rays_reduce_kernel: one workgroup of 1024 threads, float64 strided partials, then hipdev::lds_tree_sum of the
//       levels side by side -> values[level] = sum / n, and, when asked, the fold into the six scalars of mip360_losses.
// No atomics anywhere; both summation trees depend on the shapes alone, so equal inputs give equal bits.
#include <math.h>
#include "mip360_device.h"
#include "mip360_launch.h"

namespace mip360 {

using mip360dev::wave_sum, mip360dev::lds_tree_sum;

constexpr int DR_RPB = 4;            // rays (waves) per workgroup
constexpr int DR_MAX_LEVELS = 4;

struct DepthRaysArgs {
  int type, n, n_levels;
  int S[DR_MAX_LEVELS];
  const float* w[DR_MAX_LEVELS]; const float* td[DR_MAX_LEVELS]; const float* dm[DR_MAX_LEVELS];
  const float* sup; const float* dirs;
  float sigma; float scale[DR_MAX_LEVELS];
  float* g_w[DR_MAX_LEVELS]; float* g_dm[DR_MAX_LEVELS];
  float* ws;
};

__global__ __launch_bounds__(256) void depth_rays_kernel(DepthRaysArgs a) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int ray = blockIdx.x * DR_RPB + wave, lvl = blockIdx.y;
  if (ray >= a.n) return;                                            // (whole waves leave: no shuffle below is divergent)
  const int n = a.n, S = a.S[lvl];
  const float gt = a.sup[ray];
  if (!(gt > 0.f)) {                                                 // wave-uniform: the ray's gradient entries stay as they are
    if (lane == 0) a.ws[(size_t)lvl * n + ray] = 0.f;
    return;
  }
  const float sigma = a.sigma, scale = a.scale[lvl], nf = (float)n;
  const bool ok = lane < S;
  float term = 0.f, g = 0.f;
  if (ok) {
    const float* td = a.td[lvl] + (size_t)ray * (S + 1);
    const float t0 = td[lane], t1 = td[lane + 1], wi = a.w[lvl][(size_t)ray * S + lane];
    const float step = 0.5f * (t0 + t1), d = step - gt;
    if (a.type == MIP360_DEPTH_KL_RAY) {
      const float dx = a.dirs[ray * 3], dy = a.dirs[ray * 3 + 1], dz = a.dirs[ray * 3 + 2];
      const float len = (t1 - t0) * sqrtf(dx * dx + dy * dy + dz * dz);
      const float e = expf(-(d * d) / (2.f * sigma)) * len;
      term = -logf(wi + 1e-7f) * e;
      g = -e / (wi + 1e-7f);
    } else {
      const float usig = sigma / 3.f;                                // URF_SIGMA_SCALE_FACTOR
      const float log_norm = logf(usig) + logf(sqrtf(2.f * 3.14159265358979323846f));
      const bool near = step <= gt + sigma && step >= gt - sigma, empty = step < gt - sigma;
      const float pdf = expf(-(d * d) / (2.f * usig * usig) - log_norm);
      if (near) { term += (wi - pdf) * (wi - pdf); g += 2.f * (wi - pdf); }
      if (empty) { term += wi * wi; g += 2.f * wi; }
    }
    float* gw = a.g_w[lvl];
    if (gw) gw[(size_t)ray * S + lane] += scale * (g / nf);          // the written order: d value / d w, then the level's weight
  }
  float sum = wave_sum(term);
  if (lane == 0) {
    if (a.type == MIP360_DEPTH_URF_RAY) {
      const float diff = gt - a.dm[lvl][ray];
      sum = diff * diff + sum;
      float* gd = a.g_dm[lvl];
      if (gd) gd[ray] += scale * (-2.f * diff / nf);
    }
    a.ws[(size_t)lvl * n + ray] = sum;
  }
}

struct DepthRaysReduceArgs {
  int n, n_levels;
  float scale[DR_MAX_LEVELS];
  const float* ws; float* values; float* scalars;
};

__global__ __launch_bounds__(1024) void depth_rays_reduce_kernel(DepthRaysReduceArgs a) {
  __shared__ double sh[DR_MAX_LEVELS][1024];
  const int n = a.n, L = a.n_levels;
  double p[DR_MAX_LEVELS] = {0, 0, 0, 0};
  for (int r = threadIdx.x; r < n; r += blockDim.x) {
#pragma unroll
    for (int l = 0; l < DR_MAX_LEVELS; ++l)
      if (l < L) p[l] += (double)a.ws[(size_t)l * n + r];
  }
  lds_tree_sum(sh, p);
  if (threadIdx.x == 0) {
    float total = 0.f, prop = 0.f, last = 0.f;
    for (int l = 0; l < L; ++l) {                                    // level order: proposal levels first, the NeRF level last
      const float v = (float)(sh[l][0] / (double)n);
      a.values[l] = v;
      total += a.scale[l] * v;
      if (l < L - 1) prop += v;
      else last = v;
    }
    if (a.scalars) {                                                 // the six scalars mip360_losses left (depth type 0)
      a.scalars[2] = last;
      a.scalars[5] = prop;
      a.scalars[0] += total;
    }
  }
}

}  // namespace mip360

using namespace mip360;

void mip360_launch_depth_rays(hipStream_t st, int type, int n, int n_levels, const int* S, const float* const* w,
                              const float* const* td, const float* sup, const float* const* dm, const float* dirs, float sigma,
                              const float* scale, float* values, float* const* g_w, float* const* g_dm, float* scalars,
                              float* ws) {
  DepthRaysArgs a{};
  DepthRaysReduceArgs r{};
  a.type = type; a.n = n; a.n_levels = n_levels; a.sup = sup; a.dirs = dirs; a.sigma = sigma; a.ws = ws;
  for (int l = 0; l < n_levels; ++l) {
    a.S[l] = S[l]; a.w[l] = w[l]; a.td[l] = td[l]; a.scale[l] = scale[l];
    a.dm[l] = dm ? dm[l] : nullptr;
    a.g_w[l] = g_w ? g_w[l] : nullptr;
    a.g_dm[l] = g_dm ? g_dm[l] : nullptr;
    r.scale[l] = scale[l];
  }
  r.n = n; r.n_levels = n_levels; r.ws = ws; r.values = values; r.scalars = scalars;
  hipLaunchKernelGGL(depth_rays_kernel, dim3((n + DR_RPB - 1) / DR_RPB, n_levels), dim3(256), 0, st, a);
  hipLaunchKernelGGL(depth_rays_reduce_kernel, dim3(1), dim3(1024), 0, st, r);
}

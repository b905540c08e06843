// The scale-and-shift-invariant depth loss of all levels of a step (include/depthssi_hip.h).  float64 from the float32
// inputs on, no atomics, compiled with -ffp-contract=off.
//
//   groups  grid (n_groups, n_levels), 256 threads: one workgroup per (group k, level l).
//           pass A  thread t takes rays t, t + 256, ... in ascending order (coalesced loads of g, p, d) and keeps N, Sd, Sdd, Sp,
//                   Sdp of the group's supervised rays and N_sup of all groups as float64; the six are added over the wave by the
//                   xor butterfly and over the four waves in wave order (hipdev::wave_deposit / waves_collect).  Thread 0 decides
//                   `fitted`, solves for w and q, writes the group's fit row and hands w, q, D and `fitted` to the others through LDS.
//           pass B  (fitted groups) the same rays again: r = w d + q - p, the thread's sum of r^2, and the ray's gradient entry,
//                   which this thread of this workgroup alone owns (a ray is in one group): entry = float32(float64(entry) +
//                   scale * (2 w r / D)), a plain load and store.  The sums of r^2 are added like pass A's; thread 0 writes the
//                   workspace's [l, k].  Workgroup (0, l) also writes N_sup of level l (every workgroup has counted it).
//   finish  one workgroup of 256 threads, level after level: thread t adds the level's groups t, t + 256, ... in ascending order
//           (sum of r^2; N of the fitted groups), the same wave / LDS tree, thread 0 divides by D, writes values and stats and,
//           after the last level, the folds (hipdev::fold_levels).
// Both trees depend on n, n_groups and n_levels alone, so equal inputs give equal bits.
#include "depthssi_kernels.h"
#include "hip_device.h"

namespace {

using hipdev::wave_sum, hipdev::wave_deposit, hipdev::waves_collect;

constexpr int BLOCK = DEPTHSSI_BLOCK, WAVES = BLOCK / 64, SUMS = 6;
constexpr double FLAT = 1e-8;                                // N Sdd - Sd^2 <= FLAT N Sdd: the render is constant in the group

// v[0..K) summed over the workgroup; every thread returns with the same bits.  red is free on return.
template <int K>
__device__ inline void block_sum(double (&v)[K], double (&red)[WAVES][SUMS]) {
#pragma unroll
  for (int k = 0; k < K; ++k) wave_deposit(red, k, wave_sum(v[k]));
  __syncthreads();
#pragma unroll
  for (int k = 0; k < K; ++k) v[k] = waves_collect<double>(red, k);
  __syncthreads();
}

__device__ inline double divisor(int norm, int n, double n_sup) {
  if (norm == DEPTHSSI_NORM_ALL) return (double)n;
  return n_sup > 1.0 ? n_sup : 1.0;
}

__global__ __launch_bounds__(BLOCK) void depthssi_groups_kernel(DepthSsiArgs a) {
  __shared__ double red[WAVES][SUMS];
  __shared__ double solved[3];                               // w, q, D
  __shared__ int fitted_sh;
  const int k = blockIdx.x, l = blockIdx.y, tid = threadIdx.x;
  const int n = a.n, G = a.n_groups;
  const float* __restrict__ d = a.d[l];
  const float* __restrict__ p = a.p;
  const int32_t* __restrict__ g = a.g;
  const size_t gs = (size_t)a.g_stride;
  // ---- pass A: the group's five sums and the count of all supervised rays ----
  double s[SUMS] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};           // N, Sd, Sdd, Sp, Sdp, N_sup
  for (int i = tid; i < n; i += BLOCK) {
    const int gi = g ? g[(size_t)i * gs] : 0;
    const float pf = p[i], df = d[i];
    if (!(pf > 0.f) || gi < 0 || gi >= G) continue;          // a NaN prior is no supervision
    s[5] += 1.0;
    if (gi != k) continue;
    const double D = (double)df, P = (double)pf;
    s[0] += 1.0;
    s[1] += D;
    s[2] += D * D;
    s[3] += P;
    s[4] += D * P;
  }
  block_sum<SUMS>(s, red);
  if (tid == 0) {
    const double N = s[0], Sd = s[1], Sdd = s[2], Sp = s[3], Sdp = s[4];
    const double var = N * Sdd - Sd * Sd;
    const bool fitted = N >= (double)a.min_rays && var > FLAT * N * Sdd;      // a NaN depth in the group: not fitted
    double w = 0.0, q = 0.0;
    if (fitted) {
      w = (N * Sdp - Sd * Sp) / var;
      q = (Sp - w * Sd) / N;
    }
    solved[0] = w; solved[1] = q; solved[2] = divisor(a.norm, n, s[5]);
    fitted_sh = fitted ? 1 : 0;
    float* row = a.fit + ((size_t)l * G + k) * DEPTHSSI_FIT_ROW;
    row[0] = (float)w; row[1] = (float)q; row[2] = (float)N; row[3] = fitted ? 1.f : 0.f;
    if (k == 0) a.ws[(size_t)a.n_levels * G + l] = s[5];
  }
  __syncthreads();
  if (!fitted_sh) {                                          // (uniform over the workgroup)
    if (tid == 0) a.ws[(size_t)l * G + k] = 0.0;
    return;
  }
  // ---- pass B: residuals, their squares, the gradient entries this workgroup owns ----
  const double w = solved[0], q = solved[1], Dn = solved[2];
  const double sc = (double)a.scale[l];
  float* __restrict__ gb = a.grads[l];
  double r2[1] = {0.0};
  for (int i = tid; i < n; i += BLOCK) {
    const int gi = g ? g[(size_t)i * gs] : 0;
    const float pf = p[i];
    if (!(pf > 0.f) || gi != k) continue;
    const double r = w * (double)d[i] + q - (double)pf;
    r2[0] += r * r;
    if (gb) gb[i] = (float)((double)gb[i] + sc * (2.0 * w * r / Dn));
  }
  block_sum<1>(r2, red);
  if (tid == 0) a.ws[(size_t)l * G + k] = r2[0];
}

__global__ __launch_bounds__(BLOCK) void depthssi_finish_kernel(DepthSsiArgs a) {
  __shared__ double red[WAVES][SUMS];
  const int tid = threadIdx.x, G = a.n_groups, L = a.n_levels;
  float n_sup_f = 0.f;
  for (int l = 0; l < L; ++l) {
    double s[2] = {0.0, 0.0};                                // sum of r^2, supervised rays in fitted groups
    for (int k = tid; k < G; k += BLOCK) {
      s[0] += a.ws[(size_t)l * G + k];
      const float* row = a.fit + ((size_t)l * G + k) * DEPTHSSI_FIT_ROW;
      if (row[3] != 0.f) s[1] += (double)row[2];
    }
    block_sum<2>(s, red);
    if (tid != 0) continue;                                  // (no barrier below this line in the iteration)
    const double n_sup = a.ws[(size_t)L * G + l];
    const float v = (float)(s[0] / divisor(a.norm, a.n, n_sup));
    a.values[l] = v;
    a.stats[l * DEPTHSSI_STATS_ROW] = (float)n_sup;
    a.stats[l * DEPTHSSI_STATS_ROW + 1] = (float)s[1];
    n_sup_f = (float)n_sup;
  }
  if (tid == 0) hipdev::fold_levels(a.folds, a.values, a.scale, L, n_sup_f);
}

}  // namespace

void launch_depthssi_groups(hipStream_t st, const DepthSsiArgs& a) {
  depthssi_groups_kernel<<<dim3(a.n_groups, a.n_levels), BLOCK, 0, st>>>(a);
}

void launch_depthssi_finish(hipStream_t st, const DepthSsiArgs& a) {
  depthssi_finish_kernel<<<1, BLOCK, 0, st>>>(a);
}

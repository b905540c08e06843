// Depth-guided fine sampling of one level's rays (include/depthguide_hip.h).  float64 from the float32 inputs on, no
// atomics, compiled with -ffp-contract=off.
//
//   merge   grid ceil(n / 4), 256 threads: one wave per ray, and a wave only ever touches its own rows of the two LDS arrays, so the
//           kernel has no workgroup barrier -- the lanes of a wave hand over through LDS with lds_wave_sync().
//           moments  (rays without a usable prior)  lane l adds samples l, l + 64, ... of the previous level in ascending order
//                    (W = sum w and sum w z together, then sum w (z - mu)^2), the 64 lanes by the xor butterfly: every lane the
//                    same bits, trees of S_prev alone.
//           guide    lane l computes depths l, l + 64, ...: the stratified quantile, the table's linear interpolation, the clamp;
//                    float32(g) goes behind zin in s_z, into s_g (padded with +inf to a power of two) and to `guide`.
//           sort     a bitonic network over s_g.
//           merge    zin ascending and no NaN anywhere: an element's place is its own index plus its binary-search count in the
//                    other list, old before new on ties (the stable sort of the concatenation; values only).  Anything else: a
//                    stable rank sort of s_z in numpy's order (NaNs last).
// 16 KiB of LDS per workgroup (ten workgroups fit a CU's 160 KiB; the launch bound of 256 threads allows eight): as for
// sample_pdf_kernel a level's 1024 rays are 256 workgroups, one per CU, and the launch is bound by latency, not by occupancy.
#include <math.h>
#include "depthguide_kernels.h"
#include "hip_device.h"

namespace {

using hipdev::wave_sum;
using nerfpp::philox_uniform;

constexpr int RPB = DEPTHGUIDE_RAYS_PER_BLOCK, MAXM = DEPTHGUIDE_MAX_MERGED, K = DEPTHGUIDE_TABLE_K;
constexpr double W_MIN = 1e-10;

// LDS hand-off between the lanes of ONE wave (its LDS operations retire in order; the compiler must not reorder across)
__device__ __forceinline__ void lds_wave_sync() {
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  __builtin_amdgcn_wave_barrier();
}

// numpy's sort order: a strictly before b, a NaN after every number
__device__ __forceinline__ bool before(float a, float b) { return a < b || (b != b && a == a); }

__global__ __launch_bounds__(RPB * 64) void depthguide_merge_kernel(DepthGuideArgs a) {
  __shared__ float s_z[RPB][MAXM];                           // cat(zin, float32(g)), in that order
  __shared__ float s_g[RPB][MAXM];                           // float32(g) padded to a power of two, then sorted
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int ray = blockIdx.x * RPB + wave;
  if (ray >= a.n) return;                                    // (whole waves leave: no shuffle below is divergent)
  const int S_prev = a.S_prev, S_in = a.S_in, G = a.G, S_tot = S_in + G;
  float* zs = s_z[wave];
  float* nb = s_g[wave];
  const float* __restrict__ zin = a.zin + (size_t)ray * S_in;
  for (int i = lane; i < S_in; i += 64) zs[i] = zin[i];

  // ---- the ray's Gaussian (wave-uniform) ----
  const double lo = (double)a.lo[ray], hi = (double)a.hi[ray];
  const double p = a.prior ? (double)a.prior[ray] : 0.0;
  const double s = a.prior_std ? (double)a.prior_std[ray] : a.std_const;
  const double s_eff = s < a.min_std ? a.min_std : s;
  const bool guided = p > 0.0 && p < hi && s_eff > 0.0 && s_eff < (double)__builtin_inff();
  int mode = 0;
  double mu = p, sd = s_eff;
  if (!guided) {
    const float* __restrict__ zp = a.zp + (size_t)ray * S_prev;
    const float* __restrict__ wp = a.wp + (size_t)ray * S_prev;
    double sw = 0.0, swz = 0.0;
    for (int i = lane; i < S_prev; i += 64) {
      const double w = (double)wp[i];
      sw += w;
      swz += w * (double)zp[i];
    }
    const double W = wave_sum(sw), B = wave_sum(swz);
    if (W > W_MIN) {
      mode = 1;
      mu = B / W;
      double sv = 0.0;
      for (int i = lane; i < S_prev; i += 64) {
        const double d = (double)zp[i] - mu;
        sv += (double)wp[i] * (d * d);
      }
      sd = sqrt(wave_sum(sv) / W);
      sd = sd < a.min_std ? a.min_std : sd;
    } else {
      mode = 2;
    }
  }
  if (lane == 0) a.mode[ray] = mode;

  // ---- the G new depths ----
  int P2 = 1;
  while (P2 < G) P2 <<= 1;                                   // G < 512, so P2 <= 512
  const double Gd = (double)G;
  float* guide = a.guide ? a.guide + (size_t)ray * G : nullptr;
  bool clean = true;                                         // no NaN among this lane's new depths
  for (int j = lane; j < P2; j += 64) {
    float gf = __builtin_inff();
    if (j < G) {
      const size_t e = (size_t)ray * G + j;
      const float vj = a.rng.enabled ? philox_uniform(a.rng, (uint32_t)DEPTHGUIDE_RNG_STREAM, (uint64_t)e) : a.v ? a.v[e] : 0.5f;
      const double q = ((double)j + (double)vj) / Gd;
      double g;
      if (mode == 2) {
        g = lo + (hi - lo) * q;
      } else {
        const double t = q * (double)K;
        // (a uniform in [0, 1) keeps t in [0, K); anything else still reads inside the table)
        const int i = (t >= 0.0 && t < (double)K) ? (int)t : (t >= (double)K ? K - 1 : 0);
        const double f = t - (double)i, T0 = a.table[i], T1 = a.table[i + 1];
        const double x = T0 + f * (T1 - T0);
        g = mu + sd * x;
        g = g < lo ? lo : g;
        g = g > hi ? hi : g;
      }
      gf = (float)g;
      zs[S_in + j] = gf;
      if (guide) guide[j] = gf;
      clean = clean && gf == gf;
    }
    nb[j] = gf;
  }
  lds_wave_sync();

  float* __restrict__ mo = a.z_merged + (size_t)ray * S_tot;
  bool ascending = true;                                     // zin: no NaN and no descent
  for (int i = lane; i < S_in; i += 64) {
    const float x = zs[i];
    ascending = ascending && x == x && (i + 1 >= S_in || x <= zs[i + 1]);
  }
  if (__all(ascending && clean)) {
    for (int k = 2; k <= P2; k <<= 1) {
      for (int j = k >> 1; j > 0; j >>= 1) {
        for (int t = lane; t < (P2 >> 1); t += 64) {
          const int l = ((t & ~(j - 1)) << 1) | (t & (j - 1)), h = l | j;
          const bool up = (l & k) == 0;
          const float x = nb[l], y = nb[h];
          if ((x > y) == up) { nb[l] = y; nb[h] = x; }
        }
        lds_wave_sync();
      }
    }
    for (int i = lane; i < S_in; i += 64) {                  // old depth i: + #{new < it}
      const float v = zs[i];
      int l = 0, h = G;
      while (l < h) {
        const int mid = (l + h) >> 1;
        const bool lt = nb[mid] < v;
        l = lt ? mid + 1 : l;
        h = lt ? h : mid;
      }
      mo[i + l] = v;
    }
    for (int r = lane; r < G; r += 64) {                     // r-th smallest new depth: + #{old <= it}
      const float v = nb[r];
      int l = 0, h = S_in;
      while (l < h) {
        const int mid = (l + h) >> 1;
        const bool le = zs[mid] <= v;
        l = le ? mid + 1 : l;
        h = le ? h : mid;
      }
      mo[r + l] = v;
    }
    return;
  }
  for (int e = lane; e < S_tot; e += 64) {                   // stable rank sort, values only
    const float v = zs[e];
    int rank = 0;
    for (int k = 0; k < S_tot; ++k) {
      const float o = zs[k];
      rank += (before(o, v) || (!before(v, o) && k < e)) ? 1 : 0;
    }
    mo[rank] = v;
  }
}

}  // namespace

void launch_depthguide_merge(hipStream_t st, const DepthGuideArgs& a) {
  depthguide_merge_kernel<<<(a.n + RPB - 1) / RPB, RPB * 64, 0, st>>>(a);
}

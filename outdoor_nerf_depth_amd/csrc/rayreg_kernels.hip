// The distortion and opacity regularisers on the weights of one level's rays (include/rayreg_hip.h).  float64 from
// the float32 inputs on, no atomics, compiled with -ffp-contract=off.
//
//   rays    grid ceil(n / 4), 256 threads: one wave per ray.  Lane t owns the contiguous run of R = ceil(S / 64) samples from t R
//           on (the last lanes own fewer or none), so that a sum over the samples before / after s is a sum over earlier / later
//           lanes plus a serial one inside the run.
//           pass A  the lane's totals a = sum w and b = sum w u over its run, in ascending order; sum w over the wave by the xor
//                   butterfly (every lane the same bits: the opacity term); the exclusive prefix and suffix of a and b over the
//                   lanes by fixed shuffle trees (rayreg_kernels.h).
//           pass B  the run again with the running A_s, B_s: the lane's part of dist_r, and g_w[r, s], owned by the lane that owns
//                   sample s: entry = float32(float64(entry) + term / n), a plain load and vector store.  The sum over the later
//                   samples of the run is the lane's total less the running inclusive sum (both formed in the same order, so
//                   it is exactly 0 at the run's last sample).
//           A ray with hi <= lo, or a lambda of 0, skips what it does not need; a row without a term is not touched.
//   finish  one workgroup of 1024 threads: thread t adds rays t, t + 1024, ... in ascending order (dist_r, opac_r, valid; float64),
//           hipdev::lds_tree_sum over the workgroup; thread 0 divides by n, writes values and stats and applies the fold.
// Every tree depends on n and S alone, so equal inputs give equal bits.
#include <math.h>
#include "rayreg_kernels.h"
#include "hip_device.h"

namespace {

using hipdev::wave_sum, hipdev::lds_tree_sum;

constexpr int RPB = RAYREG_RAYS_PER_BLOCK, FIN = RAYREG_FINISH_BLOCK, SUMS = 3;
constexpr double OPAC_EPS = 1e-10;

__global__ __launch_bounds__(RPB * 64) void rayreg_rays_kernel(RayRegArgs a) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int ray = blockIdx.x * RPB + wave;
  if (ray >= a.n) return;                                    // (whole waves leave: no shuffle below is divergent)
  const int S = a.S, R = (S + 63) >> 6;
  const int s0 = min(lane * R, S), s1 = min(s0 + R, S);      // the lane's run [s0, s1)
  const float lof = a.lo[ray], hif = a.hi[ray];
  const bool valid = hif > lof;                              // a NaN bound is no valid ray
  const bool dist_on = a.lambda_dist > 0.0 && valid, opac_on = a.lambda_opac > 0.0;      // wave-uniform
  const double lo = (double)lof, span = (double)hif - lo, e_end = span / span, nd = (double)a.n;
  const float* __restrict__ wrow = a.w + (size_t)ray * S;
  const float* __restrict__ zrow = a.z + (size_t)ray * S;
  float* gw = a.g_w ? a.g_w + (size_t)ray * S : nullptr;
  // ---- pass A: the lane's totals ----
  double a_l = 0.0, b_l = 0.0;
  if (dist_on) {
    double e1 = s0 < S ? ((double)zrow[s0] - lo) / span : e_end;
    for (int s = s0; s < s1; ++s) {
      const double w = (double)wrow[s], e0 = e1;
      e1 = s + 1 < S ? ((double)zrow[s + 1] - lo) / span : e_end;
      a_l += w;
      b_l += w * ((e0 + e1) / 2.0);
    }
  } else {
    for (int s = s0; s < s1; ++s) a_l += (double)wrow[s];
  }
  double opac = 0.0, term_opac = 0.0;
  if (opac_on) {
    const double o = wave_sum(a_l) + OPAC_EPS, lg = log(o);
    opac = -(o * lg);
    term_opac = a.lambda_opac * -(lg + 1.0);
  }
  double dist = 0.0;
  if (dist_on) {
    // ---- pass B: the distortion of the ray and the gradient entries of its weights ----
    double A = rayreg::wave_excl_prefix_sum(a_l, lane), B = rayreg::wave_excl_prefix_sum(b_l, lane);
    const double sufA = rayreg::wave_excl_suffix_sum(a_l, lane), sufB = rayreg::wave_excl_suffix_sum(b_l, lane);
    double in_a = 0.0, in_b = 0.0, inter = 0.0, intra = 0.0;
    double e1 = s0 < S ? ((double)zrow[s0] - lo) / span : e_end;
    for (int s = s0; s < s1; ++s) {
      const double w = (double)wrow[s], e0 = e1;
      e1 = s + 1 < S ? ((double)zrow[s + 1] - lo) / span : e_end;
      const double u = (e0 + e1) / 2.0, d = e1 - e0, wu = w * u;
      in_a += w;                                             // the same additions as pass A's
      in_b += wu;
      inter += w * (u * A - B);
      intra += (w * w) * d;
      if (gw) {
        const double Ap = sufA + (a_l - in_a), Bp = sufB + (b_l - in_b);
        double term = a.lambda_dist * (2.0 * (u * (A - Ap) - (B - Bp)) + 2.0 * (w * d) / 3.0);
        if (opac_on) term += term_opac;
        gw[s] = (float)((double)gw[s] + term / nd);
      }
      A += w;
      B += wu;
    }
    dist = 2.0 * wave_sum(inter) + wave_sum(intra) / 3.0;
  } else if (opac_on && gw) {
    for (int s = s0; s < s1; ++s) gw[s] = (float)((double)gw[s] + term_opac / nd);
  }
  if (lane == 0) {
    a.ws_dist[ray] = dist;
    a.ws_opac[ray] = opac;
    a.ws_valid[ray] = valid ? 1 : 0;
  }
}

__global__ __launch_bounds__(FIN) void rayreg_finish_kernel(RayRegArgs a) {
  __shared__ double sh[SUMS][FIN];
  const int tid = threadIdx.x, n = a.n;
  double s[SUMS] = {0.0, 0.0, 0.0};                          // sum of dist_r, of opac_r; valid rays
  for (int r = tid; r < n; r += FIN) {
    s[0] += a.ws_dist[r];
    s[1] += a.ws_opac[r];
    s[2] += (double)a.ws_valid[r];
  }
  lds_tree_sum<FIN, SUMS>(sh, s);
  if (tid == 0) {
    const float v_dist = a.lambda_dist > 0.0 ? (float)(sh[0][0] / (double)n) : 0.f;
    const float v_opac = a.lambda_opac > 0.0 ? (float)(sh[1][0] / (double)n) : 0.f;
    a.values[0] = v_dist;
    a.values[1] = v_opac;
    a.stats[0] = (float)sh[2][0];
    if (a.fold_total) *a.fold_total += (float)(a.lambda_dist * (double)v_dist + a.lambda_opac * (double)v_opac);
  }
}

}  // namespace

void launch_rayreg_rays(hipStream_t st, const RayRegArgs& a) {
  rayreg_rays_kernel<<<(a.n + RPB - 1) / RPB, RPB * 64, 0, st>>>(a);
}

void launch_rayreg_finish(hipStream_t st, const RayRegArgs& a) {
  rayreg_finish_kernel<<<1, FIN, 0, st>>>(a);
}

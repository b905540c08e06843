// Depth pictures: weighted percentiles of a frame by a radix select, a frame's min / max, the colourised bytes.
// float64 from float32 inputs, no floating-point atomics, compiled with -ffp-contract=off.
//
// Percentiles.  An element's key is 56 bits: the order-preserving 32-bit image of its float (NaN last) over its 24-bit
// index, so the order is numpy's stable argsort and every key is unique.  Seven passes of one 8-bit digit, most significant
// first, each two launches:
//   hist    grid (nwg, frames): a workgroup walks tiles of 256 elements of one frame.  A tile's weights and digits (one per
//           percentile, 0xffff for an element outside that percentile's prefix) go to LDS, then thread b adds the weights
//           whose digit is b in element order: bin b has one owner, so its sum has one order.  A tile without a matching
//           element (all but one in 256 after the first pass) is skipped.  One partial histogram per workgroup.
//   select  grid (frames), 256 threads: partials added in workgroup order, then one thread per percentile walks the 256 bins
//           for the first whose running sum exceeds q and appends its digit to the prefix.
// After the last pass the prefix is the straddling element's key, `below` the running sum cw[j] in front of it and `upto`
// cw[j + 1].  pred finds the largest key below it (integer max: any order gives the same bits), interp writes np.interp's
// expression.
#include "depthvis_kernels.h"
#include "hip_device.h"

namespace {

constexpr int BLOCK = DEPTHVIS_BLOCK, MAXP = DEPTHVIS_MAX_PS;
constexpr int INDEX_BITS = 24;
constexpr double EPS32 = 1.1920928955078125e-07;             // 2^-23, jnp.finfo(jnp.float32).eps
constexpr uint64_t NO_KEY = ~0ull;

__device__ const double TABLES[2][256 * 3] = {{DEPTHVIS_TABLE_TURBO}, {DEPTHVIS_TABLE_JET}};

// the order-preserving image of a float: a < b <=> key(a) < key(b), every NaN above +inf
__device__ inline uint32_t float_key(float v) {
  const uint32_t b = __float_as_uint(v);
  if (v != v) return 0xffffffffu;
  return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__device__ inline float key_float(uint32_t k) { return __uint_as_float((k & 0x80000000u) ? (k ^ 0x80000000u) : ~k); }
__device__ inline uint64_t element_key(float v, int64_t i) { return ((uint64_t)float_key(v) << INDEX_BITS) | (uint64_t)i; }

__global__ __launch_bounds__(BLOCK) void depthvis_hist_kernel(int64_t n, int nwg, int n_ps, int pass, const float* __restrict__ value,
                                                             const float* __restrict__ weight,
                                                             const DepthvisState* __restrict__ state, double* __restrict__ hist) {
  const int f = blockIdx.y, g = blockIdx.x, tid = threadIdx.x;
  const float* fv = value + (int64_t)f * n;
  const float* fw = weight + (int64_t)f * n;
  const int shift = 8 * (DEPTHVIS_PASSES - 1 - pass);
  __shared__ uint4 tile[BLOCK];                              // weight bits, digits of percentiles 0 | 1, digits of 2 | 3
  uint64_t prefix[MAXP];
#pragma unroll
  for (int p = 0; p < MAXP; ++p) {
    prefix[p] = NO_KEY;                                      // matches no element
    if (p < n_ps) {
      if (pass == 0) prefix[p] = 0;
      else if (!state[f * MAXP + p].past_end) prefix[p] = state[f * MAXP + p].prefix;
    }
  }
  double acc[MAXP] = {0.0, 0.0, 0.0, 0.0};
  const int64_t n_tiles = (n + BLOCK - 1) / BLOCK;
  for (int64_t t = g; t < n_tiles; t += nwg) {
    const int64_t i = t * BLOCK + tid;
    uint32_t d[MAXP] = {0xffffu, 0xffffu, 0xffffu, 0xffffu};
    float w = 0.f;
    if (i < n) {
      const uint64_t key = element_key(fv[i], i);
      w = fw[i];
#pragma unroll
      for (int p = 0; p < MAXP; ++p)
        if (((key >> shift) >> 8) == prefix[p]) d[p] = (uint32_t)(key >> shift) & 0xffu;
    }
    const uint32_t d01 = d[0] | (d[1] << 16), d23 = d[2] | (d[3] << 16);
    // a barrier as well: every thread has finished reading the previous tile
    if (!__syncthreads_or((d01 & d23) != 0xffffffffu)) continue;
    tile[tid] = make_uint4(__float_as_uint(w), d01, d23, 0u);
    __syncthreads();
    const uint32_t me = (uint32_t)tid;
    for (int e = 0; e < BLOCK; ++e) {
      const uint4 v = tile[e];                               // one address for the whole wave: a broadcast read
      const double we = (double)__uint_as_float(v.x);
      acc[0] += (v.y & 0xffffu) == me ? we : 0.0;
      acc[1] += (v.y >> 16) == me ? we : 0.0;
      acc[2] += (v.z & 0xffffu) == me ? we : 0.0;
      acc[3] += (v.z >> 16) == me ? we : 0.0;
    }
  }
#pragma unroll
  for (int p = 0; p < MAXP; ++p) hist[(((int64_t)f * nwg + g) * MAXP + p) * BLOCK + tid] = acc[p];
}

__global__ __launch_bounds__(BLOCK) void depthvis_select_kernel(int nwg, int n_ps, int pass, DepthvisPs ps,
                                                               const double* __restrict__ hist, DepthvisState* __restrict__ state) {
  const int f = blockIdx.x, tid = threadIdx.x;
  __shared__ double h[MAXP][BLOCK];
  for (int p = 0; p < n_ps; ++p) {
    double s = 0.0;
    for (int g = 0; g < nwg; ++g) s += hist[(((int64_t)f * nwg + g) * MAXP + p) * BLOCK + tid];
    h[p][tid] = s;
  }
  __syncthreads();
  if (tid >= n_ps) return;
  DepthvisState st = state[f * MAXP + tid];
  if (pass == 0) {
    double total = 0.0;
    for (int b = 0; b < BLOCK; ++b) total += h[tid][b];
    const double p = tid == 0 ? ps.p[0] : tid == 1 ? ps.p[1] : tid == 2 ? ps.p[2] : ps.p[3];
    st.prefix = 0;
    st.below = 0.0;
    st.upto = 0.0;
    st.q = p * (total / 100.0);
    st.past_end = 0;
    st.pad[0] = st.pad[1] = st.pad[2] = 0;
  } else if (st.past_end) {
    return;
  }
  double c = st.below, c_last = 0.0;
  int found = -1, last = -1;
  for (int b = 0; b < BLOCK; ++b) {
    const double hb = h[tid][b];
    if (c + hb > st.q) { found = b; break; }
    if (hb > 0.0) { last = b; c_last = c; }
    c += hb;
  }
  if (found < 0) {
    if (pass == 0 || last < 0) {
      st.past_end = 1;                                       // q >= cw[-1] (or q is NaN): np.interp returns the last value
      state[f * MAXP + tid] = st;
      return;
    }
    found = last;                                            // the bucket's parts add up to less than the bucket did one pass
    c = c_last;                                              // earlier (another order of the same sum): its last weighted part
  }
  st.prefix = (st.prefix << 8) | (uint64_t)found;
  st.below = c;
  st.upto = c + h[tid][found];
  state[f * MAXP + tid] = st;
}

// pred [f, g, p]: 1 + the largest key below the straddling element's among the workgroup's elements, 0 when there is none
__global__ __launch_bounds__(BLOCK) void depthvis_pred_kernel(int64_t n, int nwg, int n_ps, const float* __restrict__ value,
                                                             const DepthvisState* __restrict__ state, uint64_t* __restrict__ pred) {
  const int f = blockIdx.y, g = blockIdx.x, tid = threadIdx.x;
  const float* fv = value + (int64_t)f * n;
  uint64_t bound[MAXP], best[MAXP] = {0, 0, 0, 0};
#pragma unroll
  for (int p = 0; p < MAXP; ++p)
    bound[p] = p < n_ps ? (state[f * MAXP + p].past_end ? NO_KEY : state[f * MAXP + p].prefix) : 0;
  for (int64_t i = (int64_t)g * BLOCK + tid; i < n; i += (int64_t)nwg * BLOCK) {
    const uint64_t key = element_key(fv[i], i);
#pragma unroll
    for (int p = 0; p < MAXP; ++p)
      if (key < bound[p] && key + 1 > best[p]) best[p] = key + 1;
  }
  __shared__ uint64_t red[MAXP][BLOCK];
#pragma unroll
  for (int p = 0; p < MAXP; ++p) red[p][tid] = best[p];
  __syncthreads();
  for (int s = BLOCK / 2; s > 0; s >>= 1) {
    if (tid < s) {
#pragma unroll
      for (int p = 0; p < MAXP; ++p) red[p][tid] = red[p][tid] > red[p][tid + s] ? red[p][tid] : red[p][tid + s];
    }
    __syncthreads();
  }
  if (tid < MAXP) pred[((int64_t)f * nwg + g) * MAXP + tid] = red[tid][0];
}

__global__ __launch_bounds__(64) void depthvis_interp_kernel(int64_t n, int nwg, int n_ps, const float* __restrict__ value,
                                                            const DepthvisState* __restrict__ state,
                                                            const uint64_t* __restrict__ pred, double* __restrict__ out) {
  const int f = blockIdx.x, p = threadIdx.x;
  if (p >= n_ps) return;
  const float* fv = value + (int64_t)f * n;
  const DepthvisState st = state[f * MAXP + p];
  uint64_t best = 0;
  for (int g = 0; g < nwg; ++g) {
    const uint64_t v = pred[((int64_t)f * nwg + g) * MAXP + p];
    best = v > best ? v : best;
  }
  const uint64_t index_mask = (1ull << INDEX_BITS) - 1;
  // best == 0 with past_end cannot happen (n >= 1); without it the straddling element is the first: q < cw[0]
  const double x_lo = best ? (double)fv[(best - 1) & index_mask] : 0.0;
  double r;
  if (st.past_end) {
    r = x_lo;
  } else {
    const double x_hi = (double)fv[st.prefix & index_mask];
    if (!best) {
      r = x_hi;
    } else if (st.below == st.q) {
      r = x_lo;
    } else {                                                 // numpy's arr_interp, its NaN repairs included
      const double slope = (x_hi - x_lo) / (st.upto - st.below);
      r = slope * (st.q - st.below) + x_lo;
      if (r != r) {
        r = slope * (st.q - st.upto) + x_hi;
        if (r != r && x_lo == x_hi) r = x_lo;
      }
    }
  }
  out[f * n_ps + p] = r;
}

__global__ __launch_bounds__(BLOCK) void depthvis_minmax_kernel(int64_t n, int nwg, const float* __restrict__ value,
                                                               uint32_t* __restrict__ keys) {
  const int f = blockIdx.y, g = blockIdx.x, tid = threadIdx.x;
  const float* fv = value + (int64_t)f * n;
  uint32_t lo = 0xffffffffu, hi = 0u, nan = 0u;
  for (int64_t i = (int64_t)g * BLOCK + tid; i < n; i += (int64_t)nwg * BLOCK) {
    const float v = fv[i];
    if (v != v) { nan = 1u; continue; }
    const uint32_t k = float_key(v);
    lo = k < lo ? k : lo;
    hi = k > hi ? k : hi;
  }
  __shared__ uint32_t red[3][BLOCK];
  red[0][tid] = lo; red[1][tid] = hi; red[2][tid] = nan;
  __syncthreads();
  for (int s = BLOCK / 2; s > 0; s >>= 1) {
    if (tid < s) {
      red[0][tid] = red[0][tid] < red[0][tid + s] ? red[0][tid] : red[0][tid + s];
      red[1][tid] = red[1][tid] > red[1][tid + s] ? red[1][tid] : red[1][tid + s];
      red[2][tid] |= red[2][tid + s];
    }
    __syncthreads();
  }
  if (tid < 3) keys[((int64_t)f * nwg + g) * 3 + tid] = red[tid][0];
}

__global__ __launch_bounds__(64) void depthvis_minmax_finish_kernel(int n_frames, int nwg, const uint32_t* __restrict__ keys,
                                                                   float* __restrict__ out) {
  const int f = blockIdx.x * 64 + threadIdx.x;
  if (f >= n_frames) return;
  uint32_t lo = 0xffffffffu, hi = 0u, nan = 0u;
  for (int g = 0; g < nwg; ++g) {
    const uint32_t* k = keys + ((int64_t)f * nwg + g) * 3;
    lo = k[0] < lo ? k[0] : lo;
    hi = k[1] > hi ? k[1] : hi;
    nan |= k[2];
  }
  const float qnan = __uint_as_float(0x7fc00000u);
  const bool none = lo > hi;                                 // no value that is not NaN
  const float nanmin = none ? qnan : key_float(lo), nanmax = none ? qnan : key_float(hi);
  out[f * 4 + 0] = nan ? qnan : nanmin;
  out[f * 4 + 1] = nan ? qnan : nanmax;
  out[f * 4 + 2] = nanmin;
  out[f * 4 + 3] = nanmax;
}

__global__ __launch_bounds__(BLOCK) void depthvis_prepare_kernel(int64_t n_pixels, const float* __restrict__ acc,
                                                                const float* __restrict__ dmean, const float* __restrict__ dmedian,
                                                                const float* __restrict__ p5, const float* __restrict__ p95,
                                                                float* __restrict__ acc_eff, float* __restrict__ trip_value,
                                                                float* __restrict__ trip_weight) {
  const int64_t px = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
  if (px >= n_pixels) return;
  const int64_t i = (int64_t)blockIdx.y * n_pixels + px;
  const float m = dmean[i];
  const float a = m != m ? 0.f : acc[i];
  acc_eff[i] = a;
  if (trip_value != nullptr) {
    const float med = dmedian[i];
    trip_value[i * 3 + 0] = 2.f * med - p5[i];
    trip_value[i * 3 + 1] = med;
    trip_value[i * 3 + 2] = p95[i];
    trip_weight[i * 3 + 0] = a;
    trip_weight[i * 3 + 1] = a;
    trip_weight[i * 3 + 2] = a;
  }
}

__device__ inline double dv_curve(double x, int curve) {
  if (curve == DEPTHVIS_CURVE_NEG_LOG) return -log(x + EPS32);
  if (curve == DEPTHVIS_CURVE_LOG) return log(x + EPS32);
  return x;
}

// nan_to_num(clip((v - min(lo, hi)) / |hi - lo|, 0, 1)) with the curved lo, hi; minimum and clip pass a NaN on
__device__ inline double dv_unit(double v, double lo, double hi) {
  const double m = (lo != lo || hi != hi) ? lo + hi : fmin(lo, hi);
  double t = (v - m) / fabs(hi - lo);
  t = t < 0.0 ? 0.0 : (t > 1.0 ? 1.0 : t);
  return t != t ? 0.0 : t;
}

// matplotlib's lookup of a float32 t: row clamp(floor(t * 256), 0, 255), a NaN is (0, 0, 0)
__device__ inline void dv_table(float t, int cmap, double c[3]) {
  if (t != t) { c[0] = c[1] = c[2] = 0.0; return; }
  const float s = floorf(t * 256.f);
  const int idx = s < 0.f ? 0 : (s > 255.f ? 255 : (int)s);
  const double* row = TABLES[cmap] + idx * 3;
  c[0] = row[0]; c[1] = row[1]; c[2] = row[2];
}

__device__ inline uint8_t dv_byte(double v) {
  if (v != v) v = 0.0;
  v = v < 0.0 ? 0.0 : (v > 1.0 ? 1.0 : v);                   // +-inf: nan_to_num's largest finite values clip the same way
  return (uint8_t)(v * 255.0);
}

// numpy's float remainder by 2
__device__ inline double dv_mod2(double a) {
  double r = fmod(a, 2.0);
  if (r != 0.0) { if (r < 0.0) r += 2.0; }
  else r = 0.0;
  return r;
}

__global__ __launch_bounds__(BLOCK) void depthvis_colorize_kernel(int H, int W, int mode, int cmap, int curve,
                                                                 const float* __restrict__ value, const float* __restrict__ acc,
                                                                 const float* __restrict__ origins, const float* __restrict__ directions,
                                                                 const double* __restrict__ lohi, const float* __restrict__ minmax,
                                                                 uint8_t* __restrict__ out) {
  const int f = blockIdx.y;
  const int64_t n_pixels = (int64_t)H * W;
  const int64_t px = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
  if (px >= n_pixels) return;
  const int64_t i = (int64_t)f * n_pixels + px;
  double c[3];
  if (mode == DEPTHVIS_MODE_MINMAX) {
    const float vmin = minmax[f * 4 + 0], vmax = minmax[f * 4 + 1] + 1e-6f;
    dv_table((value[i] - vmin) / (vmax - vmin), cmap, c);
    out[i * 3 + 0] = dv_byte(c[0]); out[i * 3 + 1] = dv_byte(c[1]); out[i * 3 + 2] = dv_byte(c[2]);
    return;
  }
  if (mode == DEPTHVIS_MODE_CMAP || mode == DEPTHVIS_MODE_CMAP3) {
    const double lo = dv_curve(lohi[f * 2 + 0] - EPS32, curve), hi = dv_curve(lohi[f * 2 + 1] + EPS32, curve);
    if (mode == DEPTHVIS_MODE_CMAP) {
      dv_table((float)dv_unit(dv_curve((double)value[i], curve), lo, hi), cmap, c);
    } else {
#pragma unroll
      for (int k = 0; k < 3; ++k) c[k] = dv_unit(dv_curve((double)value[i * 3 + k], curve), lo, hi);
    }
  } else if (mode == DEPTHVIS_MODE_MATTE_RGB) {
#pragma unroll
    for (int k = 0; k < 3; ++k) c[k] = (double)value[i * 3 + k];
  } else {                                                   // DEPTHVIS_MODE_COORDS_MOD
    const double dist = (double)value[i];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const double coord = (double)origins[i * 3 + k] + (double)directions[i * 3 + k] * dist;
      c[k] = dv_mod2(coord + 1.0) / 2.0;
    }
  }
  const int row = (int)(px / W), col = (int)(px % W);
  const double bg = (((row % 16) / 8) ^ ((col % 16) / 8)) ? 1.0 : 0.8;
  const double a = (double)acc[i];
  const double rest = bg * (1.0 - a);
#pragma unroll
  for (int k = 0; k < 3; ++k) out[i * 3 + k] = dv_byte(c[k] * a + rest);
}

}  // namespace

void launch_depthvis_hist(hipStream_t st, int n_frames, int64_t n, int nwg, int n_ps, int pass, const float* value,
                          const float* weight, const DepthvisState* state, double* hist) {
  depthvis_hist_kernel<<<dim3(nwg, n_frames), BLOCK, 0, st>>>(n, nwg, n_ps, pass, value, weight, state, hist);
}

void launch_depthvis_select(hipStream_t st, int n_frames, int nwg, int n_ps, int pass, DepthvisPs ps, const double* hist,
                            DepthvisState* state) {
  depthvis_select_kernel<<<n_frames, BLOCK, 0, st>>>(nwg, n_ps, pass, ps, hist, state);
}

void launch_depthvis_pred(hipStream_t st, int n_frames, int64_t n, int nwg, int n_ps, const float* value,
                          const DepthvisState* state, uint64_t* pred) {
  depthvis_pred_kernel<<<dim3(nwg, n_frames), BLOCK, 0, st>>>(n, nwg, n_ps, value, state, pred);
}

void launch_depthvis_interp(hipStream_t st, int n_frames, int64_t n, int nwg, int n_ps, const float* value,
                            const DepthvisState* state, const uint64_t* pred, double* out) {
  depthvis_interp_kernel<<<n_frames, 64, 0, st>>>(n, nwg, n_ps, value, state, pred, out);
}

void launch_depthvis_minmax(hipStream_t st, int n_frames, int64_t n, int nwg, const float* value, uint32_t* keys, float* out) {
  depthvis_minmax_kernel<<<dim3(nwg, n_frames), BLOCK, 0, st>>>(n, nwg, value, keys);
  depthvis_minmax_finish_kernel<<<(n_frames + 63) / 64, 64, 0, st>>>(n_frames, nwg, keys, out);
}

void launch_depthvis_prepare(hipStream_t st, int n_frames, int64_t n_pixels, const float* acc, const float* dmean,
                             const float* dmedian, const float* p5, const float* p95, float* acc_eff, float* trip_value,
                             float* trip_weight) {
  depthvis_prepare_kernel<<<dim3((unsigned)((n_pixels + BLOCK - 1) / BLOCK), n_frames), BLOCK, 0, st>>>(
      n_pixels, acc, dmean, dmedian, p5, p95, acc_eff, trip_value, trip_weight);
}

void launch_depthvis_colorize(hipStream_t st, int n_frames, int H, int W, int mode, int cmap, int curve, const float* value,
                              const float* acc, const float* origins, const float* directions, const double* lohi,
                              const float* minmax, uint8_t* out) {
  const int64_t n_pixels = (int64_t)H * W;
  depthvis_colorize_kernel<<<dim3((unsigned)((n_pixels + BLOCK - 1) / BLOCK), n_frames), BLOCK, 0, st>>>(
      H, W, mode, cmap, curve, value, acc, origins, directions, lohi, minmax, out);
}

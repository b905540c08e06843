// Aligning relative depth priors to sparse metric depth.  Float64 in the written order of
// tests/depth_align_reference.py, compiled with -ffp-contract=off.  No atomics anywhere.
//
//   tiles    grid (frames x tiles), 256 threads, launched twice: a workgroup takes 2048 consecutive pixels of one frame, eight rounds
//            of loads that are all in flight together.  A pixel is a pair iff prior > 0 and anchor > 0; the ballots of the eight rounds
//            of the four waves go to LDS.  First launch: their sum is the tile's count.  Second launch (after scan): the pairs
//            (x float32, t float64: the anchor widened, or its float64 reciprocal, computed once here and not in every pass of the
//            fit) are written in PIXEL ORDER at the tile's offset: rounds, then waves, then lanes.
//   scan     grid (frames), 256 threads: the exclusive scan of a frame's tile counts (integers), and the frame's pair count.
//   fit      grid (frames), 1024 threads: all iters + 1 solves of a frame in one launch over its compacted list, which stays in L2 (a
//            5 % anchor of a 375 x 1242 frame is 279 KB of pairs: more than the CU's LDS).  Thread j adds pairs j, j + 1024, ... in
//            that order and the 1024 partials meet in hipdev::lds_tree_sum: the tree is a function of the pair count alone.  (Wave
//            shuffles and 16 wave sums in wave order instead measured slower: 1.50 against 1.35 ms for the whole call.)  The weights
//            are recomputed from (s, b, sigma) of the previous solve rather than stored.
//   apply    grid over the flat [frames x pixels] array, 256 threads x 4 consecutive pixels, 16-byte accesses when every base is
//            aligned to 16 (a frame's own base need not be: the four pixels may straddle two frames, and each looks up its own row).
#include "depthalign_kernels.h"
#include "hip_device.h"

namespace {

constexpr int BLOCK = DEPTHALIGN_BLOCK, WAVES = BLOCK / 64, TILE = DEPTHALIGN_TILE, ROUNDS = TILE / BLOCK, FIT = DEPTHALIGN_FIT_BLOCK;
constexpr int ROW = DEPTHALIGN_ROW;
constexpr double GAUSS = 1.2533141373155001;                 // sqrt(pi / 2)

__global__ __launch_bounds__(BLOCK) void depthalign_tiles_kernel(int64_t frame_px, int64_t wg0, int64_t tiles, int disparity,
                                                                const float* __restrict__ prior, const float* __restrict__ anchor,
                                                                int32_t* __restrict__ counts, const int32_t* __restrict__ offsets,
                                                                float* __restrict__ xs, double* __restrict__ ts) {
  __shared__ int cnt[ROUNDS][WAVES];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t g = wg0 + (int64_t)blockIdx.x;
  const int64_t f = g / tiles, tile = g % tiles;
  const float* pf = prior + f * frame_px;
  const float* af = anchor + f * frame_px;
  float pk[ROUNDS], ak[ROUNDS];                              // every load of the tile is in flight before the first is looked at
#pragma unroll
  for (int k = 0; k < ROUNDS; ++k) {
    const int64_t i = tile * TILE + k * BLOCK + tid;
    pk[k] = i < frame_px ? pf[i] : 0.f;
    ak[k] = i < frame_px ? af[i] : 0.f;
  }
  unsigned long long m[ROUNDS];
#pragma unroll
  for (int k = 0; k < ROUNDS; ++k) {
    m[k] = __ballot(pk[k] > 0.f && ak[k] > 0.f);             // 0, negatives and NaN are invalid
    if (lane == 0) cnt[k][wave] = (int)__popcll(m[k]);
  }
  __syncthreads();
  if (xs == nullptr) {                                       // (uniform) the first launch: the count alone
    if (tid == 0) {
      int n = 0;
#pragma unroll
      for (int k = 0; k < ROUNDS; ++k)
#pragma unroll
        for (int w = 0; w < WAVES; ++w) n += cnt[k][w];
      counts[g] = n;
    }
    return;
  }
  const int64_t first = f * frame_px + offsets[g];           // at most frame_px pairs of the frame: every write stays inside its frame
  int base = 0;
#pragma unroll
  for (int k = 0; k < ROUNDS; ++k) {
#pragma unroll
    for (int w = 0; w < WAVES; ++w) {
      if (w == wave && pk[k] > 0.f && ak[k] > 0.f) {
        const int64_t pos = first + base + (int)__popcll(m[k] & ((1ull << lane) - 1ull));
        xs[pos] = pk[k];
        ts[pos] = disparity ? 1.0 / (double)ak[k] : (double)ak[k];
      }
      base += cnt[k][w];
    }
  }
}

__global__ __launch_bounds__(BLOCK) void depthalign_scan_kernel(int64_t tiles, const int32_t* __restrict__ counts,
                                                               int32_t* __restrict__ offsets, int32_t* __restrict__ n_pairs) {
  __shared__ int part[BLOCK];
  const int tid = threadIdx.x;
  const int64_t f = blockIdx.x, per = (tiles + BLOCK - 1) / BLOCK;
  const int32_t* cf = counts + f * tiles;
  int32_t* of = offsets + f * tiles;
  const int64_t t0 = tid * per, t1 = t0 + per < tiles ? t0 + per : tiles;     // thread tid scans tiles [t0, t1)
  int sum = 0;
  for (int64_t t = t0; t < t1; ++t) sum += cf[t];
  part[tid] = sum;
  __syncthreads();
  int before = 0;
  for (int j = 0; j < tid; ++j) before += part[j];
  for (int64_t t = t0; t < t1; ++t) {
    of[t] = before;
    before += cf[t];
  }
  if (tid == BLOCK - 1) n_pairs[f] = before;
}

__global__ __launch_bounds__(FIT) void depthalign_fit_kernel(int64_t frame_px, const float* __restrict__ xs, const double* __restrict__ ts,
                                                           const int32_t* __restrict__ n_pairs, DepthAlignParams prm,
                                                           double* __restrict__ rows) {
  __shared__ double sh[5][FIT];
  __shared__ int inl[FIT / 64];
  const int tid = threadIdx.x;
  const int64_t f = blockIdx.x;
  const int n = n_pairs[f];
  const float* X = xs + f * frame_px;
  const double* Tg = ts + f * frame_px;
  double* row = rows + f * ROW;
  int status = DEPTHALIGN_STATUS_FITTED, done = 0, n_in = 0;
  double s = 0.0, b = 0.0, sigma = 0.0, rms = 0.0;
  if (n < prm.min_points) {                                  // (uniform, like every branch on a sum below: all threads read the same LDS words)
    status = DEPTHALIGN_STATUS_FEW;
  } else {
    bool have = false;                                       // weights of (sp, bp, cs) of the previous solve; none: w = 1
    double sp = 0.0, bp = 0.0, cs = 1.0, rss = 0.0;
    for (int k = 0; k <= prm.iters; ++k) {
      double v[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
      for (int i = tid; i < n; i += FIT) {
        const double x = (double)X[i], t = Tg[i];
        double w = 1.0;
        if (have) {
          const double q = fabs((sp * x + bp) - t) / cs;
          w = 1.0 / (1.0 + q * q);
        }
        const double wx = w * x;
        v[0] += w;
        v[1] += wx;
        v[2] += w * t;
        v[3] += wx * x;
        v[4] += wx * t;
      }
      hipdev::lds_tree_sum<FIT, 5>(sh, v);
      const double Sw = sh[0][0], Sx = sh[1][0], St = sh[2][0], Sxx = sh[3][0], Sxt = sh[4][0];
      __syncthreads();                                       // every thread has read the sums before the next tree stores
      const double den = Sw * Sxx - Sx * Sx;
      if (!(den > (1e-8 * Sw) * Sxx)) {
        status = DEPTHALIGN_STATUS_DEGENERATE;
        break;
      }
      s = (Sw * Sxt - Sx * St) / den;
      b = (St - s * Sx) / Sw;
      ++done;
      double u[5] = {0.0, 0.0, 0.0, 0.0, 0.0};               // sum w |r| and sum r r of this solve, under the weights it was solved with
      for (int i = tid; i < n; i += FIT) {
        const double x = (double)X[i], t = Tg[i];
        double w = 1.0;
        if (have) {
          const double q = fabs((sp * x + bp) - t) / cs;
          w = 1.0 / (1.0 + q * q);
        }
        const double r = (s * x + b) - t;
        u[0] += w * fabs(r);
        u[1] += r * r;
      }
      hipdev::lds_tree_sum<FIT, 5>(sh, u);
      const double Swr = sh[0][0];
      rss = sh[1][0];
      __syncthreads();
      sigma = GAUSS * (Swr / Sw);
      if (!(k < prm.iters && sigma > 0.0)) break;            // the last solve, or an exact fit
      sp = s;
      bp = b;
      cs = prm.c * sigma;
      have = true;
    }
    if (status == DEPTHALIGN_STATUS_FITTED) {
      rms = sqrt(rss / (double)n);
      if (!(s > 0.0 && isfinite(s) && isfinite(b) && isfinite(sigma) && isfinite(rms))) {
        status = DEPTHALIGN_STATUS_INVERTED;
      } else {
        const double three = 3.0 * sigma;
        int mine = 0;
        for (int i = tid; i < n; i += FIT) {
          mine += fabs((s * (double)X[i] + b) - Tg[i]) <= three ? 1 : 0;
        }
        mine = hipdev::wave_sum_lane0(mine);                 // integers: every order gives the same count
        if ((tid & 63) == 0) inl[tid >> 6] = mine;
        __syncthreads();
        if (tid == 0)
          for (int w = 0; w < FIT / 64; ++w) n_in += inl[w];
      }
    }
  }
  if (tid != 0) return;
  const bool ok = status == DEPTHALIGN_STATUS_FITTED;
  row[DEPTHALIGN_ROW_S] = ok ? s : 0.0;
  row[DEPTHALIGN_ROW_B] = ok ? b : 0.0;
  row[DEPTHALIGN_ROW_SIGMA] = ok ? sigma : 0.0;
  row[DEPTHALIGN_ROW_N_PAIRS] = (double)n;
  row[DEPTHALIGN_ROW_N_INLIERS] = ok ? (double)n_in : 0.0;
  row[DEPTHALIGN_ROW_STATUS] = (double)status;
  row[DEPTHALIGN_ROW_ITERATIONS] = (double)done;
  row[DEPTHALIGN_ROW_RMS] = ok ? rms : 0.0;
}

// one pixel of step 6 and 7: depth_out and std_out of prior p and anchor a under the row of the pixel's frame
__device__ __forceinline__ void apply_pixel(float p, float a, const double* __restrict__ row, const DepthAlignParams& prm, float& d, float& sd) {
  d = 0.f;
  sd = 0.f;
  if (row[DEPTHALIGN_ROW_STATUS] == (double)DEPTHALIGN_STATUS_FITTED && p > 0.f) {
    const double sigma = row[DEPTHALIGN_ROW_SIGMA];
    const double v = row[DEPTHALIGN_ROW_S] * (double)p + row[DEPTHALIGN_ROW_B];
    const bool disp = prm.space == DEPTHALIGN_SPACE_DISPARITY;
    const double z = disp ? 1.0 / v : v;
    if (v > 0.0 && z <= prm.max_depth) {
      const double sdev = disp ? (sigma * z) * z : sigma;
      d = (float)z;
      sd = (float)(sdev > prm.std_floor ? sdev : prm.std_floor);
    }
  }
  if (prm.keep_anchor && a > 0.f) {                          // a measurement beats the aligned guess: the anchor's own bits
    d = a;
    sd = (float)prm.std_floor;
  }
}

template <bool VEC>
__global__ __launch_bounds__(BLOCK) void depthalign_apply_kernel(int64_t n_px, int64_t frame_px, int64_t wg0, const float* __restrict__ prior,
                                                                const float* __restrict__ anchor, const double* __restrict__ rows,
                                                                DepthAlignParams prm, float* __restrict__ depth_out,
                                                                float* __restrict__ std_out) {
  const int64_t i0 = ((wg0 + (int64_t)blockIdx.x) * BLOCK + threadIdx.x) * 4;
  if (i0 >= n_px) return;
  const bool whole = i0 + 4 <= n_px;
  float p[4], a[4], d[4], sd[4];
  if (VEC && whole) {
    const hipdev::f32x4 pv = *(const hipdev::f32x4*)(prior + i0), av = *(const hipdev::f32x4*)(anchor + i0);
#pragma unroll
    for (int e = 0; e < 4; ++e) p[e] = pv[e], a[e] = av[e];
  } else {
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      p[e] = i0 + e < n_px ? prior[i0 + e] : 0.f;
      a[e] = i0 + e < n_px ? anchor[i0 + e] : 0.f;
    }
  }
  int64_t f = i0 / frame_px, rem = i0 - f * frame_px;        // the frame of the first pixel; the others may lie in later frames
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    while (rem >= frame_px) {
      rem -= frame_px;
      ++f;
    }
    if (i0 + e < n_px) apply_pixel(p[e], a[e], rows + f * ROW, prm, d[e], sd[e]);
    else d[e] = sd[e] = 0.f;
    ++rem;
  }
  if (VEC && whole) {
    hipdev::f32x4 dv, sv;
#pragma unroll
    for (int e = 0; e < 4; ++e) dv[e] = d[e], sv[e] = sd[e];
    *(hipdev::f32x4*)(depth_out + i0) = dv;
    if (std_out != nullptr) *(hipdev::f32x4*)(std_out + i0) = sv;
  } else {
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      if (i0 + e >= n_px) break;
      depth_out[i0 + e] = d[e];
      if (std_out != nullptr) std_out[i0 + e] = sd[e];
    }
  }
}

}  // namespace

void launch_depthalign_tiles(hipStream_t st, int height, int width, int64_t wg0, int64_t n_wg, int disparity, const float* prior,
                             const float* anchor, int32_t* counts, const int32_t* offsets, float* xs, double* ts) {
  depthalign_tiles_kernel<<<(unsigned)n_wg, BLOCK, 0, st>>>((int64_t)height * width, wg0, depthalign_tiles(height, width), disparity, prior,
                                                          anchor, counts, offsets, xs, ts);
}

void launch_depthalign_scan(hipStream_t st, int n_frames, int64_t tiles, const int32_t* counts, int32_t* offsets, int32_t* n_pairs) {
  depthalign_scan_kernel<<<n_frames, BLOCK, 0, st>>>(tiles, counts, offsets, n_pairs);
}

void launch_depthalign_fit(hipStream_t st, int n_frames, int64_t frame_px, const float* xs, const double* ts, const int32_t* n_pairs,
                           const DepthAlignParams& prm, double* rows) {
  depthalign_fit_kernel<<<n_frames, FIT, 0, st>>>(frame_px, xs, ts, n_pairs, prm, rows);
}

void launch_depthalign_apply(hipStream_t st, int n_frames, int64_t frame_px, const float* prior, const float* anchor, const double* rows,
                             const DepthAlignParams& prm, float* depth_out, float* std_out) {
  const int64_t n_px = (int64_t)n_frames * frame_px, n_wg = (n_px + 4 * BLOCK - 1) / (4 * BLOCK);
  const bool vec = (((uintptr_t)prior | (uintptr_t)anchor | (uintptr_t)depth_out | (uintptr_t)std_out) & 15) == 0;
  for (int64_t g0 = 0; g0 < n_wg; g0 += depthprior::MAX_GRID) {
    const unsigned grid = (unsigned)(n_wg - g0 < depthprior::MAX_GRID ? n_wg - g0 : depthprior::MAX_GRID);
    if (vec) depthalign_apply_kernel<true><<<grid, BLOCK, 0, st>>>(n_px, frame_px, g0, prior, anchor, rows, prm, depth_out, std_out);
    else depthalign_apply_kernel<false><<<grid, BLOCK, 0, st>>>(n_px, frame_px, g0, prior, anchor, rows, prm, depth_out, std_out);
  }
}

// Plane-sweep multi-view stereo.  Integer arithmetic for everything discrete, float64 in the written order of
// tests/depth_mvs_reference.py for the geometry and the refinement, compiled with -ffp-contract=off.
//
//   census  grid (pixels / 256), 256 threads: one pixel per thread, the luma of its 25 taps from rgb (taps outside the frame read
//           the nearest pixel inside), 24 bits.
//   sweep   grid (frames x tiles), 256 threads: a tile of 32 x 16 pixels of one frame, two pixels per thread (rows ty and ty + 8).
//           The point of pixel (X, Y, 1) of frame i on plane w in camera j is h = A (X, Y, 1) + w b with A = Rj^T Ri and
//           b = Rj^T (ti - tj), written h_c = (A_c0 X + A_c1 Y) + (A_c2 + w b_c).  Everything but w is hoisted out of the plane loop
//           in separable form: A_c0 X per view and column and A_c1 Y per view and row of the tile and its aggregation halo, in LDS
//           (24 KB at 16 views instead of 24 bytes per pixel and view in registers); per plane 3 n_views threads write the
//           plane's (A_c2 + w b_c) for the next plane.  A step of the loop (cell, view, plane) is then six LDS reads, six adds,
//           two divisions, the floor, one gather of the neighbour's census word and a __popc.  The costs of a cell's views go
//           into a histogram of 24 five-bit bins in two 64-bit registers (a view out of bounds costs 24 and needs no bin); the
//           sum of the best_views smallest walks the occupied bins from the lowest.  The slice c | n_in << 9 of the tile and
//           halo goes to LDS (16 bits per cell, two buffers, one barrier per plane) and every thread box-sums its two pixels
//           from there.  A halo cell outside the frame is the cell of the nearest pixel inside.
//           The running state of a pixel is in registers: the four smallest (C << 8 | k) in order -- `second`, the minimum of C
//           over |k - k*| > 1, leaves out at most three planes, so it is among the four smallest whatever order the planes
//           arrive in, and ties go to the lower k because k is the low byte --, the cost before and after the best, and n_in at
//           the best.  No curve is kept, nothing grows with the number of planes, and the planes are walked once.
//           The tile's three counts are wave sums, added over the four waves in wave order.
//   rows    grid (frames), 64 threads: lane l adds the partials of tiles l, l + 64, ... and a shfl_down tree adds the lanes.  The
//           partials are integers, so every order gives the same bits.
#include "depthmvs_kernels.h"
#include "depth_prior_device.h"

namespace {

constexpr int BLOCK = DEPTHMVS_BLOCK, TW = DEPTHMVS_TILE_W, TH = DEPTHMVS_TILE_H, PPT = DEPTHMVS_PPT, WAVES = BLOCK / 64;
constexpr int RMAX = DEPTHMVS_MAX_RADIUS, VMAX = DEPTHMVS_MAX_VIEWS, ROWS_PER_ROUND = BLOCK / TW;
constexpr int HW_MAX = TW + 2 * RMAX, HH_MAX = TH + 2 * RMAX, CELLS_MAX = HW_MAX * HH_MAX;
constexpr int CPT = (CELLS_MAX + BLOCK - 1) / BLOCK;         // cells of tile and halo per thread, at most
constexpr int OUT = DEPTHMVS_CENSUS_BITS;                    // the cost of a view out of bounds
constexpr int CAM = DEPTHMVS_CAM;

__device__ __forceinline__ int clampi(int v, int hi) { return v < 0 ? 0 : (v > hi ? hi : v); }

__global__ __launch_bounds__(BLOCK) void depthmvs_census_kernel(const uint8_t* __restrict__ rgb, int height, int width, int64_t i0,
                                                                int64_t n, uint32_t* __restrict__ census) {
  const int64_t t = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
  if (t >= n) return;
  const int64_t i = i0 + t, px = (int64_t)height * width, f = i / px, r = i % px;
  const int y = (int)(r / width), x = (int)(r % width);
  const uint8_t* img = rgb + 3 * f * px;
  const auto luma = [&](int xx, int yy) {
    const uint8_t* p = img + 3 * ((int64_t)clampi(yy, height - 1) * width + clampi(xx, width - 1));
    return (77 * (int)p[0] + 150 * (int)p[1] + 29 * (int)p[2] + 128) >> 8;
  };
  const int centre = luma(x, y);
  uint32_t bits = 0;
  int tap = 0;
#pragma unroll
  for (int dy = -2; dy <= 2; ++dy) {
#pragma unroll
    for (int dx = -2; dx <= 2; ++dx) {
      if (dy == 0 && dx == 0) continue;
      bits |= (uint32_t)(luma(x + dx, y + dy) < centre) << tap;
      ++tap;
    }
  }
  census[i] = bits;
}

struct V3 {
  double c[3];
};

__global__ __launch_bounds__(BLOCK) void depthmvs_sweep_kernel(const DepthmvsSweep a, int64_t wg0) {
  __shared__ V3 l_col[VMAX][HW_MAX];                         // A_c0 X of every view and column of tile and halo
  __shared__ V3 l_row[VMAX][HH_MAX];                         // A_c1 Y of every view and row
  __shared__ V3 l_pl[2][VMAX];                               // A_c2 + w b_c of the plane, two buffers
  __shared__ double l_A[VMAX][3][3], l_b[VMAX][3], l_K[VMAX][4];
  __shared__ int l_j[VMAX];                                  // the view's frame, -1: none
  __shared__ uint16_t l_slice[2][CELLS_MAX];                 // c | n_in << 9 of every cell, two buffers
  __shared__ int red[WAVES][3];
  const int tid = threadIdx.x, tx = tid % TW, ty = tid / TW;
  const int64_t g = wg0 + (int64_t)blockIdx.x;
  const int64_t f = g / a.tiles, tile = g % a.tiles;
  const int x0 = (int)(tile % a.tiles_x) * TW, y0 = (int)(tile / a.tiles_x) * TH;
  const int height = a.height, width = a.width, V = a.n_views, D = a.n_planes, r = a.radius;
  const int hw = TW + 2 * r, hh = TH + 2 * r, cells = hw * hh;
  const int64_t px = (int64_t)height * width, base = f * px;
  const double* ci = a.cams + f * CAM;

  if (tid < V) {                                             // the view's frame, A = Rj^T Ri, b = Rj^T (ti - tj) and its intrinsics
    const int j = a.nbr[f * V + tid];
    const bool have = j >= 0 && j < a.n_frames;
    l_j[tid] = have ? j : -1;
    if (have) {
      const double* cj = a.cams + (int64_t)j * CAM;
      const double d0 = ci[7] - cj[7], d1 = ci[11] - cj[11], d2 = ci[15] - cj[15];
#pragma unroll
      for (int c = 0; c < 3; ++c) {
#pragma unroll
        for (int q = 0; q < 3; ++q) l_A[tid][c][q] = (cj[4 + c] * ci[4 + q] + cj[8 + c] * ci[8 + q]) + cj[12 + c] * ci[12 + q];
        l_b[tid][c] = (cj[4 + c] * d0 + cj[8 + c] * d1) + cj[12 + c] * d2;
      }
#pragma unroll
      for (int q = 0; q < 4; ++q) l_K[tid][q] = cj[q];
    }
  }
  __syncthreads();
  for (int q = tid; q < V * hw; q += BLOCK) {
    const int s = q / hw, hx = q - s * hw;
    if (l_j[s] < 0) continue;
    const double X = (((double)clampi(x0 + hx - r, width - 1) + 0.5) - ci[2]) / ci[0];
#pragma unroll
    for (int c = 0; c < 3; ++c) l_col[s][hx].c[c] = l_A[s][c][0] * X;
  }
  for (int q = tid; q < V * hh; q += BLOCK) {
    const int s = q / hh, hy = q - s * hh;
    if (l_j[s] < 0) continue;
    const double Y = (((double)clampi(y0 + hy - r, height - 1) + 0.5) - ci[3]) / ci[1];
#pragma unroll
    for (int c = 0; c < 3; ++c) l_row[s][hy].c[c] = l_A[s][c][1] * Y;
  }
  if (tid < 3 * V && l_j[tid / 3] >= 0) l_pl[0][tid / 3].c[tid % 3] = l_A[tid / 3][tid % 3][2] + a.inv_depth[0] * l_b[tid / 3][tid % 3];

  // the thread's cells of tile and halo: its census word, hoisted
  uint32_t cen[CPT];
#pragma unroll
  for (int n = 0; n < CPT; ++n) {
    const int q = tid + n * BLOCK;
    cen[n] = 0;
    if (q < cells) {
      const int hy = q / hw, hx = q - hy * hw;
      cen[n] = a.census[base + (int64_t)clampi(y0 + hy - r, height - 1) * width + clampi(x0 + hx - r, width - 1)];
    }
  }
  __syncthreads();

  // the running state of the thread's two pixels
  uint32_t m0[PPT], m1[PPT], m2[PPT], m3[PPT];               // the four smallest C << 8 | k, in order
  int cm[PPT], cp[PPT], prev[PPT], nin[PPT];
#pragma unroll
  for (int p = 0; p < PPT; ++p) {
    m0[p] = m1[p] = m2[p] = m3[p] = 0xffffffffu;
    cm[p] = cp[p] = prev[p] = nin[p] = 0;
  }
  const double wlim = (double)width, hlim = (double)height;

  for (int k = 0; k < D; ++k) {
    const int buf = k & 1;
    if (k + 1 < D && tid < 3 * V && l_j[tid / 3] >= 0)
      l_pl[buf ^ 1][tid / 3].c[tid % 3] = l_A[tid / 3][tid % 3][2] + a.inv_depth[k + 1] * l_b[tid / 3][tid % 3];
#pragma unroll
    for (int n = 0; n < CPT; ++n) {
      const int q = tid + n * BLOCK;
      if (q >= cells) continue;
      const int hy = q / hw, hx = q - hy * hw;
      unsigned long long lo = 0, hi = 0;                     // bins 0 .. 11 and 12 .. 23 of the views' costs, five bits each
      uint32_t occ = 0;
      int n_in = 0;
      for (int s = 0; s < V; ++s) {
        const int j = l_j[s];
        if (j < 0) continue;                                 // (uniform)
        const V3 cc = l_col[s][hx], rr = l_row[s][hy], pl = l_pl[buf][s];
        const double h0 = (cc.c[0] + rr.c[0]) + pl.c[0], h1 = (cc.c[1] + rr.c[1]) + pl.c[1], h2 = (cc.c[2] + rr.c[2]) + pl.c[2];
        const double fu = floor(l_K[s][0] * (h0 / h2) + l_K[s][2]), fv = floor(l_K[s][1] * (h1 / h2) + l_K[s][3]);
        if (h2 > 0.0 && fu >= 0.0 && fu < wlim && fv >= 0.0 && fv < hlim) {     // a NaN is outside
          const uint32_t other = a.census[(int64_t)j * px + (int64_t)(int)fv * width + (int)fu];
          const int cost = __popc(cen[n] ^ other);
          ++n_in;
          if (cost < OUT) {
            occ |= 1u << cost;
            if (cost < 12) lo += 1ull << (5 * cost);
            else hi += 1ull << (5 * (cost - 12));
          }
        }
      }
      int rem = a.best_views, sum = 0;
      while (occ != 0 && rem > 0) {
        const int c = __ffs((int)occ) - 1;
        occ &= occ - 1;
        const int cnt = (int)((c < 12 ? lo >> (5 * c) : hi >> (5 * (c - 12))) & 31ull), take = cnt < rem ? cnt : rem;
        sum += take * c;
        rem -= take;
      }
      sum += rem * OUT;
      l_slice[buf][q] = (uint16_t)(sum | (n_in << 9));
    }
    __syncthreads();
#pragma unroll
    for (int p = 0; p < PPT; ++p) {
      const uint16_t* mid = &l_slice[buf][(ty + p * ROWS_PER_ROUND + r) * hw + tx + r];
      int C = 0;
      for (int dy = -r; dy <= r; ++dy)
        for (int dx = -r; dx <= r; ++dx) C += mid[dy * hw + dx] & 511;
      if (k == (int)(m0[p] & 255u) + 1) cp[p] = C;            // the plane after the best so far
      uint32_t v = ((uint32_t)C << 8) | (uint32_t)k;
      if (v < m0[p]) {                                       // a new best: strictly lower C, as k only grows
        cm[p] = prev[p];
        nin[p] = mid[0] >> 9;
      }
      uint32_t t;
      t = v < m0[p] ? v : m0[p]; v = v < m0[p] ? m0[p] : v; m0[p] = t;
      t = v < m1[p] ? v : m1[p]; v = v < m1[p] ? m1[p] : v; m1[p] = t;
      t = v < m2[p] ? v : m2[p]; v = v < m2[p] ? m2[p] : v; m2[p] = t;
      m3[p] = v < m3[p] ? v : m3[p];
      prev[p] = C;
    }
  }

  int n_acc = 0, n_end = 0, n_amb = 0;
#pragma unroll
  for (int p = 0; p < PPT; ++p) {
    const int x = x0 + tx, y = y0 + ty + p * ROWS_PER_ROUND;
    if (x >= width || y >= height) continue;
    const int64_t i = base + (int64_t)y * width + x;
    const int kb = (int)(m0[p] & 255u), Cs = (int)(m0[p] >> 8);
    const auto apart = [&](uint32_t m) { const int d = (int)(m & 255u) - kb; return d > 1 || d < -1; };
    const int sec = (int)((apart(m1[p]) ? m1[p] : apart(m2[p]) ? m2[p] : m3[p]) >> 8);
    int status = DEPTHMVS_ACCEPTED;
    if (nin[p] < a.best_views) status = DEPTHMVS_UNSEEN;
    else if (kb == 0 || kb == D - 1) status = DEPTHMVS_END;
    else if (!((double)Cs <= a.uniqueness * (double)sec)) status = DEPTHMVS_AMBIGUOUS;
    float z32 = 0.f, s32 = 0.f;
    if (status == DEPTHMVS_ACCEPTED) {
      const int den = cm[p] - 2 * Cs + cp[p];
      const double off = den > 0 ? (double)(cm[p] - cp[p]) / (double)(2 * den) : 0.0;
      const double wk = a.inv_depth[kb];
      const double step = off < 0.0 ? wk - a.inv_depth[kb - 1] : a.inv_depth[kb + 1] - wk;
      const double w = wk + off * step, z = 1.0 / w;
      z32 = (float)z;
      s32 = (float)(((a.std_planes * z) * z) * step);
    }
    a.depth[i] = z32;
    a.std[i] = s32;
    a.status[i] = (uint8_t)status;
    if (a.plane != nullptr) a.plane[i] = (uint8_t)kb;
    if (a.cost != nullptr) a.cost[i] = (uint16_t)Cs;
    if (a.second != nullptr) a.second[i] = (uint16_t)sec;
    n_acc += status == DEPTHMVS_ACCEPTED;
    n_end += status == DEPTHMVS_END;
    n_amb += status == DEPTHMVS_AMBIGUOUS;
  }
  if (a.partial == nullptr) return;                          // (uniform)
  hipdev::wave_deposit(red, 0, hipdev::wave_sum_lane0(n_acc));
  hipdev::wave_deposit(red, 1, hipdev::wave_sum_lane0(n_end));
  hipdev::wave_deposit(red, 2, hipdev::wave_sum_lane0(n_amb));
  __syncthreads();
  if (tid < 4) a.partial[g * 4 + tid] = tid < 3 ? hipdev::waves_collect<int>(red, tid) : 0;
}

__global__ __launch_bounds__(64) void depthmvs_rows_kernel(int64_t tiles, int64_t frame_px, const int32_t* __restrict__ partial,
                                                           int64_t* __restrict__ rows) {
  const int f = blockIdx.x;
  long long s[3];
  depthprior::rows_partials<3, 4>(partial, tiles, f, s);
  if (threadIdx.x != 0) return;
  int64_t* o = rows + (int64_t)f * DEPTHMVS_ROW;
  o[DEPTHMVS_N_ACCEPTED] = s[0];
  o[DEPTHMVS_N_END] = s[1];
  o[DEPTHMVS_N_AMBIGUOUS] = s[2];
  o[DEPTHMVS_N_UNSEEN] = frame_px - ((s[0] + s[1]) + s[2]);
}

}  // namespace

void launch_depthmvs_census(hipStream_t st, const uint8_t* rgb, int height, int width, int64_t i0, int64_t n, uint32_t* census) {
  depthmvs_census_kernel<<<(unsigned)((n + BLOCK - 1) / BLOCK), BLOCK, 0, st>>>(rgb, height, width, i0, n, census);
}

void launch_depthmvs_sweep(hipStream_t st, const DepthmvsSweep& a, int64_t wg0, int64_t n_wg) {
  depthmvs_sweep_kernel<<<(unsigned)n_wg, BLOCK, 0, st>>>(a, wg0);
}

void launch_depthmvs_rows(hipStream_t st, int n_frames, int64_t tiles, int64_t frame_px, const int32_t* partial, int64_t* rows) {
  depthmvs_rows_kernel<<<n_frames, 64, 0, st>>>(tiles, frame_px, partial, rows);
}

// Completing sparse depth priors by image-guided filtering.  Float64 in the written order of
// tests/depth_complete_reference.py, compiled with -ffp-contract=off.
//
//   pass   grid (frames x tiles), 256 threads: a tile of 32 x 16 pixels of one frame, two pixels per thread (rows ty and ty + 8).
//          The threads read their own pixels' state first; a tile without an empty pixel writes them back and leaves (a dense prior
//          costs one read and one write).  Otherwise the state of the tile and its halo of `radius` pixels and their colour, packed
//          into 32 bits, go to LDS as 16-byte cells (z, c, v, colour) with the two weight tables.  The tile's empty pixels are
//          compacted into a list (ballots and per-wave counts, no atomic), and thread t takes entries t, t + 256: after the first
//          pass few pixels of a tile are empty, and the walk is paid for those alone.  A walk visits every tap in raster order
//          (a cell outside the frame is marked in its colour word and weighs 0, so the loops are scalar): one 16-byte LDS read, one
//          v_sad_u8 for the colour distance, two table reads and the float64 sums, without a branch.  A tile with no confidence anywhere in tile and halo skips the walk: every pixel of it is NONE whatever the
//          weights say.  The first pass builds the state from depth and std_in as it reads; the last writes the outputs in their
//          final form and the tile's three counts (wave sums, added over the four waves in wave order).
//   rows   grid (frames), 64 threads: lane l adds the partials of tiles l, l + 64, ... and a shfl_down tree adds the lanes.  The
//          partials are integers, so every order gives the same bits.
#include "depthcomp_kernels.h"
#include "depth_prior_device.h"

namespace {

constexpr int BLOCK = DEPTHCOMP_BLOCK, TW = DEPTHCOMP_TILE_W, TH = DEPTHCOMP_TILE_H, PPT = DEPTHCOMP_PPT, WAVES = BLOCK / 64;
constexpr int RMAX = DEPTHCOMP_MAX_RADIUS, ROWS_PER_ROUND = BLOCK / TW;
constexpr int NC = DEPTHCOMP_COLOUR_TABLE;
// A cell outside the frame carries 255 in the fourth byte of its colour, which no pixel has.  Its tap is given g = 0, so gc = 0: it
// adds +0.0 to G, which is never negative, and is skipped -- as the definition skips it -- while every walk has the same trip counts
// and the loops are scalar.  Its colour distance is 255 .. 1020, so the colour table in LDS goes on, with zeros, up to there.
constexpr uint32_t OUTSIDE = 0xff000000u;
constexpr int NC_LDS = NC + 255;

// the state of pixel i as a pass reads it: the first pass from the inputs, every later one from the state before it
template <bool FIRST>
__device__ __forceinline__ void read_state(const DepthcompPass& a, int64_t i, float& z, float& c, float& v) {
  if constexpr (FIRST) {
    const float d = a.depth[i];
    const bool valid = d > 0.f;                              // 0, negatives and NaN are not
    z = valid ? d : 0.f;
    c = valid ? 1.f : 0.f;
    v = 0.f;
    if (valid && a.std_in != nullptr) {
      const float s = a.std_in[i];
      if (s > 0.f) v = (float)((double)s * (double)s);
    }
  } else {
    z = a.in.z[i];
    c = a.in.c[i];
    v = a.in.v[i];
  }
}

// a cell of the tile and its halo in LDS: one 16-byte read per tap
struct __attribute__((aligned(16))) Cell {
  float z, c, v;
  uint32_t rgb;
};

template <bool FIRST, bool LAST>
__global__ __launch_bounds__(BLOCK) void depthcomp_pass_kernel(const DepthcompPass a, int64_t wg0) {
  // LDS sized by the launch for the call's radius (pass_lds_bytes): the cells of tile and halo, the colour table, the window's
  // weights, then the tile's empty pixels, compacted (ty * TW + tx).  A smaller radius leaves room for more workgroups per CU.
  extern __shared__ __attribute__((aligned(16))) unsigned char l_raw[];
  const int r = a.radius, hw = TW + 2 * r, hh = TH + 2 * r, side = 2 * r + 1;
  Cell* const l_cell = (Cell*)l_raw;
  double* const l_wc = (double*)(l_raw + (size_t)hh * hw * sizeof(Cell));
  double* const l_ws = l_wc + NC_LDS;
  uint16_t* const l_list = (uint16_t*)(l_ws + side * side);
  __shared__ int l_count[PPT][WAVES];
  __shared__ int red[WAVES][3];
  const int tid = threadIdx.x, tx = tid % TW, ty = tid / TW, lane = tid & 63, wave = tid >> 6;
  const int64_t g = wg0 + (int64_t)blockIdx.x;
  const int64_t f = g / a.tiles, tile = g % a.tiles;
  const int x0 = (int)(tile % a.tiles_x) * TW, y0 = (int)(tile / a.tiles_x) * TH;
  const int height = a.height, width = a.width;
  const int64_t base = f * ((int64_t)height * width);

  // The thread's own two pixels.  One with confidence is carried: written back below by this thread.  The empty ones are compacted
  // into l_list, so that the window walk runs on full waves of them whatever share of the tile they are.
  float z[PPT], c[PPT], v[PPT];
  int ps[PPT];
  int64_t at[PPT];                                           // the pixel's index in its plane, -1 outside the frame
  bool empty[PPT];
  unsigned long long mask[PPT];
  const int x = x0 + tx;
  bool any_conf = false, any_empty = false;
#pragma unroll
  for (int k = 0; k < PPT; ++k) {
    const int y = y0 + ty + k * ROWS_PER_ROUND;
    at[k] = x < width && y < height ? base + (int64_t)y * width + x : -1;
    z[k] = c[k] = v[k] = 0.f;
    ps[k] = 0;
    if (at[k] >= 0) {
      read_state<FIRST>(a, at[k], z[k], c[k], v[k]);
      if constexpr (!FIRST) ps[k] = a.in.pass[at[k]];
    }
    empty[k] = at[k] >= 0 && !(c[k] > 0.f);
    any_conf |= c[k] > 0.f;
    any_empty |= empty[k];
  }
  int n_own = 0, n_filled = 0, n_refused = 0;
  if (__syncthreads_or(any_empty)) {                         // (uniform) a tile without an empty pixel copies and leaves
#pragma unroll
    for (int k = 0; k < PPT; ++k) {
      mask[k] = __ballot(empty[k]);
      if (lane == 0) l_count[k][wave] = (int)__popcll(mask[k]);
    }
    __syncthreads();
    int n_empty = 0;                                         // the list in (round, wave, lane) order; in the end the tile's count
#pragma unroll
    for (int k = 0; k < PPT; ++k) {
#pragma unroll
      for (int w = 0; w < WAVES; ++w) {
        if (w == wave && empty[k])
          l_list[n_empty + (int)__popcll(mask[k] & ((1ull << lane) - 1ull))] = (uint16_t)((ty + k * ROWS_PER_ROUND) * TW + tx);
        n_empty += l_count[k][w];
      }
    }
    const int cells = hh * hw;
    for (int q = tid; q < cells; q += BLOCK) {
      const int hy = q / hw, hx = q - hy * hw;
      const int gy = y0 + hy - r, gx = x0 + hx - r;
      const bool interior = hy >= r && hy < r + TH && hx >= r && hx < r + TW;
      uint32_t colour = OUTSIDE;
      float qz = 0.f, qc = 0.f, qv = 0.f;
      if (gy >= 0 && gy < height && gx >= 0 && gx < width) {
        const int64_t i = base + (int64_t)gy * width + gx;
        const uint8_t* p = a.rgb + 3 * i;
        colour = (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16);
        if (!interior) read_state<FIRST>(a, i, qz, qc, qv);
      }
      l_cell[q].rgb = colour;
      if (!interior) {                                       // the tile's own cells come from the registers below
        l_cell[q].z = qz;
        l_cell[q].c = qc;
        l_cell[q].v = qv;
        any_conf |= qc > 0.f;
      }
    }
#pragma unroll
    for (int k = 0; k < PPT; ++k) {
      const int q = (ty + k * ROWS_PER_ROUND + r) * hw + tx + r;
      l_cell[q].z = z[k];
      l_cell[q].c = c[k];
      l_cell[q].v = v[k];
    }
    for (int q = tid; q < side * side; q += BLOCK) l_ws[q] = a.w_space[q];
    for (int q = tid; q < NC_LDS; q += BLOCK) l_wc[q] = q < NC ? a.w_colour[q] : 0.0;
    // (uniform; the barrier the LDS reads below wait for)  Without confidence anywhere in tile and halo every pixel is NONE.
    const bool walk = __syncthreads_or(any_conf);
    for (int e = tid; e < n_empty; e += BLOCK) {
      const int id = l_list[e], py = id / TW, px = id % TW;
      const int ly = py + r, lx = px + r, gy = y0 + py, gx = x0 + px;
      const int64_t i = base + (int64_t)gy * width + gx;
      float zf = 0.f, cf = 0.f, vf = 0.f;
      int status = DEPTHCOMP_ORIGIN_NONE;
      if (walk) {
        const uint32_t mine = l_cell[ly * hw + lx].rgb;
        double G = 0.0, S = 0.0, SZ = 0.0, SZZ = 0.0, SV = 0.0;
        int n = 0;
        for (int dy = -r; dy <= r; ++dy) {                   // every tap, in raster order
          const Cell* row = l_cell + (ly + dy) * hw + lx;
          const double* wrow = l_ws + (dy + r) * side + r;
          for (int dx = -r; dx <= r; ++dx) {
            const Cell q = row[dx];
            const double gw = wrow[dx] * l_wc[__builtin_amdgcn_sad_u8(mine, q.rgb, 0u)], gq = q.rgb >= OUTSIDE ? 0.0 : gw;
            G += gq;
            // A tap with gc = 0 is skipped: it adds +0.0 to sums that are never negative, which changes no bit, once its depth and
            // variance are taken as 0 too (0 * inf would be a NaN).  No branch: the taps' loads run ahead of the sums.
            const double gc = gq * (double)q.c;
            const bool use = gc > 0.0;
            const double gcu = use ? gc : 0.0, zq = (double)(use ? q.z : 0.f), vq = (double)(use ? q.v : 0.f);
            n += use ? 1 : 0;
            S += gcu;
            const double t = gcu * zq;
            SZ += t;
            SZZ += t * zq;
            SV += gcu * vq;
          }
        }
        if (n >= a.min_points && G > 0.0) {                  // step 3
          const double conf = S / G;
          if (!(conf < a.min_conf)) {
            const double mean = SZ / S, d = SZZ / S - mean * mean, var = d > 0.0 ? d : 0.0;   // step 4
            if (sqrt(var) > a.max_rel_spread * mean) {
              status = DEPTHCOMP_ORIGIN_REFUSED;
            } else {
              const float z32 = (float)mean, c32 = (float)(a.decay * conf), v32 = (float)(var + SV / S);   // step 5
              if (z32 > 0.f && z32 < __builtin_inff() && c32 > 0.f) {
                zf = z32;
                cf = c32;
                vf = v32;
              }
            }
          }
        }
      }
      const bool have = cf > 0.f;
      if constexpr (!LAST) {
        a.out.z[i] = zf;
        a.out.c[i] = cf;
        a.out.v[i] = vf;
        a.out.pass[i] = (uint8_t)(have ? a.k : 0);
      } else {
        a.out.z[i] = have ? zf : a.depth[i];                 // an input that is not replaced keeps its bits
        a.out.v[i] = have ? (float)sqrt((double)vf) : 0.f;
        if (a.out.c != nullptr) a.out.c[i] = cf;
        if (a.out.pass != nullptr) a.out.pass[i] = (uint8_t)(have ? a.k : 0);
        a.origin[i] = (uint8_t)(have ? DEPTHCOMP_ORIGIN_FILLED : status);
        n_filled += have;
        n_refused += !have && status == DEPTHCOMP_ORIGIN_REFUSED;
      }
    }
  }

  // the carried pixels: unchanged
#pragma unroll
  for (int k = 0; k < PPT; ++k) {
    const int64_t i = at[k];
    if (i < 0 || empty[k]) continue;
    if constexpr (!LAST) {
      a.out.z[i] = z[k];
      a.out.c[i] = c[k];
      a.out.v[i] = v[k];
      a.out.pass[i] = (uint8_t)ps[k];
    } else {
      a.out.z[i] = z[k];
      a.out.v[i] = (float)sqrt((double)v[k]);
      if (a.out.c != nullptr) a.out.c[i] = c[k];
      if (a.out.pass != nullptr) a.out.pass[i] = (uint8_t)ps[k];
      a.origin[i] = (uint8_t)(ps[k] == 0 ? DEPTHCOMP_ORIGIN_OWN : DEPTHCOMP_ORIGIN_FILLED);
      n_own += ps[k] == 0;
      n_filled += ps[k] != 0;
    }
  }
  if constexpr (LAST) {
    if (a.partial == nullptr) return;                        // (uniform)
    hipdev::wave_deposit(red, 0, hipdev::wave_sum_lane0(n_own));
    hipdev::wave_deposit(red, 1, hipdev::wave_sum_lane0(n_filled));
    hipdev::wave_deposit(red, 2, hipdev::wave_sum_lane0(n_refused));
    __syncthreads();
    if (tid < 4) a.partial[g * 4 + tid] = tid < 3 ? hipdev::waves_collect<int>(red, tid) : 0;
  }
}

__global__ __launch_bounds__(64) void depthcomp_rows_kernel(int64_t tiles, int64_t frame_px, const int32_t* __restrict__ partial,
                                                            int64_t* __restrict__ rows) {
  const int f = blockIdx.x;
  long long s[3];
  depthprior::rows_partials<3, 4>(partial, tiles, f, s);
  if (threadIdx.x != 0) return;
  int64_t* o = rows + (int64_t)f * DEPTHCOMP_ROW;
  o[DEPTHCOMP_N_OWN] = s[0];
  o[DEPTHCOMP_N_FILLED] = s[1];
  o[DEPTHCOMP_N_REFUSED] = s[2];
  o[DEPTHCOMP_N_NONE] = frame_px - ((s[0] + s[1]) + s[2]);
}

}  // namespace

// bytes of the pass kernel's LDS at a radius: 15.4 + 8.2 + 0.6 + 1 KB at radius 4, 24.6 + 8.2 + 2.3 + 1 KB at radius 8
constexpr size_t pass_lds_bytes(int radius) {
  return (TH + 2 * (size_t)radius) * (TW + 2 * (size_t)radius) * sizeof(Cell) +
         (NC_LDS + (2 * (size_t)radius + 1) * (2 * (size_t)radius + 1)) * sizeof(double) + TW * TH * sizeof(uint16_t);
}
static_assert(pass_lds_bytes(RMAX) <= 48 * 1024, "the widest window fits the LDS a launch may ask for without an attribute");

void launch_depthcomp_pass(hipStream_t st, const DepthcompPass& a, bool first, bool last, int64_t wg0, int64_t n_wg) {
  const unsigned n = (unsigned)n_wg;
  const size_t lds = pass_lds_bytes(a.radius);
  if (first && last) depthcomp_pass_kernel<true, true><<<n, BLOCK, lds, st>>>(a, wg0);
  else if (first) depthcomp_pass_kernel<true, false><<<n, BLOCK, lds, st>>>(a, wg0);
  else if (last) depthcomp_pass_kernel<false, true><<<n, BLOCK, lds, st>>>(a, wg0);
  else depthcomp_pass_kernel<false, false><<<n, BLOCK, lds, st>>>(a, wg0);
}

void launch_depthcomp_rows(hipStream_t st, int n_frames, int64_t tiles, int64_t frame_px, const int32_t* partial, int64_t* rows) {
  depthcomp_rows_kernel<<<n_frames, 64, 0, st>>>(tiles, frame_px, partial, rows);
}

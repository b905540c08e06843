// Semi-global smoothing of the plane sweep.  Integer arithmetic throughout; the refinement is the sweep's
// (depthmvs_sweep.h: decide), compiled with -ffp-contract=off like it.
//
//   census  the sweep's, over all frames of the call: neighbours cross chunks.
//   slab    the sweep's plane loop with SLAB = true (depthmvs_sweep.h), over the frames of a chunk: C(p, k) | unseen << 15 as
//           uint16 into cslab [frame, y, x, k], rows of dp = n_planes rounded up to 8 planes.
//   paths   one launch per direction, grid (frames x lines / 4), 256 threads: one wave walks one scanline from the pixel whose
//           predecessor is outside the frame to the last one inside.  The planes sit on the lanes: lane l holds plane l
//           (n_planes <= 64) or planes 4 l .. 4 l + 3 (up to 256), a plane past the table holds INF.  A step loads the next pixel's C
//           (2 or 8 bytes per lane) and, for every direction but the first, the pixel's S (4 or 16 bytes per lane) ahead of the
//           recurrence, takes L(k - 1) and L(k + 1) by one shuffle each, M by a butterfly of shuffles, and stores or adds L into
//           sslab [frame, y, x, k] uint32.  Within a launch every (pixel, plane) belongs to one wave; the launches are ordered on
//           the stream, so the sum needs no atomics and has one order.
//   select  grid (frames x tiles), 256 threads, the sweep's tile and thread -> pixel map: a thread reads the S curve of its two
//           pixels in 16-byte loads through the sweep's running state (Running), the unseen bit of the winner from cslab, and
//           applies the sweep's steps 6 and 7 (decide).  The tile's partials are the sweep's; the rows launch is the sweep's.
#include "depthsgm_kernels.h"
#include "depthmvs_sweep.h"

using namespace depthmvs_dev;

namespace {

constexpr int INF = 1 << 20;                                 // above every L (< 2^16); INF + P2 and 8 INF fit easily
constexpr int PATH_BLOCK = 64 * DEPTHSGM_PATH_WAVES;

__device__ __forceinline__ int mini(int a, int b) { return a < b ? a : b; }

__device__ __forceinline__ int wave_min(int v) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) v = mini(v, __shfl_xor(v, d, 64));
  return v;
}

template <int NPL>
__global__ __launch_bounds__(PATH_BLOCK) void depthsgm_paths_kernel(const DepthsgmPaths a, int64_t wg0) {
  static_assert(NPL == 1 || NPL == 4, "one plane per lane, or four in a row");
  const int lane = threadIdx.x & 63;
  const int64_t w = (wg0 + (int64_t)blockIdx.x) * DEPTHSGM_PATH_WAVES + (threadIdx.x >> 6);
  if (w >= (int64_t)a.frames * a.lines) return;              // (uniform in the wave; the kernel has no barrier)
  const int64_t fl = w / a.lines;
  const int l = (int)(w % a.lines);
  const int H = a.height, W = a.width, dx = a.dx, dy = a.dy, D = a.n_planes;
  // the line's first pixel: the one whose predecessor is outside.  Diagonals enter along the row they start from (all of it) and
  // along the column (without the corner).
  int x, y;
  if (dy == 0) { x = dx > 0 ? 0 : W - 1; y = l; }
  else if (dx == 0) { x = l; y = dy > 0 ? 0 : H - 1; }
  else if (l < W) { x = l; y = dy > 0 ? 0 : H - 1; }
  else { const int t = l - W + 1; x = dx > 0 ? 0 : W - 1; y = dy > 0 ? t : H - 1 - t; }
  const int nx = dx > 0 ? W - x : dx < 0 ? x + 1 : 0x7fffffff, ny = dy > 0 ? H - y : dy < 0 ? y + 1 : 0x7fffffff;
  const int n = mini(nx, ny);                                // pixels of the line

  const int k0 = lane * NPL;
  const bool act = k0 < a.dp;                                // the lane has entries in the slabs' rows
  const int64_t px = (int64_t)H * W;
  const int64_t step = ((int64_t)dy * W + dx) * a.dp;        // entries from a pixel to the next
  int64_t at = (fl * px + (int64_t)y * W + x) * a.dp + k0;
  const uint8_t* img = a.rgb + 3 * fl * px;
  const auto luma = [&](int xx, int yy) {
    const uint8_t* p = img + 3 * ((int64_t)yy * W + xx);
    return (77 * (int)p[0] + 150 * (int)p[1] + 29 * (int)p[2] + 128) >> 8;
  };
  const auto load_c = [&](int64_t i, int (&c)[NPL]) {
    if constexpr (NPL == 1) {
      c[0] = act ? (int)a.cslab[i] : 0;
    } else {
      const uint2 v = act ? *(const uint2*)(a.cslab + i) : make_uint2(0, 0);
      c[0] = (int)(v.x & 0xffffu); c[1] = (int)(v.x >> 16); c[2] = (int)(v.y & 0xffffu); c[3] = (int)(v.y >> 16);
    }
  };

  int L[NPL], c_next[NPL];
  load_c(at, c_next);
  int y_prev = 0;
  for (int i = 0; i < n; ++i) {
    int c[NPL];
#pragma unroll
    for (int j = 0; j < NPL; ++j) c[j] = c_next[j] & 0x7fff;
    if (i + 1 < n) load_c(at + step, c_next);                // the next pixel's C, ahead of the recurrence
    uint32_t s_old[NPL] = {};
    if (!a.first && act) {
      if constexpr (NPL == 1) {
        s_old[0] = a.sslab[at];
      } else {
        const uint4 v = *(const uint4*)(a.sslab + at);
        s_old[0] = v.x; s_old[1] = v.y; s_old[2] = v.z; s_old[3] = v.w;
      }
    }
    int p2 = a.p2;
    if (a.edge > 0) {                                        // (uniform)
      const int y_here = luma(x, y);
      if (i > 0) {
        const int d = y_here > y_prev ? y_here - y_prev : y_prev - y_here;
        p2 = a.p2 / (1 + d / a.edge);
        p2 = p2 < a.p1 ? a.p1 : p2;
      }
      y_prev = y_here;
    }
    if (i == 0) {
#pragma unroll
      for (int j = 0; j < NPL; ++j) L[j] = k0 + j < D ? c[j] : INF;
    } else {
      int m = L[0];
#pragma unroll
      for (int j = 1; j < NPL; ++j) m = mini(m, L[j]);
      const int M = wave_min(m);
      int up = __shfl_up(L[NPL - 1], 1, 64), dn = __shfl_down(L[0], 1, 64);       // L(k0 - 1) and L(k0 + NPL) of the lane
      if (lane == 0) up = INF;
      if (lane == 63) dn = INF;
      int Ln[NPL];
#pragma unroll
      for (int j = 0; j < NPL; ++j) {
        const int below = j == 0 ? up : L[j - 1], above = j == NPL - 1 ? dn : L[j + 1];
        const int t = mini(mini(L[j], mini(below, above) + a.p1), M + p2);
        Ln[j] = k0 + j < D ? c[j] + t - M : INF;
      }
#pragma unroll
      for (int j = 0; j < NPL; ++j) L[j] = Ln[j];
    }
    if (act) {                                               // (planes D .. dp - 1 of the row are written and never read)
      if constexpr (NPL == 1) {
        a.sslab[at] = s_old[0] + (uint32_t)L[0];
      } else {
        *(uint4*)(a.sslab + at) = make_uint4(s_old[0] + (uint32_t)L[0], s_old[1] + (uint32_t)L[1], s_old[2] + (uint32_t)L[2],
                                             s_old[3] + (uint32_t)L[3]);
      }
    }
    at += step;
    x += dx;
    y += dy;
  }
}

__global__ __launch_bounds__(BLOCK) void depthsgm_select_kernel(const DepthsgmSelect a, int64_t wg0) {
  __shared__ int red[WAVES][3];
  const int tid = threadIdx.x, tx = tid % TW, ty = tid / TW;
  const int64_t gl = wg0 + (int64_t)blockIdx.x;              // (frame of the chunk, tile)
  const int64_t fl = gl / a.tiles, tile = gl % a.tiles;
  const int x0 = (int)(tile % a.tiles_x) * TW, y0 = (int)(tile / a.tiles_x) * TH;
  const int height = a.height, width = a.width, D = a.n_planes;
  const int64_t px = (int64_t)height * width;
  int n_acc = 0, n_end = 0, n_amb = 0;
#pragma unroll
  for (int p = 0; p < PPT; ++p) {
    const int x = x0 + tx, y = y0 + ty + p * ROWS_PER_ROUND;
    if (x >= width || y >= height) continue;
    const int64_t row = (fl * px + (int64_t)y * width + x) * a.dp;
    const uint32_t* S = a.sslab + row;
    Running run;
    run.init();
    for (int k = 0; k < D; k += 4) {                         // dp is a multiple of 8: the load stays in the pixel's row
      const uint4 v = *(const uint4*)(S + k);
      run.step((int)v.x, k);
      if (k + 1 < D) run.step((int)v.y, k + 1);
      if (k + 2 < D) run.step((int)v.z, k + 2);
      if (k + 3 < D) run.step((int)v.w, k + 3);
    }
    const int kb = run.plane(), Cs = run.cost(), sec = run.second();
    const bool seen = (a.cslab[row + kb] & 0x8000) == 0;
    const Decision d = decide(a.inv_depth, D, a.uniqueness, a.std_planes, seen, kb, Cs, sec, run.cm, run.cp);
    const int64_t i = (a.f0 + fl) * px + (int64_t)y * width + x;
    a.depth[i] = d.z;
    a.std[i] = d.s;
    a.status[i] = (uint8_t)d.status;
    if (a.plane != nullptr) a.plane[i] = (uint8_t)kb;
    if (a.cost != nullptr) a.cost[i] = (uint32_t)Cs;
    if (a.second != nullptr) a.second[i] = (uint32_t)sec;
    n_acc += d.status == DEPTHMVS_ACCEPTED;
    n_end += d.status == DEPTHMVS_END;
    n_amb += d.status == DEPTHMVS_AMBIGUOUS;
  }
  if (a.partial == nullptr) return;                          // (uniform)
  tile_partials(red, a.partial, (a.f0 + fl) * a.tiles + tile, n_acc, n_end, n_amb);
}

}  // namespace

void launch_depthsgm_census(hipStream_t st, const uint8_t* rgb, int height, int width, int64_t i0, int64_t n, uint32_t* census) {
  depthmvs_census_kernel<<<(unsigned)((n + BLOCK - 1) / BLOCK), BLOCK, 0, st>>>(rgb, height, width, i0, n, census);
}

void launch_depthsgm_slab(hipStream_t st, const DepthmvsSweep& a, int64_t wg0, int64_t n_wg) {
  depthmvs_sweep_kernel<true><<<(unsigned)n_wg, BLOCK, 0, st>>>(a, wg0);
}

void launch_depthsgm_paths(hipStream_t st, const DepthsgmPaths& a, int64_t wg0, int64_t n_wg) {
  if (a.n_planes <= 64) depthsgm_paths_kernel<1><<<(unsigned)n_wg, PATH_BLOCK, 0, st>>>(a, wg0);
  else depthsgm_paths_kernel<4><<<(unsigned)n_wg, PATH_BLOCK, 0, st>>>(a, wg0);
}

void launch_depthsgm_select(hipStream_t st, const DepthsgmSelect& a, int64_t wg0, int64_t n_wg) {
  depthsgm_select_kernel<<<(unsigned)n_wg, BLOCK, 0, st>>>(a, wg0);
}

void launch_depthsgm_rows(hipStream_t st, int n_frames, int64_t tiles, int64_t frame_px, const int32_t* partial, int64_t* rows) {
  depthmvs_rows_kernel<<<n_frames, 64, 0, st>>>(tiles, frame_px, partial, rows);
}

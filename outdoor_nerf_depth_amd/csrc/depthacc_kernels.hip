// Densifying sparse depth priors from neighbouring frames.  The geometry in float64 in the written order of
// tests/depth_accumulate_reference.py, compiled with -ffp-contract=off.
//
//   scatter  grid (frames x slots x scatter tiles), 256 threads: a workgroup takes 2048 consecutive pixels of the source frame
//            j = nbr[i][v] into the target frame i.  Both cameras are wave-uniform loads (scalar registers).  A sparse prior leaves
//            most pixels invalid, so the workgroup first compacts its valid pixels into LDS (ballot + one LDS add per wave and
//            round) and then spends the float64 work on full waves of them.  A pixel that lands on a target pixel with a measurement
//            of its own is dropped: that key could never be seen (a dense prior issues no atomic at all).  Every other one is ONE
//            global_atomic_umin_x2 on the 8-byte key (z bits, slot, source pixel): a minimum over integers, the same bits for every
//            order of arrival.
//   resolve  grid (frames x tiles), 256 threads: a tile of 32 x 8 pixels of one frame, one thread per pixel.  The surface values of
//            the tile and its halo of occl_radius pixels go to LDS, every one read from memory once, in two rounds of loads that are
//            all in flight together (the depths, then the keys of the pixels without a depth); the window minimum is two separable
//            passes (along the rows, then down the columns).  The three counts of the tile are ballots, added over the
//            four waves in wave order.
//   rows     grid (frames), 64 threads: lane l adds the partials of tiles l, l + 64, ... and a shfl_down tree adds the lanes.  The
//            partials are integers, so every order gives the same bits.
#include "depthacc_kernels.h"
#include "depth_prior_device.h"

namespace {

using depthprior::P3, depthprior::FX, depthprior::FY, depthprior::CX, depthprior::CY;
constexpr int BLOCK = DEPTHACC_BLOCK, TW = DEPTHACC_TILE_W, TH = DEPTHACC_TILE_H, WAVES = BLOCK / 64, CAM = DEPTHACC_CAM;
constexpr int STILE = DEPTHACC_SCATTER_TILE;
constexpr uint64_t EMPTY = depthprior::EMPTY_KEY;
using Window = depthprior::Window<TW, TH, DEPTHACC_MAX_RADIUS, BLOCK>;   // the visibility window of the resolve (depth_prior_device.h)
constexpr int HALO_ROUNDS = Window::HALO_ROUNDS;

__global__ __launch_bounds__(BLOCK) void depthacc_scatter_kernel(int n_frames, int height, int width, int n_views, int64_t wg0,
                                                                int64_t tiles, const float* __restrict__ depth,
                                                                const double* __restrict__ cams, const int32_t* __restrict__ nbr,
                                                                unsigned long long* __restrict__ zbuf) {
  __shared__ float l_d[STILE];                               // the valid pixels of the tile, compacted: depth and pixel index
  __shared__ int l_p[STILE];
  __shared__ int l_n;
  const int tid = threadIdx.x, lane = tid & 63;
  const int64_t g = wg0 + (int64_t)blockIdx.x;
  const int64_t tile = g % tiles, slot = g / tiles;
  const int i = (int)(slot / n_views), v = (int)(slot % n_views);
  const int j = nbr[(int64_t)i * n_views + v];
  if (j < 0 || j >= n_frames) return;                        // (uniform) an index outside the batch is skipped: no read outside the buffers
  const int64_t frame_px = (int64_t)height * width;
  const float* dj = depth + (int64_t)j * frame_px;
  if (tid == 0) l_n = 0;
  __syncthreads();
  float dk[STILE / BLOCK];                                   // every load of the tile is in flight before the first is looked at
#pragma unroll
  for (int k = 0; k < STILE / BLOCK; ++k) {
    const int64_t p = tile * STILE + k * BLOCK + tid;
    dk[k] = p < frame_px ? dj[p] : 0.f;
  }
#pragma unroll
  for (int k = 0; k < STILE / BLOCK; ++k) {
    const int64_t p = tile * STILE + k * BLOCK + tid;
    const float d = dk[k];
    const bool valid = d > 0.f;                              // 0, negatives and NaN are invalid
    const unsigned long long m = __ballot(valid);
    if (m != 0) {                                            // (wave-uniform)
      int base = 0;
      if (lane == 0) base = atomicAdd(&l_n, __popcll(m));
      base = __shfl(base, 0, 64);
      if (valid) {
        const int pos = base + __popcll(m & ((1ull << lane) - 1ull));
        l_d[pos] = d;
        l_p[pos] = (int)p;
      }
    }
  }
  __syncthreads();
  const int n = l_n;
  if (n == 0) return;
  const double* cj = cams + (int64_t)j * CAM;
  const double* ci = cams + (int64_t)i * CAM;
  const float* di = depth + (int64_t)i * frame_px;
  unsigned long long* zi = zbuf + (int64_t)i * frame_px;
  const double w_d = (double)width, h_d = (double)height;
  for (int q = tid; q < n; q += BLOCK) {
    const int p = l_p[q];
    const double d = (double)l_d[q];
    const int y = p / width, x = p - y * width;
    // steps 1, 2: Pc = ((x + 0.5 - cx) / fx * d, (y + 0.5 - cy) / fy * d, d), Pw = R_j Pc + t_j; step 3: P = R_i^T (Pw - t_i)
    const P3 pc = depthprior::world_to_cam(ci, depthprior::pixel_to_world(cj, (double)x + 0.5, (double)y + 0.5, d));
    if (!(pc.z > 0.0)) continue;                             // step 4
    const double u = ci[FX] * (pc.x / pc.z) + ci[CX], w = ci[FY] * (pc.y / pc.z) + ci[CY];   // step 5
    if (!(u >= 0.0 && u < w_d && w >= 0.0 && w < h_d)) continue;   // step 6: in float64, before any integer; a NaN is outside
    const int tx = (int)floor(u), ty = (int)floor(w);        // step 7: 0 .. width - 1, 0 .. height - 1
    const float z32 = (float)pc.z;                           // step 8: to nearest
    if (!(z32 > 0.f && z32 < __builtin_inff())) continue;
    const int64_t t = (int64_t)ty * width + tx;
    if (di[t] > 0.f) continue;                               // the target has its own measurement: this key would never be read
    const unsigned long long key = ((unsigned long long)__float_as_uint(z32) << 32) | ((unsigned long long)(unsigned)v << 28) |
                                   (unsigned long long)(unsigned)p;   // step 9
    atomicMin(zi + t, key);                                  // step 10
  }
}

__global__ __launch_bounds__(BLOCK) void depthacc_resolve_kernel(int height, int width, int64_t wg0, int tiles_x, int64_t tiles,
                                                                const float* __restrict__ depth,
                                                                const unsigned long long* __restrict__ zbuf, int radius,
                                                                double one_plus_tol, float* __restrict__ depth_out,
                                                                uint8_t* __restrict__ origin, int32_t* __restrict__ src,
                                                                int32_t* __restrict__ partial) {
  __shared__ float surf[Window::SURF];                       // surface values of the tile and its halo, +inf outside the frame
  __shared__ float rowmin[Window::ROWMIN];                   // their minimum over the window's columns
  __shared__ int red[WAVES][3];
  const int tid = threadIdx.x, tx = tid % TW, ty = tid / TW;
  const int64_t g = wg0 + (int64_t)blockIdx.x;
  const int64_t f = g / tiles, tile = g % tiles;
  const int x0 = (int)(tile % tiles_x) * TW, y0 = (int)(tile / tiles_x) * TH;
  const int r = radius, hw = TW + 2 * r;
  const int64_t frame_px = (int64_t)height * width;
  const float* df = depth + f * frame_px;
  const unsigned long long* zf = zbuf + f * frame_px;

  // The thread's own pixel and its share of the halo ring (cells tid, tid + 256, ...).  Two rounds of loads, each with every load in
  // flight at once: the depths, then the keys of the pixels that have no measurement of their own.
  const int x = x0 + tx, y = y0 + ty;
  const bool inside = x < width && y < height;
  const int64_t t = (int64_t)y * width + x;
  int ht[HALO_ROUNDS], hc[HALO_ROUNDS];                      // a halo cell's index in the frame (-1: outside it) and in surf (-1: none)
  float hs[HALO_ROUNDS];
  Window::halo_cells(tid, x0, y0, r, height, width, hc, ht);
  const float own = inside ? df[t] : 0.f;
#pragma unroll
  for (int k = 0; k < HALO_ROUNDS; ++k) hs[k] = ht[k] >= 0 ? df[ht[k]] : __builtin_inff();
  const bool own_valid = own > 0.f;                          // 0, negatives and NaN are not
  unsigned long long key = EMPTY, hk[HALO_ROUNDS];
  if (inside && !own_valid) key = zf[t];
#pragma unroll
  for (int k = 0; k < HALO_ROUNDS; ++k) {
    hk[k] = EMPTY;
    if (ht[k] >= 0 && !(hs[k] > 0.f)) hk[k] = zf[ht[k]];
  }
  const bool cand = inside && !own_valid && key != EMPTY;
  const float z = __uint_as_float((unsigned)(key >> 32));
  surf[(ty + r) * hw + tx + r] = own_valid ? own : cand ? z : __builtin_inff();
#pragma unroll
  for (int k = 0; k < HALO_ROUNDS; ++k)
    if (hc[k] >= 0)
      surf[hc[k]] = hs[k] > 0.f ? hs[k] : hk[k] != EMPTY ? __uint_as_float((unsigned)(hk[k] >> 32)) : __builtin_inff();
  const float zmin = Window::window_min(surf, rowmin, tid, r);
  const bool hidden = cand && (double)z > (double)zmin * one_plus_tol;
  const bool added = cand && !hidden;
  if (inside) {
    const int64_t o = f * frame_px + t;
    depth_out[o] = added ? z : own;                          // an input that is not replaced keeps its bits
    if (origin != nullptr)
      origin[o] = (uint8_t)(own_valid ? DEPTHACC_ORIGIN_OWN : !cand ? DEPTHACC_ORIGIN_NONE : added ? DEPTHACC_ORIGIN_ADDED : DEPTHACC_ORIGIN_HIDDEN);
    if (src != nullptr) src[o] = cand ? (int32_t)(unsigned)key : -1;
  }
  if (partial == nullptr) return;                            // (uniform)
  hipdev::wave_deposit(red, 0, (int)__popcll(__ballot(own_valid)));
  hipdev::wave_deposit(red, 1, (int)__popcll(__ballot(cand)));
  hipdev::wave_deposit(red, 2, (int)__popcll(__ballot(added)));
  __syncthreads();
  if (tid < 4) partial[g * 4 + tid] = tid < 3 ? hipdev::waves_collect<int>(red, tid) : 0;
}

__global__ __launch_bounds__(64) void depthacc_rows_kernel(int64_t tiles, const int32_t* __restrict__ partial, int64_t* __restrict__ rows) {
  const int f = blockIdx.x;
  long long a[3];
  depthprior::rows_partials<3, 4>(partial, tiles, f, a);
  if (threadIdx.x != 0) return;
  int64_t* o = rows + (int64_t)f * DEPTHACC_ROW;
  o[DEPTHACC_N_OWN] = a[0];
  o[DEPTHACC_N_CANDIDATES] = a[1];
  o[DEPTHACC_N_ADDED] = a[2];
  o[DEPTHACC_N_HIDDEN] = a[1] - a[2];
}

}  // namespace

void launch_depthacc_scatter(hipStream_t st, int n_frames, int height, int width, int n_views, int64_t wg0, int64_t n_wg,
                             const float* depth, const double* cams, const int32_t* nbr, unsigned long long* zbuf) {
  depthacc_scatter_kernel<<<(unsigned)n_wg, BLOCK, 0, st>>>(n_frames, height, width, n_views, wg0, depthacc_scatter_tiles(height, width),
                                                          depth, cams, nbr, zbuf);
}

void launch_depthacc_resolve(hipStream_t st, int height, int width, int64_t wg0, int64_t n_wg, const float* depth,
                             const unsigned long long* zbuf, int radius, double one_plus_tol, float* depth_out, uint8_t* origin,
                             int32_t* src, int32_t* partial) {
  depthacc_resolve_kernel<<<(unsigned)n_wg, BLOCK, 0, st>>>(height, width, wg0, (int)depthprior::tiles_x(width, TW), depthacc_tiles(height, width),
                                                          depth, zbuf, radius, one_plus_tol, depth_out, origin, src, partial);
}

void launch_depthacc_rows(hipStream_t st, int n_frames, int64_t tiles, const int32_t* partial, int64_t* rows) {
  depthacc_rows_kernel<<<n_frames, 64, 0, st>>>(tiles, partial, rows);
}

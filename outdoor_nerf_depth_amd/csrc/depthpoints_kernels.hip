// A sparse depth prior from a point cloud with tracks.  The geometry in float64 in the written order of
// tests/depth_points_reference.py, compiled with -ffp-contract=off.
//
//   scatter  `track`: grid (ceil(n_obs / 256)), 256 threads, one thread per row (point, frame) of obs.  Rows sorted by frame keep a
//            wave on one camera almost always: its 16 values are then one address per load, and the two counts of the wave go out
//            as one integer atomic add each (a wave that straddles two frames adds lane by lane).
//            `all`: grid (frames x point tiles), 256 threads: a workgroup takes 1024 consecutive points into one frame.  The camera
//            is a wave-uniform load (scalar registers), the points' 32 bytes are two 16-byte loads, all of a tile in flight
//            together; the count of the tile is summed over its four waves and added once.
//            Either way a point that projects is ONE global_atomic_umin_x2 on the 8-byte key (z bits, point index): a minimum over
//            integers, the same bits for every order of arrival.  The nearest point wins, the lower index among equal depths.
//   resolve  grid (frames x tiles), 256 threads: a tile of 32 x 8 pixels of one frame, one thread per pixel.  The depths of the tile
//            and its halo of occl_radius pixels go to LDS, every key read from memory once with every load in flight together; the
//            window minimum is two separable passes (along the rows, then down the columns).  The two counts of the tile are
//            ballots, added over the four waves in wave order.
//   rows     grid (frames), 64 threads: lane l adds the partials of tiles l, l + 64, ... and a shfl_down tree adds the lanes.  The
//            partials and the counters are integers, so every order gives the same bits.
#include "depthpoints_kernels.h"
#include "depth_prior_device.h"

namespace {

using depthprior::FX, depthprior::FY, depthprior::CX, depthprior::CY;
constexpr int BLOCK = DEPTHPOINTS_BLOCK, TW = DEPTHPOINTS_TILE_W, TH = DEPTHPOINTS_TILE_H, WAVES = BLOCK / 64, CAM = DEPTHPOINTS_CAM;
constexpr int PTILE = DEPTHPOINTS_POINT_TILE;
constexpr uint64_t EMPTY = depthprior::EMPTY_KEY;
using Window = depthprior::Window<TW, TH, DEPTHPOINTS_MAX_RADIUS, BLOCK>;   // the visibility window of the resolve (depth_prior_device.h)
constexpr int HALO_ROUNDS = Window::HALO_ROUNDS;

// Steps 1 - 6 of a point (wx, wy, wz) and a camera c: true iff the point projects into the frame, then t is its pixel and z32 its
// depth.  Every comparison is written so that a NaN fails it.
__device__ __forceinline__ bool project(const double* __restrict__ c, double wx, double wy, double wz, const DepthPointsRange& rg,
                                        int height, int width, int64_t& t, float& z32) {
  const auto [x, y, z] = depthprior::world_to_cam(c, {wx, wy, wz});   // step 1: P = R^T (Pw - t)
  if (!(z >= rg.near && z <= rg.far)) return false;            // step 2: near and far are finite, so z is
  const double u = c[FX] * x / z + c[CX], w = c[FY] * y / z + c[CY];   // step 3
  if (!(u >= 0.0 && u < (double)width && w >= 0.0 && w < (double)height)) return false;   // step 4: in float64, before any integer
  const int tx = (int)floor(u), ty = (int)floor(w);            // step 5: 0 .. width - 1, 0 .. height - 1
  z32 = (float)z;                                              // step 6: to nearest
  if (!(z32 > 0.f && z32 < __builtin_inff())) return false;    // (a near below float32's range, a far above it)
  t = (int64_t)ty * width + tx;
  return true;
}

__device__ __forceinline__ unsigned long long make_key(float z32, int64_t p) {
  return ((unsigned long long)__float_as_uint(z32) << 32) | (unsigned long long)(unsigned)p;   // step 7
}

__global__ __launch_bounds__(BLOCK) void depthpoints_scatter_obs_kernel(int n_frames, int height, int width, int64_t wg0,
                                                                       const double* __restrict__ cams, int64_t n_points,
                                                                       const double* __restrict__ points, int64_t n_obs,
                                                                       const int32_t* __restrict__ obs, DepthPointsRange rg,
                                                                       unsigned long long* __restrict__ zbuf,
                                                                       unsigned long long* __restrict__ counts) {
  const int lane = threadIdx.x & 63;
  const int64_t o = (wg0 + (int64_t)blockIdx.x) * BLOCK + threadIdx.x;
  int p = -1, f = -1;
  if (o < n_obs) {
    const int2 row = *reinterpret_cast<const int2*>(obs + o * DEPTHPOINTS_OBS);
    p = row.x;
    f = row.y;
  }
  const bool valid = p >= 0 && (int64_t)p < n_points && f >= 0 && f < n_frames;   // an index outside the tables is skipped: no read outside the buffers
  bool hit = false;
  if (valid) {
    const double2* pp = reinterpret_cast<const double2*>(points + (int64_t)p * DEPTHPOINTS_POINT);
    const double2 xy = pp[0], zc = pp[1];
    int64_t t;
    float z32;
    hit = project(cams + (int64_t)f * CAM, xy.x, xy.y, zc.x, rg, height, width, t, z32);
    if (hit) atomicMin(zbuf + (int64_t)f * height * width + t, make_key(z32, p));   // step 8
  }
  if (counts == nullptr) return;                               // (uniform)
  const unsigned long long m_valid = __ballot(valid), m_hit = __ballot(hit);
  if (m_valid == 0) return;                                    // (wave-uniform)
  const int leader = __ffsll((long long)m_valid) - 1;
  const int f0 = __shfl(f, leader, 64);
  if (__ballot(valid && f != f0) == 0) {                       // (wave-uniform) the wave is on one frame: one add per count
    if (lane == leader) {
      atomicAdd(counts + (int64_t)f0 * 2, (unsigned long long)__popcll(m_valid));
      if (m_hit != 0) atomicAdd(counts + (int64_t)f0 * 2 + 1, (unsigned long long)__popcll(m_hit));
    }
  } else if (valid) {
    atomicAdd(counts + (int64_t)f * 2, 1ull);
    if (hit) atomicAdd(counts + (int64_t)f * 2 + 1, 1ull);
  }
}

__global__ __launch_bounds__(BLOCK) void depthpoints_scatter_all_kernel(int height, int width, int64_t wg0, int64_t tiles,
                                                                       const double* __restrict__ cams, int64_t n_points,
                                                                       const double* __restrict__ points, DepthPointsRange rg,
                                                                       unsigned long long* __restrict__ zbuf,
                                                                       unsigned long long* __restrict__ counts) {
  __shared__ int red[WAVES][1];
  const int tid = threadIdx.x;
  const int64_t g = wg0 + (int64_t)blockIdx.x;
  const int64_t f = g / tiles, tile = g % tiles;
  const double* c = cams + f * CAM;                            // (uniform)
  unsigned long long* zf = zbuf + f * height * width;
  double2 xy[PTILE / BLOCK], zc[PTILE / BLOCK];                // every load of the tile is in flight before the first is looked at
#pragma unroll
  for (int k = 0; k < PTILE / BLOCK; ++k) {
    const int64_t p = tile * PTILE + k * BLOCK + tid;
    xy[k] = zc[k] = make_double2(__builtin_nan(""), __builtin_nan(""));
    if (p < n_points) {
      const double2* pp = reinterpret_cast<const double2*>(points + p * DEPTHPOINTS_POINT);
      xy[k] = pp[0];
      zc[k] = pp[1];
    }
  }
  int n_hit = 0;
#pragma unroll
  for (int k = 0; k < PTILE / BLOCK; ++k) {
    const int64_t p = tile * PTILE + k * BLOCK + tid;
    int64_t t;
    float z32;
    if (p < n_points && project(c, xy[k].x, xy[k].y, zc[k].x, rg, height, width, t, z32)) {
      atomicMin(zf + t, make_key(z32, p));                     // step 8
      ++n_hit;
    }
  }
  if (counts == nullptr) return;                               // (uniform)
  hipdev::wave_deposit(red, 0, hipdev::wave_sum_lane0(n_hit));
  __syncthreads();
  if (tid != 0) return;
  const int64_t left = n_points - tile * PTILE;
  atomicAdd(counts + f * 2, (unsigned long long)(left < PTILE ? left : PTILE));
  const int total = hipdev::waves_collect<int>(red, 0);
  if (total != 0) atomicAdd(counts + f * 2 + 1, (unsigned long long)total);
}

__global__ __launch_bounds__(BLOCK) void depthpoints_resolve_kernel(int height, int width, int64_t wg0, int tiles_x, int64_t tiles,
                                                                   const double* __restrict__ cams, const double* __restrict__ points,
                                                                   const unsigned long long* __restrict__ zbuf, int radius,
                                                                   double one_plus_tol, double std_scale, double std_floor,
                                                                   float* __restrict__ depth_out, float* __restrict__ std_out,
                                                                   int32_t* __restrict__ point, uint8_t* __restrict__ origin,
                                                                   int32_t* __restrict__ partial) {
  __shared__ float surf[Window::SURF];                       // depths of the tile and its halo, +inf where no point reached or outside the frame
  __shared__ float rowmin[Window::ROWMIN];                   // their minimum over the window's columns
  __shared__ int red[WAVES][2];
  const int tid = threadIdx.x, tx = tid % TW, ty = tid / TW;
  const int64_t g = wg0 + (int64_t)blockIdx.x;
  const int64_t f = g / tiles, tile = g % tiles;
  const int x0 = (int)(tile % tiles_x) * TW, y0 = (int)(tile / tiles_x) * TH;
  const int r = radius, hw = TW + 2 * r;
  const int64_t frame_px = (int64_t)height * width;
  const unsigned long long* zf = zbuf + f * frame_px;

  // The thread's own pixel and its share of the halo ring (cells tid, tid + 256, ...): every key is loaded before one is looked at.
  const int x = x0 + tx, y = y0 + ty;
  const bool inside = x < width && y < height;
  const int64_t t = (int64_t)y * width + x;
  int ht[HALO_ROUNDS], hc[HALO_ROUNDS];                      // a halo cell's index in the frame (-1: outside it) and in surf (-1: none)
  Window::halo_cells(tid, x0, y0, r, height, width, hc, ht);
  unsigned long long key = EMPTY, hk[HALO_ROUNDS];
  if (inside) key = zf[t];
#pragma unroll
  for (int k = 0; k < HALO_ROUNDS; ++k) {
    hk[k] = EMPTY;
    if (ht[k] >= 0) hk[k] = zf[ht[k]];
  }
  const bool cand = key != EMPTY;
  const float z = __uint_as_float((unsigned)(key >> 32));
  surf[(ty + r) * hw + tx + r] = cand ? z : __builtin_inff();
#pragma unroll
  for (int k = 0; k < HALO_ROUNDS; ++k)
    if (hc[k] >= 0) surf[hc[k]] = hk[k] != EMPTY ? __uint_as_float((unsigned)(hk[k] >> 32)) : __builtin_inff();
  const float zmin = Window::window_min(surf, rowmin, tid, r);
  const bool hidden = cand && (double)z > (double)zmin * one_plus_tol;
  const bool kept = cand && !hidden;
  if (inside) {
    const int64_t o = f * frame_px + t;
    const int32_t idx = (int32_t)(unsigned)key;              // below 2^31 wherever a point reached
    depth_out[o] = kept ? z : 0.f;
    if (std_out != nullptr) {
      float s32 = 0.f;
      if (kept) {
        const double zd = (double)z, coef = points[(int64_t)idx * DEPTHPOINTS_POINT + 3];
        const double s = std_scale * coef * zd * zd / cams[f * CAM + FX];
        s32 = (float)(s < std_floor ? std_floor : s);
      }
      std_out[o] = s32;
    }
    if (point != nullptr) point[o] = kept ? idx : -1;
    if (origin != nullptr)
      origin[o] = (uint8_t)(!cand ? DEPTHPOINTS_ORIGIN_NONE : kept ? DEPTHPOINTS_ORIGIN_POINT : DEPTHPOINTS_ORIGIN_HIDDEN);
  }
  if (partial == nullptr) return;                            // (uniform)
  hipdev::wave_deposit(red, 0, (int)__popcll(__ballot(kept)));
  hipdev::wave_deposit(red, 1, (int)__popcll(__ballot(hidden)));
  __syncthreads();
  if (tid < 2) partial[g * 2 + tid] = hipdev::waves_collect<int>(red, tid);
}

__global__ __launch_bounds__(64) void depthpoints_rows_kernel(int64_t tiles, const int32_t* __restrict__ partial,
                                                             const unsigned long long* __restrict__ counts, int64_t* __restrict__ rows) {
  const int f = blockIdx.x;
  long long a[2];
  depthprior::rows_partials<2, 2>(partial, tiles, f, a);
  if (threadIdx.x != 0) return;
  int64_t* o = rows + (int64_t)f * DEPTHPOINTS_ROW;
  o[DEPTHPOINTS_N_OBS] = (int64_t)counts[(int64_t)f * 2];
  o[DEPTHPOINTS_N_PROJECTED] = (int64_t)counts[(int64_t)f * 2 + 1];
  o[DEPTHPOINTS_N_KEPT] = a[0];
  o[DEPTHPOINTS_N_HIDDEN] = a[1];
}

}  // namespace

void launch_depthpoints_scatter_obs(hipStream_t st, int n_frames, int height, int width, int64_t wg0, int64_t n_wg, const double* cams,
                                    int64_t n_points, const double* points, int64_t n_obs, const int32_t* obs, DepthPointsRange rg,
                                    unsigned long long* zbuf, unsigned long long* counts) {
  depthpoints_scatter_obs_kernel<<<(unsigned)n_wg, BLOCK, 0, st>>>(n_frames, height, width, wg0, cams, n_points, points, n_obs, obs, rg,
                                                                 zbuf, counts);
}

void launch_depthpoints_scatter_all(hipStream_t st, int height, int width, int64_t wg0, int64_t n_wg, const double* cams,
                                    int64_t n_points, const double* points, DepthPointsRange rg, unsigned long long* zbuf,
                                    unsigned long long* counts) {
  depthpoints_scatter_all_kernel<<<(unsigned)n_wg, BLOCK, 0, st>>>(height, width, wg0, depthpoints_point_tiles(n_points), cams, n_points,
                                                                 points, rg, zbuf, counts);
}

void launch_depthpoints_resolve(hipStream_t st, int height, int width, int64_t wg0, int64_t n_wg, const double* cams,
                                const double* points, const unsigned long long* zbuf, int radius, double one_plus_tol,
                                double std_scale, double std_floor, float* depth_out, float* std_out, int32_t* point, uint8_t* origin,
                                int32_t* partial) {
  depthpoints_resolve_kernel<<<(unsigned)n_wg, BLOCK, 0, st>>>(height, width, wg0, (int)depthprior::tiles_x(width, TW),
                                                             depthpoints_tiles(height, width), cams, points, zbuf, radius, one_plus_tol,
                                                             std_scale, std_floor, depth_out, std_out, point, origin, partial);
}

void launch_depthpoints_rows(hipStream_t st, int n_frames, int64_t tiles, const int32_t* partial, const unsigned long long* counts,
                             int64_t* rows) {
  depthpoints_rows_kernel<<<n_frames, 64, 0, st>>>(tiles, partial, counts, rows);
}

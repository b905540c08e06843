// Multi-view consistency check of depth priors.  The geometry in float64 in the written order of
// tests/depth_consistency_reference.py, compiled with -ffp-contract=off; no atomics.
//
//   check  grid (tiles, frames), 256 threads: a workgroup is a tile of 32 x 8 pixels of one frame, one thread per pixel, a wave two
//          rows of 32, so the gathers of a tile in a neighbour fall into a patch of about the tile's size (a few cache lines per
//          row).  The neighbour list of the frame and the cameras of the frame and of its neighbours go to LDS once per workgroup;
//          in the loop over the neighbours they are wave-uniform LDS reads (broadcasts).  The pixel's outputs are written on the
//          way; the three counts of the tile (valid, verifiable, kept) are ballots, added over the four waves in wave order.
//   rows   grid (frames), 64 threads: lane l adds the partials of tiles l, l + 64, ... in that order and a shfl_down tree adds the
//          lanes.  The partials are integers, so every order gives the same bits.
#include "depthcons_kernels.h"
#include "depth_prior_device.h"

namespace {

using depthprior::P3, depthprior::pixel_to_world, depthprior::world_to_cam;   // the camera maths (depth_prior_device.h)
using depthprior::FX, depthprior::FY, depthprior::CX, depthprior::CY;
constexpr int BLOCK = DEPTHCONS_BLOCK, TW = DEPTHCONS_TILE_W, WAVES = BLOCK / 64, CAM = DEPTHCONS_CAM, KMAX = DEPTHCONS_MAX_VIEWS;

__global__ __launch_bounds__(BLOCK) void depthcons_check_kernel(int n_frames, int height, int width, int n_views, int frame0,
                                                               int64_t tile0, int tiles_x, int64_t tiles,
                                                               const float* __restrict__ depth, const double* __restrict__ cams,
                                                               const int32_t* __restrict__ nbr, DepthconsParams prm,
                                                               float* __restrict__ depth_out, float* __restrict__ std_out,
                                                               uint8_t* __restrict__ counts, int32_t* __restrict__ partial) {
  __shared__ double cam[KMAX + 1][CAM];                      // slot 0: the frame's own camera; slot k + 1: neighbour k's
  __shared__ int nb[KMAX];                                   // the neighbours, -1 = skipped
  __shared__ int red[WAVES][3];
  const int tid = threadIdx.x;
  const int f = frame0 + (int)blockIdx.y;
  const int64_t tile = tile0 + (int64_t)blockIdx.x;
  if (tid < KMAX) {
    const int j = tid < n_views ? nbr[(int64_t)f * n_views + tid] : -1;
    nb[tid] = (j >= 0 && j < n_frames) ? j : -1;             // an index outside the batch is skipped: no read outside the buffers
  }
  __syncthreads();
  for (int i = tid; i < (n_views + 1) * CAM; i += BLOCK) {
    const int slot = i / CAM, fr = slot == 0 ? f : nb[slot - 1];
    if (fr >= 0) cam[slot][i % CAM] = cams[(int64_t)fr * CAM + i % CAM];
  }
  __syncthreads();

  const int x = (int)(tile % tiles_x) * TW + (tid % TW);
  const int y = (int)(tile / tiles_x) * DEPTHCONS_TILE_H + tid / TW;
  const bool inside = x < width && y < height;
  const int64_t frame_px = (int64_t)height * width;
  const int64_t pix = (int64_t)f * frame_px + (int64_t)y * width + x;
  const float d32 = inside ? depth[pix] : 0.f;
  const bool valid = d32 > 0.f;                              // 0, negatives and NaN are invalid
  const double d = (double)d32;
  int n_seen = 0, n_ok = 0;
  double s = 0.0;
  if (valid) {
    const double px = (double)x + 0.5, py = (double)y + 0.5;
    const double* c0 = cam[0];
    const P3 pw = pixel_to_world(c0, px, py, d);
    const double tol_d = prm.rel_tol * d;
    for (int k = 0; k < n_views; ++k) {
      const int j = nb[k];
      if (j < 0) continue;
      const double* cj = cam[k + 1];
      const P3 pj = world_to_cam(cj, pw);
      if (pj.z <= 0.0) continue;
      const double u = cj[FX] * (pj.x / pj.z) + cj[CX], v = cj[FY] * (pj.y / pj.z) + cj[CY];
      const double xi = floor(u), yi = floor(v);
      if (!(xi >= 0.0 && xi < (double)width && yi >= 0.0 && yi < (double)height)) continue;   // a NaN is outside
      const float dj32 = depth[(int64_t)j * frame_px + (int64_t)(int)yi * width + (int)xi];
      if (!(dj32 > 0.f)) continue;
      ++n_seen;
      const P3 qw = pixel_to_world(cj, xi + 0.5, yi + 0.5, (double)dj32);
      const P3 qi = world_to_cam(c0, qw);
      if (qi.z <= 0.0) continue;
      const double u2 = c0[FX] * (qi.x / qi.z) + c0[CX], v2 = c0[FY] * (qi.y / qi.z) + c0[CY];
      const double du = u2 - px, dv = v2 - py;
      const double e_pix2 = du * du + dv * dv, e = qi.z - d;
      if (e_pix2 <= prm.pix_tol2 && fabs(e) <= tol_d) {      // a NaN is not ok
        ++n_ok;
        s += e * e;
      }
    }
  }
  const bool verifiable = n_seen >= prm.min_views;
  const bool keep = verifiable ? n_ok >= prm.min_views : prm.keep_unverified != 0;
  if (inside) {
    depth_out[pix] = (valid && !keep) ? 0.f : d32;           // an invalid input keeps its bits
    if (std_out != nullptr) {
      float sd = 0.f;
      if (valid && keep) {
        const double spread = n_ok > 0 ? sqrt(s / (double)n_ok) : prm.rel_tol * d;
        sd = (float)(spread < prm.std_floor ? prm.std_floor : spread);
      }
      std_out[pix] = sd;
    }
    if (counts != nullptr) {
      counts[2 * pix] = (uint8_t)n_seen;
      counts[2 * pix + 1] = (uint8_t)n_ok;
    }
  }
  if (partial == nullptr) return;                            // (uniform)
  hipdev::wave_deposit(red, 0, (int)__popcll(__ballot(valid)));
  hipdev::wave_deposit(red, 1, (int)__popcll(__ballot(valid && verifiable)));
  hipdev::wave_deposit(red, 2, (int)__popcll(__ballot(valid && keep)));
  __syncthreads();
  if (tid < 4) partial[((int64_t)f * tiles + tile) * 4 + tid] = tid < 3 ? hipdev::waves_collect<int>(red, tid) : 0;
}

__global__ __launch_bounds__(64) void depthcons_rows_kernel(int64_t tiles, const int32_t* __restrict__ partial,
                                                           int64_t* __restrict__ rows) {
  const int f = blockIdx.x;
  long long a[3];
  depthprior::rows_partials<3, 4>(partial, tiles, f, a);
  if (threadIdx.x != 0) return;
  int64_t* o = rows + (int64_t)f * DEPTHCONS_ROW;
  o[DEPTHCONS_N_VALID] = a[0];
  o[DEPTHCONS_N_VERIFIABLE] = a[1];
  o[DEPTHCONS_N_KEPT] = a[2];
  o[DEPTHCONS_N_DROPPED] = a[0] - a[2];
}

}  // namespace

void launch_depthcons_check(hipStream_t st, int n_frames, int height, int width, int n_views, int frame0, int n_launch_frames,
                            int64_t tile0, int64_t n_tiles, const float* depth, const double* cams, const int32_t* nbr,
                            DepthconsParams prm, float* depth_out, float* std_out, uint8_t* counts, int32_t* partial) {
  depthcons_check_kernel<<<dim3((unsigned)n_tiles, (unsigned)n_launch_frames), BLOCK, 0, st>>>(
      n_frames, height, width, n_views, frame0, tile0, (int)depthprior::tiles_x(width, TW), depthcons_tiles(height, width), depth, cams, nbr,
      prm, depth_out, std_out, counts, partial);
}

void launch_depthcons_rows(hipStream_t st, int n_frames, int64_t tiles, const int32_t* partial, int64_t* rows) {
  depthcons_rows_kernel<<<n_frames, 64, 0, st>>>(tiles, partial, rows);
}

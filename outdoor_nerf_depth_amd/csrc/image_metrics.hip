// SSIM (scikit-image structural_similarity, defaults: uniform 7 x 7 window, sample covariance, K1 = 0.01, K2 = 0.03,
// data_range = 255) and 8-bit PSNR of uint8 [F, H, W, 3] image pairs: nerfpp_image_metrics_u8 (include/nerfpp_hip.h).
//
// The inputs are bytes, so the five window sums (x, y, x^2, y^2, xy over 49 pixels) are exact int32 values; S is evaluated
// per window in float64 from those integers, in the order scikit-image writes the expression.  Nothing here is an atomic:
// every workgroup writes its own partials, and a second kernel adds them in index order, so a frame's two values depend on
// that frame's bytes alone -- not on the batch around it and not on which workgroup finished first.
//
// image_metrics_tile_kernel: one workgroup = one TH x TW tile of window positions of one frame, all three channels.
//   1. stage the (TH + 6) x (TW + 6) pixel region of both images in LDS, row by row: whole dwords where the row's global
//      address allows, single bytes for the head and the tail of a row (W * 3 is not a multiple of 4 for every width, so the
//      phase changes from row to row).  A staged row keeps the phase (address & 3) of its global row, which is what lets
//      an aligned global dword land on an aligned LDS dword.  Nothing outside [row start, row end) is ever read.
//   2. per channel: horizontal 7-sums of the five quantities into LDS, then vertical 7-sums, S in float64, wave-shuffle
//      reduction and the four waves in wave order (hipdev::wave_deposit / waves_collect), one float64 partial per (frame, channel, tile).
//   3. the exact integer sum of (x - y)^2 over the pixels the tile owns (its TH x TW corner; the last tile row / column
//      also owns the 6-pixel rim), one uint64 per (frame, tile).
// image_metrics_finish_kernel: one workgroup per frame; adds the partials in tile order and writes (ssim, psnr8).
#include <math.h>
#include "hip_device.h"
#include "nerfpp_kernels.h"

namespace {

constexpr int WIN = 7, HALO = WIN - 1;
constexpr int TH = 16, TW = 32;                   // window positions per tile
constexpr int RH = TH + HALO, RW = TW + HALO;     // staged pixels per tile
constexpr int ROW_DW = 32;                        // dwords per staged row: <= 3 phase bytes + RW * 3 = 114 pixel bytes
constexpr int ROW_B = ROW_DW * 4;
constexpr int THREADS = 256, WAVES = THREADS / 64;
static_assert(3 + RW * 3 <= ROW_B, "a staged row holds the phase bytes and the pixels");
static_assert(TH * TW == 2 * THREADS, "two window positions per thread and channel");
static_assert((long long)RH * RW * 3 * 255 * 255 < (1ll << 32), "a tile's squared error fits uint32");

// rows [0, nrows) x bytes [0, nbytes) of the image region starting at `src` (row pitch `pitch` bytes) -> lds[r][phase_r + b]
__device__ __forceinline__ void stage_rows(const unsigned char* __restrict__ src, size_t pitch, int nrows, int nbytes,
                                           uint32_t* lds) {
  for (int item = threadIdx.x; item < nrows * ROW_DW; item += THREADS) {
    const int r = item / ROW_DW, k = item % ROW_DW;
    const unsigned char* p = src + (size_t)r * pitch;
    const int ph = (int)((uintptr_t)p & 3);
    const int b0 = 4 * k - ph;                    // row-relative byte of this dword's first byte
    if (b0 >= nbytes) continue;
    if (b0 >= 0 && b0 + 4 <= nbytes) {
      lds[item] = *reinterpret_cast<const uint32_t*>(p + b0);        // (p + b0) & 3 == 0
    } else {                                      // head or tail of the row: only the bytes that belong to it
      unsigned char* l = reinterpret_cast<unsigned char*>(lds + item);
      for (int q = 0; q < 4; ++q)
        if (b0 + q >= 0 && b0 + q < nbytes) l[q] = p[b0 + q];
    }
  }
}

using hipdev::wave_sum_lane0, hipdev::wave_deposit, hipdev::waves_collect;

__global__ __launch_bounds__(THREADS) void image_metrics_tile_kernel(int H, int W, const unsigned char* __restrict__ gt,
                                                                     const unsigned char* __restrict__ pred,
                                                                     double* __restrict__ part_s,
                                                                     unsigned long long* __restrict__ part_e) {
  __shared__ uint32_t sx[RH * ROW_DW], sy[RH * ROW_DW];
  __shared__ int hs[5][RH][TW];
  __shared__ double red_s[WAVES][1];
  __shared__ uint32_t red_e[WAVES][1];

  const int tid = threadIdx.x;
  const int f = blockIdx.z, x0 = blockIdx.x * TW, y0 = blockIdx.y * TH;
  const int ntiles = gridDim.x * gridDim.y, tile = blockIdx.y * gridDim.x + blockIdx.x;
  const int nrows = min(RH, H - y0), ncols = min(RW, W - x0);         // staged pixels that exist
  const int vi = min(TH, H - HALO - y0), vj = min(TW, W - HALO - x0); // window positions that exist (>= 1 by the grid)
  const size_t pitch = (size_t)W * 3;
  const size_t org = ((size_t)f * H + y0) * pitch + (size_t)x0 * 3;
  const unsigned char* gx = gt + org;
  const unsigned char* gy = pred + org;
  stage_rows(gx, pitch, nrows, ncols * 3, sx);
  stage_rows(gy, pitch, nrows, ncols * 3, sy);
  __syncthreads();
  const unsigned char* bx = reinterpret_cast<const unsigned char*>(sx);
  const unsigned char* by = reinterpret_cast<const unsigned char*>(sy);
  const uint32_t ax = (uint32_t)(uintptr_t)gx, ay = (uint32_t)(uintptr_t)gy, pl = (uint32_t)pitch;
  // byte 0 of staged row r sits at r * ROW_B + phase of its global row
  auto rowx = [&](int r) { return bx + r * ROW_B + ((ax + (uint32_t)r * pl) & 3u); };
  auto rowy = [&](int r) { return by + r * ROW_B + ((ay + (uint32_t)r * pl) & 3u); };

  // ---- squared error over the pixels this tile owns
  {
    const int own_r = blockIdx.y == gridDim.y - 1 ? nrows : TH;
    const int own_b = (blockIdx.x == gridDim.x - 1 ? ncols : TW) * 3;
    uint32_t e = 0;
    for (int item = tid; item < own_r * own_b; item += THREADS) {
      const int r = item / own_b, b = item % own_b;
      const int d = (int)rowx(r)[b] - (int)rowy(r)[b];
      e += (uint32_t)(d * d);
    }
    wave_deposit(red_e, 0, wave_sum_lane0(e));
  }

  const double C1 = (0.01 * 255.0) * (0.01 * 255.0), C2 = (0.03 * 255.0) * (0.03 * 255.0);
  const double NP = 49.0, cov_norm = NP / (NP - 1.0);
  for (int ch = 0; ch < 3; ++ch) {
    // ---- horizontal 7-sums
    for (int item = tid; item < nrows * TW; item += THREADS) {
      const int r = item / TW, j = item % TW;
      if (j >= vj) continue;
      const unsigned char* px = rowx(r) + j * 3 + ch;
      const unsigned char* py = rowy(r) + j * 3 + ch;
      int a = 0, b = 0, aa = 0, bb = 0, ab = 0;
#pragma unroll
      for (int k = 0; k < WIN; ++k) {
        const int x = px[3 * k], y = py[3 * k];
        a += x; b += y; aa += x * x; bb += y * y; ab += x * y;
      }
      hs[0][r][j] = a; hs[1][r][j] = b; hs[2][r][j] = aa; hs[3][r][j] = bb; hs[4][r][j] = ab;
    }
    __syncthreads();
    // ---- vertical 7-sums, S in float64
    double acc = 0.0;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int o = tid + h * THREADS, i = o / TW, j = o % TW;
      if (i < vi && j < vj) {
        int s[5] = {0, 0, 0, 0, 0};
#pragma unroll
        for (int k = 0; k < WIN; ++k)
#pragma unroll
          for (int q = 0; q < 5; ++q) s[q] += hs[q][i + k][j];
        const double ux = (double)s[0] / NP, uy = (double)s[1] / NP;
        const double uxx = (double)s[2] / NP, uyy = (double)s[3] / NP, uxy = (double)s[4] / NP;
        const double vx = cov_norm * (uxx - ux * ux), vy = cov_norm * (uyy - uy * uy), vxy = cov_norm * (uxy - ux * uy);
        const double A1 = 2.0 * ux * uy + C1, A2 = 2.0 * vxy + C2;
        const double B1 = ux * ux + uy * uy + C1, B2 = vx + vy + C2;
        acc += (A1 * A2) / (B1 * B2);
      }
    }
    wave_deposit(red_s, 0, wave_sum_lane0(acc));
    __syncthreads();                              // also: every read of hs is done before the next channel overwrites it
    if (tid == 0) {
      part_s[((size_t)f * 3 + ch) * ntiles + tile] = waves_collect<double>(red_s, 0);
      if (ch == 0) part_e[(size_t)f * ntiles + tile] = waves_collect<unsigned long long>(red_e, 0);
    }
    __syncthreads();                              // red_s is free again
  }
}

__global__ __launch_bounds__(64) void image_metrics_finish_kernel(int ntiles, double n_windows, double n_values,
                                                                  const double* __restrict__ part_s,
                                                                  const unsigned long long* __restrict__ part_e,
                                                                  double* __restrict__ out) {
  __shared__ double ch_mean[3];
  __shared__ unsigned long long err;
  const int f = blockIdx.x, t = threadIdx.x;
  if (t < 3) {
    const double* p = part_s + ((size_t)f * 3 + t) * ntiles;
    double s = 0.0;
    for (int k = 0; k < ntiles; ++k) s += p[k];
    ch_mean[t] = s / n_windows;
  } else if (t == 3) {
    const unsigned long long* p = part_e + (size_t)f * ntiles;
    unsigned long long s = 0;
    for (int k = 0; k < ntiles; ++k) s += p[k];
    err = s;
  }
  __syncthreads();
  if (t == 0) {
    out[2 * f] = (ch_mean[0] + ch_mean[1] + ch_mean[2]) / 3.0;
    out[2 * f + 1] = err == 0 ? (double)INFINITY : 10.0 * log10((255.0 * 255.0) / ((double)err / n_values));
  }
}

}  // namespace

int64_t image_metrics_tiles(int H, int W) {
  return (int64_t)((H - HALO + TH - 1) / TH) * ((W - HALO + TW - 1) / TW);
}

void launch_image_metrics(hipStream_t st, int F, int H, int W, const unsigned char* gt, const unsigned char* pred,
                          void* workspace, double* out) {
  const int ty = (H - HALO + TH - 1) / TH, tx = (W - HALO + TW - 1) / TW;
  const int ntiles = tx * ty;
  double* part_s = (double*)workspace;
  unsigned long long* part_e = (unsigned long long*)(part_s + (size_t)F * 3 * ntiles);
  image_metrics_tile_kernel<<<dim3(tx, ty, F), THREADS, 0, st>>>(H, W, gt, pred, part_s, part_e);
  image_metrics_finish_kernel<<<F, 64, 0, st>>>(ntiles, (double)(H - HALO) * (double)(W - HALO), (double)H * (double)W * 3.0,
                                               part_s, part_e, out);
}

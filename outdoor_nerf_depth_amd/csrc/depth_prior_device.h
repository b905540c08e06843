// What the six depth-prior libraries (depthcons, depthacc, depthalign, depthcomp, depthmvs, depthpoints: DESIGN.md 8.13) share on
// the device and at their launches: the tiling of a frame, the 16-value camera, the visibility window of the two z-buffer
// resolves and the rows sum.  Header-only, like hip_device.h; every device function is __forceinline__, so a kernel that calls one
// holds the instructions it held when the lines stood in its own file.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "hip_device.h"

namespace depthprior {

// ---------------------------------------------------------------------------------------------------------------------
// Tiles and launches
constexpr int64_t MAX_GRID = 1ll << 22;                      // workgroups of one launch (2^30 threads)
constexpr uint64_t EMPTY_KEY = ~0ull;                        // the z-buffer key of a pixel nothing reached

inline int64_t tiles_x(int width, int TW) { return (width + TW - 1) / TW; }
inline int64_t tiles(int height, int width, int TW, int TH) { return tiles_x(width, TW) * ((height + TH - 1) / TH); }

// ---------------------------------------------------------------------------------------------------------------------
// A camera's 16 values: fx fy cx cy | R00 R01 R02 t0 | R10 R11 R12 t1 | R20 R21 R22 t2 (camera-to-world, OpenCV axes).  Float64
// in the written order of the numpy restatements; the files that use these are compiled with -ffp-contract=off.  How a camera is
// read (LDS, wave-uniform global loads), how a pixel is formed from the camera point and which depths are refused differ between
// the libraries and stay at their call sites.
constexpr int FX = 0, FY = 1, CX = 2, CY = 3;

struct P3 {
  double x, y, z;
};

// pixel (px, py) at z-depth d of camera c -> world: Pc = ((px - cx) / fx * d, (py - cy) / fy * d, d), Pw = R Pc + t
__device__ __forceinline__ P3 pixel_to_world(const double* c, double px, double py, double d) {
  const double xc = (px - c[CX]) / c[FX] * d, yc = (py - c[CY]) / c[FY] * d;
  P3 w;
  w.x = ((c[4] * xc + c[5] * yc) + c[6] * d) + c[7];
  w.y = ((c[8] * xc + c[9] * yc) + c[10] * d) + c[11];
  w.z = ((c[12] * xc + c[13] * yc) + c[14] * d) + c[15];
  return w;
}

// world -> camera c: R^T (Pw - t)
__device__ __forceinline__ P3 world_to_cam(const double* c, P3 w) {
  const double dx = w.x - c[7], dy = w.y - c[11], dz = w.z - c[15];
  P3 p;
  p.x = (c[4] * dx + c[8] * dy) + c[12] * dz;
  p.y = (c[5] * dx + c[9] * dy) + c[13] * dz;
  p.z = (c[6] * dx + c[10] * dy) + c[14] * dz;
  return p;
}

// ---------------------------------------------------------------------------------------------------------------------
// The visibility window of a z-buffer resolve: a workgroup of BLOCK = TW x TH threads is a tile of one frame, one thread per pixel;
// `surf` holds the surface values of the tile and its halo of r <= RMAX pixels, row-major with rows of TW + 2 r, +inf where there
// is no surface or no frame.  The caller loads what its surface is made of and stores it to surf; the rest is here.
template <int TW, int TH, int RMAX, int BLOCK>
struct Window {
  static_assert(BLOCK == TW * TH, "one thread per pixel of the tile");
  static constexpr int SURF = (TH + 2 * RMAX) * (TW + 2 * RMAX), ROWMIN = (TH + 2 * RMAX) * TW;
  static constexpr int HALO_ROUNDS = (SURF + BLOCK - 1) / BLOCK;   // rounds of BLOCK cells that cover a tile with the widest halo

  // The thread's share of the halo ring of the tile at (x0, y0): cells tid, tid + BLOCK, ...  hc[k]: the cell's index in surf (-1:
  // none, the cell is past the end or one of the tile's own); ht[k]: its pixel's index in the frame (-1: none, or outside the frame)
  static __device__ __forceinline__ void halo_cells(int tid, int x0, int y0, int r, int height, int width, int (&hc)[HALO_ROUNDS],
                                                    int (&ht)[HALO_ROUNDS]) {
    const int hw = TW + 2 * r, hh = TH + 2 * r;
    const int cells = hh * hw;
    const unsigned inv_hw = ((1u << 20) + hw - 1) / hw;      // c / hw == (c * inv_hw) >> 20 for c < 1280 and hw = 32, 34, .. 48
    static_assert(HALO_ROUNDS * BLOCK <= 1280 && TW == 32 && RMAX <= 8, "the range the reciprocal was checked on");
#pragma unroll
    for (int k = 0; k < HALO_ROUNDS; ++k) {
      ht[k] = hc[k] = -1;
      if (k * BLOCK >= cells) continue;                      // (uniform) a radius of 2 takes two of the five rounds
      const int c = tid + k * BLOCK, hy = (int)(((unsigned)c * inv_hw) >> 20), hx = c - hy * hw;
      const int gy = y0 + hy - r, gx = x0 + hx - r;
      if (c < cells && !(hy >= r && hy < r + TH && hx >= r && hx < r + TW)) {
        hc[k] = c;
        if (gy >= 0 && gy < height && gx >= 0 && gx < width) ht[k] = gy * width + gx;
      }
    }
  }

  // The minimum of surf over the (2 r + 1)^2 window of the thread's pixel, as two separable passes (along the rows into rowmin,
  // then down the columns).  Every thread of the workgroup calls it after its stores to surf: the barriers are in here.
  static __device__ __forceinline__ float window_min(const float (&surf)[SURF], float (&rowmin)[ROWMIN], int tid, int r) {
    const int tx = tid % TW, ty = tid / TW, hw = TW + 2 * r, hh = TH + 2 * r;
    __syncthreads();
    for (int c = tid; c < hh * TW; c += BLOCK) {
      const int hy = c / TW, cx = c % TW;
      const float* row = surf + hy * hw + cx;
      float m = row[0];
      for (int k = 1; k <= 2 * r; ++k) m = row[k] < m ? row[k] : m;
      rowmin[c] = m;
    }
    __syncthreads();
    float zmin = rowmin[ty * TW + tx];
    for (int k = 1; k <= 2 * r; ++k) {
      const float m = rowmin[(ty + k) * TW + tx];
      zmin = m < zmin ? m : zmin;
    }
    return zmin;
  }
};

// ---------------------------------------------------------------------------------------------------------------------
// The rows sum: one wave per frame f.  Lane l adds columns 0 .. K - 1 of the partials of tiles l, l + 64, ... (partial is
// [frames, tiles, STRIDE] int32) and a shfl_down tree adds the lanes: out[k] is the frame's sum in LANE 0.  The partials are
// integers, so every order gives the same bits.
template <int K, int STRIDE>
__device__ __forceinline__ void rows_partials(const int32_t* __restrict__ partial, int64_t tiles, int f, long long (&out)[K]) {
  const int lane = threadIdx.x;
  const int32_t* fp = partial + (int64_t)f * tiles * STRIDE;
  long long a[K] = {};
  for (int64_t t = lane; t < tiles; t += 64) {
#pragma unroll
    for (int k = 0; k < K; ++k) a[k] += fp[t * STRIDE + k];
  }
#pragma unroll
  for (int k = 0; k < K; ++k) out[k] = hipdev::wave_sum_lane0(a[k]);
}

}  // namespace depthprior

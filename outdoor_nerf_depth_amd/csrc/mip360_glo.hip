// Per-image appearance embeddings (GLO) of the NerfMLP's view branch (internal/models.py:64-65, 101-110, 228, 566-573):
// one learned float32 vector of G <= 4 features per training image, appended to [bottleneck (256) | pos_enc(viewdirs) (27)]
// -- columns 283 .. 283+G-1 of the view layer's 288-column input row, columns 27 .. 27+G-1 of the per-ray direction table
// mip360_view_branch_fm reads.  Column 287 / 31 stays the zero K padding.
//
//   dir_glo_encode_kernel : mip360_dir_encode's arithmetic (same expressions, same -ffp-contract=off) + the gathered embedding.
//   glo_partial_kernel    : stage 1 of the embedding gradient.  One wave per ray: the ray's S rows of d_hz (128 bf16 = 256
//       bytes each) are read 16 bytes per lane (16 lanes per row, 4 rows per wave-wide load, up to 8 loads in flight per
//       lane), multiplied with the G weight rows W_view[283+g, 0:128] a lane keeps in registers (its 8 columns), summed in
//       float32 per lane in sample order and then over the wave by a fixed xor butterfly -> partial[ray][0..3].
//   glo_reduce_kernel     : stage 2.  One 256-thread workgroup per embedding row e: thread t adds, in ray order, the partials
//       of rays t, t + 256, ... whose camera is e; the 64 lanes of a wave are summed by the same butterfly and the four waves
//       in wave order.  Every row of g_embed is written (0 when no ray belongs to it); no atomics anywhere: the summation
//       tree depends on the shapes alone, so equal inputs give equal bits.
#include <math.h>
#include "mip360_device.h"
#include "mip360_launch.h"

namespace mip360 {

constexpr int GLO_COL0 = 27, GLO_MAX = 4, VIEW_W = 128;

__global__ void dir_glo_encode_kernel(int n, int S, const float* __restrict__ viewdirs, const float* __restrict__ embed, int E,
                                      int G, const int32_t* __restrict__ cam_idx, int cam_stride, __bf16* __restrict__ out,
                                      int ld, int col0, int width) {
  const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t row = idx / width;
  const int c = (int)(idx - row * width);
  if (row >= (int64_t)n * S) return;
  const int ray = (int)(row / S);
  float v = 0.f;
  if (c < 3) v = viewdirs[ray * 3 + c];
  else if (c < GLO_COL0) {
    // four_feat = sin(concat([scaled_x, scaled_x + pi/2])): scaled_x index = k*3 + d  (as dir_encode_kernel)
    const int q = c - 3, half = q / 12, r = q - half * 12, k = r / 3, d = r - k * 3;
    const float sx = viewdirs[ray * 3 + d] * (float)(1 << k);
    v = sinf(half ? sx + 1.5707963267948966f : sx);
  } else if (cam_idx && c < GLO_COL0 + G) {
    const int e = cam_idx[(size_t)ray * cam_stride];
    if ((unsigned)e < (unsigned)E) v = embed[(size_t)e * G + (c - GLO_COL0)];      // an index outside [0, E) reads nothing: zeros
  }
  out[(size_t)row * ld + col0 + c] = (__bf16)v;
}

__device__ __forceinline__ float bf16_lo(uint32_t u) { return __uint_as_float(u << 16); }
__device__ __forceinline__ float bf16_hi(uint32_t u) { return __uint_as_float(u & 0xffff0000u); }

using mip360dev::wave_sum;

// partial [n_rays, 4]: columns G..3 are written as zero
__global__ __launch_bounds__(256) void glo_partial_kernel(int n_rays, int S, int G, const __bf16* __restrict__ d_hz, int ld_dhz,
                                                          const __bf16* __restrict__ wb_view, int ld_wb, int row0,
                                                          float* __restrict__ partial) {
  const int lane = threadIdx.x & 63;
  const int ray = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (ray >= n_rays) return;                                        // (whole waves leave: no shuffle below is divergent)
  const int sub = lane >> 4, c8 = (lane & 15) * 8;
  float w[GLO_MAX][8];
#pragma unroll
  for (int g = 0; g < GLO_MAX; ++g) {
    uint4 u = make_uint4(0u, 0u, 0u, 0u);
    if (g < G) u = *reinterpret_cast<const uint4*>(wb_view + (size_t)(row0 + g) * ld_wb + c8);
    w[g][0] = bf16_lo(u.x); w[g][1] = bf16_hi(u.x); w[g][2] = bf16_lo(u.y); w[g][3] = bf16_hi(u.y);
    w[g][4] = bf16_lo(u.z); w[g][5] = bf16_hi(u.z); w[g][6] = bf16_lo(u.w); w[g][7] = bf16_hi(u.w);
  }
  float acc[GLO_MAX] = {0.f, 0.f, 0.f, 0.f};
  const __bf16* base = d_hz + (size_t)ray * S * ld_dhz + c8;
  for (int s0 = 0; s0 < S; s0 += 32) {
    uint4 v[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const int s = s0 + i * 4 + sub;
      v[i] = s < S ? *reinterpret_cast<const uint4*>(base + (size_t)s * ld_dhz) : make_uint4(0u, 0u, 0u, 0u);
    }
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const float x[8] = {bf16_lo(v[i].x), bf16_hi(v[i].x), bf16_lo(v[i].y), bf16_hi(v[i].y),
                          bf16_lo(v[i].z), bf16_hi(v[i].z), bf16_lo(v[i].w), bf16_hi(v[i].w)};
#pragma unroll
      for (int g = 0; g < GLO_MAX; ++g)
#pragma unroll
        for (int j = 0; j < 8; ++j) acc[g] = fmaf(x[j], w[g][j], acc[g]);
    }
  }
#pragma unroll
  for (int g = 0; g < GLO_MAX; ++g) acc[g] = wave_sum(acc[g]);
  if (lane == 0) *reinterpret_cast<float4*>(partial + (size_t)ray * 4) = make_float4(acc[0], acc[1], acc[2], acc[3]);
}

__global__ __launch_bounds__(256) void glo_reduce_kernel(int n_rays, int G, const int32_t* __restrict__ cam_idx, int cam_stride,
                                                         const float* __restrict__ partial, float* __restrict__ g_embed) {
  __shared__ float4 sh[4];
  const int e = blockIdx.x;
  float4 a = make_float4(0.f, 0.f, 0.f, 0.f);
  for (int r0 = 0; r0 < n_rays; r0 += 4 * 256) {
    int cam[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int r = r0 + i * 256 + (int)threadIdx.x;
      cam[i] = r < n_rays ? cam_idx[(size_t)r * cam_stride] : -1;
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      if (cam[i] == e) {
        const float4 p = *reinterpret_cast<const float4*>(partial + (size_t)(r0 + i * 256 + (int)threadIdx.x) * 4);
        a.x += p.x; a.y += p.y; a.z += p.z; a.w += p.w;
      }
    }
  }
  a.x = wave_sum(a.x); a.y = wave_sum(a.y); a.z = wave_sum(a.z); a.w = wave_sum(a.w);
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = a;
  __syncthreads();
  if ((int)threadIdx.x < G) {
    const int g = threadIdx.x;
    float s = 0.f;
#pragma unroll
    for (int wv = 0; wv < 4; ++wv) s += g == 0 ? sh[wv].x : g == 1 ? sh[wv].y : g == 2 ? sh[wv].z : sh[wv].w;
    g_embed[(size_t)e * G + g] = s;
  }
}

}  // namespace mip360

using namespace mip360;

void mip360_launch_dir_glo_encode(hipStream_t st, int n, int S, const float* viewdirs, const float* embed, int E, int G,
                                  const int32_t* cam_idx, int cam_stride, void* out, int ld, int col0, int width) {
  const int64_t tot = (int64_t)n * S * width;
  hipLaunchKernelGGL(dir_glo_encode_kernel, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, st, n, S, viewdirs, embed, E, G, cam_idx,
                     cam_stride, (__bf16*)out, ld, col0, width);
}

void mip360_launch_glo_backward(hipStream_t st, int n_rays, int S, int G, int E, const void* d_hz, int ld_dhz, const void* wb_view,
                                int ld_wb, int row0, const int32_t* cam_idx, int cam_stride, float* partial, float* g_embed) {
  hipLaunchKernelGGL(glo_partial_kernel, dim3((unsigned)((n_rays + 3) / 4)), dim3(256), 0, st, n_rays, S, G, (const __bf16*)d_hz, ld_dhz,
                     (const __bf16*)wb_view, ld_wb, row0, partial);
  hipLaunchKernelGGL(glo_reduce_kernel, dim3((unsigned)E), dim3(256), 0, st, n_rays, G, cam_idx, cam_stride, partial, g_embed);
}

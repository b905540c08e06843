// 3 x 3 convolution + bias + ReLU of NHWC float32 maps as an implicit GEMM on v_mfma_f32_32x32x2_f32 (lpips_hip.h).
//
//   M = every pixel of every image of the call (m = (img * H + y) * W + x), N = Cout, K = 9 * Cin with k = tap * Cin + c.
// A (the im2col matrix) is never materialised: a chunk of 16 k rows of a 128-pixel tile is gathered from the input map into
// LDS, zero where the tap falls outside the image.  When Cin is a multiple of 16 a chunk is 16 consecutive channels of ONE
// tap, so every pixel contributes one 64-byte run (four float4 loads); the first layer (Cin = 3, K = 27 padded to 32) takes
// the scalar gather.  B is the packed weight [Kp, Cout] (lpips_pack_conv), staged 16 rows at a time.
//
// Workgroup: 256 threads = 2 x 2 waves, tile 128 pixels x BN outputs (BN = 128, or 64 for Cout = 64); a wave owns
// 64 x BN/2 = 2 x BN/64 MFMA tiles of 32 x 32.  The next chunk's global loads are issued before the current chunk's MFMAs.
// float32 operands and accumulation: each output is one k-ordered fma chain (exact float32 products, one rounding per
// step), the same chain for a pixel wherever its tile falls, so a map does not depend on the batch around it.
//
// Bounds: rows m >= M load zeros and store nothing; taps outside the image load zeros; k >= 9 * Cin (scalar gather) loads
// zeros and multiplies zero weight rows; Cout is a multiple of BN and Kp of 16 (checked by the callers in lpips_api.hip).
#include "hip_device.h"
#include "lpips_kernels.h"

namespace {

using hipdev::f32x16;

constexpr int BM = 128, KC = LPIPS_KC, LDA = BM + 4, THREADS = 256;

template <int BN, bool VEC>
__global__ __launch_bounds__(THREADS) void lpips_conv3x3_kernel(int M, int H, int W, int Cin, int Cout, int Kp,
                                                                const float* __restrict__ x, const float* __restrict__ wp,
                                                                const float* __restrict__ bias, float* __restrict__ y) {
  constexpr int NT = BN / 64;                     // 32-wide n tiles per wave
  constexpr int NA = VEC ? 2 : 8;                 // A items per thread and chunk: float4 (VEC) or scalars
  __shared__ float As[KC * LDA];
  __shared__ __attribute__((aligned(16))) float Bs[KC * BN];

  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int m0 = blockIdx.x * BM, n0 = blockIdx.y * BN;
  const int HW = H * W, K = 9 * Cin;

  // ---- the pixels this thread gathers for: VEC item = tid + r * 256 -> (pixel item >> 2, channel quad item & 3);
  //      scalar item -> (pixel item & 127, k row item >> 7)
  int py[NA], px[NA];                             // pixel coordinates; py = -4 marks a row beyond M
  size_t pbase[NA];                               // element offset of the pixel's channel 0
#pragma unroll
  for (int r = 0; r < NA; ++r) {
    const int item = tid + r * THREADS;
    const int m = m0 + (VEC ? item >> 2 : item & (BM - 1));
    if (m < M) {
      const int rem = m % HW;
      py[r] = rem / W; px[r] = rem % W;
      pbase[r] = (size_t)m * Cin;
    } else {
      py[r] = -4; px[r] = 0; pbase[r] = 0;
    }
  }

  float4 ra[VEC ? 2 : 1];
  float rs[VEC ? 1 : 8];
  float4 rb[NT];
  auto load_chunk = [&](int k0) {
    if constexpr (VEC) {
      const int tap = k0 / Cin, c0 = k0 - tap * Cin;
      const int dy = tap / 3 - 1, dx = tap % 3 - 1;
#pragma unroll
      for (int r = 0; r < 2; ++r) {
        const int q = (tid + r * THREADS) & 3;
        const int sy = py[r] + dy, sx = px[r] + dx;
        if (sy >= 0 && sy < H && sx >= 0 && sx < W)
          ra[r] = *reinterpret_cast<const float4*>(x + (ptrdiff_t)pbase[r] + ((ptrdiff_t)dy * W + dx) * Cin + c0 + 4 * q);
        else
          ra[r] = make_float4(0.f, 0.f, 0.f, 0.f);
      }
    } else {
#pragma unroll
      for (int r = 0; r < 8; ++r) {
        const int k = k0 + ((tid + r * THREADS) >> 7);
        float v = 0.f;
        if (k < K) {
          const int tap = k / Cin, c = k - tap * Cin;
          const int dy = tap / 3 - 1, dx = tap % 3 - 1;
          const int sy = py[r] + dy, sx = px[r] + dx;
          if (sy >= 0 && sy < H && sx >= 0 && sx < W) v = x[(ptrdiff_t)pbase[r] + ((ptrdiff_t)dy * W + dx) * Cin + c];
        }
        rs[r] = v;
      }
    }
#pragma unroll
    for (int r = 0; r < NT; ++r) {
      const int item = tid + r * THREADS, kk = item / (BN / 4), nq = item % (BN / 4);
      rb[r] = *reinterpret_cast<const float4*>(wp + (size_t)(k0 + kk) * Cout + n0 + 4 * nq);
    }
  };
  auto store_chunk = [&]() {
    if constexpr (VEC) {
#pragma unroll
      for (int r = 0; r < 2; ++r) {
        const int item = tid + r * THREADS, ml = item >> 2, q = item & 3;
        As[(4 * q + 0) * LDA + ml] = ra[r].x;
        As[(4 * q + 1) * LDA + ml] = ra[r].y;
        As[(4 * q + 2) * LDA + ml] = ra[r].z;
        As[(4 * q + 3) * LDA + ml] = ra[r].w;
      }
    } else {
#pragma unroll
      for (int r = 0; r < 8; ++r) {
        const int item = tid + r * THREADS;
        As[(item >> 7) * LDA + (item & (BM - 1))] = rs[r];
      }
    }
#pragma unroll
    for (int r = 0; r < NT; ++r) {
      const int item = tid + r * THREADS, kk = item / (BN / 4), nq = item % (BN / 4);
      *reinterpret_cast<float4*>(Bs + kk * BN + 4 * nq) = rb[r];
    }
  };

  f32x16 acc[2][NT];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < NT; ++j)
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.f;

  const int wm = wv & 1, wn = wv >> 1, lr = lane & 31, lh = lane >> 5;
  const float* a_rd = As + lh * LDA + wm * 64 + lr;
  const float* b_rd = Bs + lh * BN + wn * (BN / 2) + lr;

  load_chunk(0);
  for (int k0 = 0; k0 < Kp; k0 += KC) {
    __syncthreads();                              // the previous chunk's MFMA operands have been read
    store_chunk();
    __syncthreads();
    if (k0 + KC < Kp) load_chunk(k0 + KC);
#pragma unroll
    for (int s = 0; s < KC / 2; ++s) {
      float a[2], b[NT];
#pragma unroll
      for (int i = 0; i < 2; ++i) a[i] = a_rd[2 * s * LDA + i * 32];
#pragma unroll
      for (int j = 0; j < NT; ++j) b[j] = b_rd[2 * s * BN + j * 32];
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < NT; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[i], b[j], acc[i][j], 0, 0, 0);
    }
  }

  // ---- bias, ReLU, store: C/D element e of lane (lr, lh) is row (e & 3) + 8 * (e >> 2) + 4 * lh, column lr
#pragma unroll
  for (int j = 0; j < NT; ++j) {
    const int n = n0 + wn * (BN / 2) + j * 32 + lr;
    const float bv = bias[n];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        const int m = m0 + wm * 64 + i * 32 + (e & 3) + 8 * (e >> 2) + 4 * lh;
        if (m < M) y[(size_t)m * Cout + n] = fmaxf(acc[i][j][e] + bv, 0.f);
      }
  }
}

__global__ __launch_bounds__(256) void lpips_pack_conv_kernel(int Cin, int Cout, int Kp, const float* __restrict__ w,
                                                              float* __restrict__ wp) {
  const int idx = blockIdx.x * 256 + threadIdx.x;
  if (idx >= Kp * Cout) return;
  const int k = idx / Cout, o = idx - k * Cout;
  float v = 0.f;
  if (k < 9 * Cin) {
    const int tap = k / Cin, c = k - tap * Cin;
    v = w[((size_t)o * Cin + c) * 9 + tap];
  }
  wp[idx] = v;
}

}  // namespace

void launch_lpips_pack_conv(hipStream_t st, int Cin, int Cout, const float* w, float* wp) {
  const int Kp = lpips_kp(Cin), n = Kp * Cout;
  lpips_pack_conv_kernel<<<(n + 255) / 256, 256, 0, st>>>(Cin, Cout, Kp, w, wp);
}

void launch_lpips_conv3x3_relu(hipStream_t st, int n_images, int H, int W, int Cin, int Cout, const float* x, const float* wp,
                               const float* bias, float* y) {
  const int M = n_images * H * W, Kp = lpips_kp(Cin);
  const bool vec = Cin % 16 == 0;
  const int mb = (M + BM - 1) / BM;
  if (Cout % 128 == 0) {
    const dim3 grid(mb, Cout / 128);
    if (vec) lpips_conv3x3_kernel<128, true><<<grid, THREADS, 0, st>>>(M, H, W, Cin, Cout, Kp, x, wp, bias, y);
    else lpips_conv3x3_kernel<128, false><<<grid, THREADS, 0, st>>>(M, H, W, Cin, Cout, Kp, x, wp, bias, y);
  } else {
    const dim3 grid(mb, Cout / 64);
    if (vec) lpips_conv3x3_kernel<64, true><<<grid, THREADS, 0, st>>>(M, H, W, Cin, Cout, Kp, x, wp, bias, y);
    else lpips_conv3x3_kernel<64, false><<<grid, THREADS, 0, st>>>(M, H, W, Cin, Cout, Kp, x, wp, bias, y);
  }
}

// Device-side vocabulary every library of the package shares: vector types, the SGPR-pair pointer, the LDS-DMA wrappers the
// counted vmcnt waits rely on, the transposed fragment read, the wave reductions and scans.  Header-only (nothing here is an
// exported symbol); a kernel file takes what it uses into its own namespace with using declarations or a using directive.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <atomic>

namespace hipdev {

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x2 __attribute__((ext_vector_type(2)));
typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x8 __attribute__((ext_vector_type(8)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef short s16x2 __attribute__((ext_vector_type(2)));
typedef short s16x8 __attribute__((ext_vector_type(8)));
typedef unsigned short u16x2 __attribute__((ext_vector_type(2)));

// a wave-uniform pointer as an SGPR pair
__device__ __forceinline__ uint64_t uniform64(const void* p) {
  const uint64_t b = (uint64_t)(uintptr_t)p;
  return ((uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((uint32_t)(b >> 32)) << 32) |
         (uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((uint32_t)b);
}

// ---------------------------------------------------------------------------------------------------------------------
// LDS-DMA of 64 x 16 bytes (global_load_lds_dwordx4), LDS address = lds_abs + 16 * lane.  Inline asm: hipcc's waitcnt pass
// must not see it, or it drains vmcnt to 0 before every LDS read of a ring (it cannot prove that the reads do not alias the
// in-flight destination); completion is tracked by the kernels' counted s_waitcnt instead, which relies on a wrapper being
// exactly N VMEM instructions.  M0 carries the wave-uniform LDS destination; it is saved and restored inside the statement
// (the compiler does not track it).
//   glds16xN_saddr<N>: global address = wave-uniform base (SGPR pair) + per-lane byte offset (one VGPR): no 64-bit VALU add.
//                      N (<= 4) consecutive 1 KiB fragments with ONE M0 / address set-up: the instruction offset advances
//                      the global and the LDS address alike.
//   glds16_saddr:      the same for one fragment
//   glds16_vaddr<NT>:  global address = per-lane pointer (a VGPR pair); NT: non-temporal (streams nothing re-reads)
#define GLDS_HEAD "s_mov_b32 %0, m0\n\ts_mov_b32 m0, %3\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, %2"
#define GLDS_TAIL "\n\ts_mov_b32 m0, %0"
template <int N>
__device__ __forceinline__ void glds16xN_saddr(const void* sbase, uint32_t voff, uint32_t lds_abs) {
  static_assert(N >= 1 && N <= 4, "the 13-bit instruction offset reaches 3 x 1024");
  const uint32_t dst = __builtin_amdgcn_readfirstlane(lds_abs);
  const uint64_t base = uniform64(sbase);
  uint32_t keep;
  if constexpr (N == 4)
    asm volatile(GLDS_HEAD "\n\tglobal_load_lds_dwordx4 %1, %2 offset:1024\n\tglobal_load_lds_dwordx4 %1, %2 offset:2048\n\t"
                 "global_load_lds_dwordx4 %1, %2 offset:3072" GLDS_TAIL : "=&s"(keep) : "v"(voff), "s"(base), "s"(dst) : "memory");
  else if constexpr (N == 3)
    asm volatile(GLDS_HEAD "\n\tglobal_load_lds_dwordx4 %1, %2 offset:1024\n\tglobal_load_lds_dwordx4 %1, %2 offset:2048" GLDS_TAIL
                 : "=&s"(keep) : "v"(voff), "s"(base), "s"(dst) : "memory");
  else if constexpr (N == 2)
    asm volatile(GLDS_HEAD "\n\tglobal_load_lds_dwordx4 %1, %2 offset:1024" GLDS_TAIL : "=&s"(keep) : "v"(voff), "s"(base), "s"(dst) : "memory");
  else
    asm volatile(GLDS_HEAD GLDS_TAIL : "=&s"(keep) : "v"(voff), "s"(base), "s"(dst) : "memory");
}
#undef GLDS_HEAD
#undef GLDS_TAIL
__device__ __forceinline__ void glds16_saddr(const void* sbase, uint32_t voff, uint32_t lds_abs) { glds16xN_saddr<1>(sbase, voff, lds_abs); }
#define GLDS_VADDR(mod) asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off" mod \
                                     "\n\ts_mov_b32 m0, %0" : "=&s"(keep) : "v"(g), "s"(dst) : "memory")
template <bool NT = false>
__device__ __forceinline__ void glds16_vaddr(const void* g, uint32_t lds_abs) {
  const uint32_t dst = __builtin_amdgcn_readfirstlane(lds_abs);
  uint32_t keep;
  if constexpr (NT) GLDS_VADDR(" nt");
  else GLDS_VADDR("");
}
#undef GLDS_VADDR

// MFMA fragment (8 consecutive k per lane) from two ds_read_b64_tr_b16 transposed reads of the dynamic LDS array `smem`:
// k 0..3 at byte `off`, k 4..7 at `off + second`.  (An address_space(3) pointer + 32-bit byte offset: a flat pointer would
// drag a flat->LDS null check into divergent code.)
__device__ __forceinline__ bf16x8 tr_frag(const char* smem, uint32_t off, uint32_t second) {
  __attribute__((address_space(3))) char* base = (__attribute__((address_space(3))) char*)smem;
  const bf16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((__attribute__((address_space(3))) bf16x4*)(base + off));
  const bf16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((__attribute__((address_space(3))) bf16x4*)(base + off + second));
  return __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
}

// ---------------------------------------------------------------------------------------------------------------------
// Sums over the 64 lanes of a wave, each a fixed tree.  Two different operations:
//   wave_sum:       xor butterfly, EVERY lane ends with the sum (the same bits in all of them)
//   wave_sum_lane0: shfl_down tree, LANE 0 holds the sum, the other lanes partial ones
template <typename T>
__device__ __forceinline__ T wave_sum(T v) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d, 64);
  return v;
}
template <typename T>
__device__ __forceinline__ T wave_sum_lane0(T v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
  return v;
}
__device__ __forceinline__ uint32_t wave_sum_lane0(uint32_t v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += (uint32_t)__shfl_down((int)v, o, 64);
  return v;
}
// ---------------------------------------------------------------------------------------------------------------------
// Sums over a workgroup, each a fixed tree of the block size alone: equal inputs give equal bits.  Two shapes are in use.
//
// The wave sums of a workgroup of W waves, in wave order, as two steps around the CALLER's __syncthreads():
//   wave_deposit:  lane 0 of each wave stores s, its wave's sum (wave_sum or wave_sum_lane0 of the thread's value), to red[wave][k]
//   waves_collect: red[0][k] + red[1][k] + ... + red[W-1][k], added left to right in an accumulator of type A; whoever calls it
//                  (every thread, thread 0, thread k for column k) gets the same bits
template <typename T, int W, int K>
__device__ __forceinline__ void wave_deposit(T (&red)[W][K], int k, T s) {
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6][k] = s;
}
template <typename A, typename T, int W, int K>
__device__ __forceinline__ A waves_collect(const T (&red)[W][K], int k) {
  A s = red[0][k];
#pragma unroll
  for (int w = 1; w < W; ++w) s += red[w][k];
  return s;
}
// The LDS halving tree over a workgroup of B threads (a power of two), K sums side by side in one barrier sequence: thread t
// stores v[k] to sh[k][t]; then, for d = B/2, B/4, ..., 1, every thread t < d does sh[k][t] += sh[k][t + d], a barrier after the
// stores and after each d.  The sums are in sh[k][0], visible to every thread, on return.  The steps stay a loop (unroll 1), as
// they were at every site that calls this while the block size was read from blockDim: the constant B changes no ds_, barrier or
// floating-point instruction of those kernels.
template <int B, int K>
__device__ __forceinline__ void lds_tree_sum(double (&sh)[K][B], const double (&v)[K]) {
  static_assert(B >= 2 && (B & (B - 1)) == 0, "the tree halves a power of two");
#pragma unroll
  for (int k = 0; k < K; ++k) sh[k][threadIdx.x] = v[k];
  __syncthreads();
#pragma unroll 1
  for (int d = B >> 1; d > 0; d >>= 1) {
    if ((int)threadIdx.x < d)
#pragma unroll
      for (int k = 0; k < K; ++k) sh[k][threadIdx.x] += sh[k][threadIdx.x + d];
    __syncthreads();
  }
}

// The scalars of a loss head that a multi-level depth loss folds its per-level values into; a null pointer skips that one.
struct LevelFolds {
  float* total; float* last; float* others; float* n_sup;
};
// float32, in level order: *total += sum_l scale[l] * values[l]; *last = values[L-1]; *others = sum_{l < L-1} values[l];
// *n_sup = n_sup.  One thread calls it.
__device__ __forceinline__ void fold_levels(const LevelFolds& f, const float* values, const float* scale, int L, float n_sup) {
  float total = 0.f, others = 0.f, last = 0.f;
  for (int l = 0; l < L; ++l) {
    const float v = values[l];
    total += scale[l] * v;
    if (l < L - 1) others += v;
    else last = v;
  }
  if (f.total) *f.total += total;
  if (f.last) *f.last = last;
  if (f.others) *f.others = others;
  if (f.n_sup) *f.n_sup = n_sup;
}

// inclusive prefix sum across the wave: out(lane) = sum_{l <= lane} x(l)
__device__ __forceinline__ float wave_incl_sum(float x, int lane) {
  float v = x;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const float t = __shfl_up(v, d, 64);
    if (lane >= d) v += t;
  }
  return v;
}
// exclusive suffix sum (the inclusive scan from the top, shifted by one): out(lane) = sum_{l > lane} x(l)
__device__ __forceinline__ float wave_excl_suffix_sum(float x, int lane) {
  float v = x;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const float t = __shfl_down(v, d, 64);
    if (lane + d < 64) v += t;
  }
  const float e = __shfl_down(v, 1, 64);
  return lane == 63 ? 0.f : e;
}

// Host: hipFuncSetAttribute is per device: remember which devices of this process have had it applied (one bit per device id)
static inline bool first_launch_on_this_device(std::atomic<uint64_t>& done) {
  int dev = 0;
  (void)hipGetDevice(&dev);
  const uint64_t bit = 1ull << (dev & 63);
  return (done.fetch_or(bit) & bit) == 0;
}

}  // namespace hipdev

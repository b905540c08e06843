// Device-side vocabulary of libmip360_hip.so: the one definition of the fragment-major layout and of the primitives the
// mip360_*.hip kernels share.  Every kernel file takes what it uses into its own namespace with using declarations.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <atomic>

namespace mip360dev {

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef short s16x2 __attribute__((ext_vector_type(2)));
typedef unsigned short u16x2 __attribute__((ext_vector_type(2)));

// ---------------------------------------------------------------------------------------------------------------------
// Layout ("fm").  A [rows, ld] bf16 tensor (rows % 32 == 0, ld % 16 == 0) is stored as 1 KiB blocks of 32 rows x 16
// columns, block (r / 32, c / 16) at ((r / 32) * (ld / 16) + c / 16) * 1024.  Inside a block the 16-byte unit of
// (row, hi) -- hi = ((c % 16) / 4) % 2 -- holds the 8 columns {4 hi + 0..3, 8 + 4 hi + 0..3} (element t = 4 ((c % 16) / 8)
// + c % 4) and sits at unit index  u = 8 (row >> 2) + 4 (hi ^ (row >> 4)) + (row & 3).
//   * A unit is exactly what one lane of v_mfma_f32_32x32x16_bf16 supplies for a 16-wide k step (lane = row + 32 hi; the
//     k order inside the step is the same permutation for both operands, so the contraction is exact), AND what one lane
//     of the 32 x 32 accumulator block owns of a 16-column block of the output (registers 8 b .. 8 b + 7 of lane
//     (row, hi) are columns 16 b + {4 hi + 0..3, 8 + 4 hi + 0..3}).  So a layer's epilogue stores its accumulators with
//     plain 16-byte stores, 1 KiB contiguous per wave instruction, no LDS staging, and the next layer's operand DMA
//     (global_load_lds_dwordx4) is a linear copy of whole blocks whose LDS image needs no swizzle.
//   * The unit order makes BOTH read patterns conflict-free: ds_read_b128 by lane (row, hi) (the 16-lane service groups
//     of MI355X_MICROARCH.md "LDS" see 16 distinct units mod 16), and the ds_read_b64_tr_b16 patches of the weight-
//     gradient kernel (4 rows x 16 columns = 8 consecutive units).
constexpr int FM_BLOCK = 1024;                                                       // bytes of a block
// bytes from one 32-row block of a tensor with ld columns to the next
__host__ __device__ __forceinline__ size_t fm_row_block_bytes(int ld) { return (size_t)(ld >> 4) * FM_BLOCK; }
// index of block (rb, cb); its address is FM_BLOCK times that
__host__ __device__ __forceinline__ size_t fm_block_index(size_t rb, int cb, int ld) { return rb * (ld >> 4) + cb; }
__host__ __device__ __forceinline__ uint32_t unit_of(int row, int hi) { return 8u * (row >> 2) + 4u * (hi ^ (row >> 4)) + (row & 3); }
__device__ __forceinline__ void unit_to_row_hi(int u, int& row, int& hi) {
  row = ((u >> 3) << 2) | (u & 3);
  hi = ((u >> 2) & 1) ^ (row >> 4);
}
// element (r, c) of an fm tensor with ld columns, in elements
__device__ __forceinline__ size_t fm_elem(int r, int c, int ld) {
  const int row = r & 31, f = c & 15, hi = (f >> 2) & 1;
  return fm_block_index(r >> 5, c >> 4, ld) * (FM_BLOCK / 2) + (size_t)unit_of(row, hi) * 8 + 4 * (f >> 3) + (f & 3);
}

// 32 x 32 accumulator block of v_mfma_f32_32x32x16_bf16 whose first row is row0: lane (j = lane & 31, hi = lane >> 5) holds
// column j; its register r is this row.  (The same map gives the 8 columns of a 16-column block that element r < 8 of the fm
// unit (row, hi) holds.)
__host__ __device__ __forceinline__ int acc_row(int row0, int r, int hi) { return row0 + (r & 3) + 8 * (r >> 2) + 4 * hi; }

// ---------------------------------------------------------------------------------------------------------------------
// a wave-uniform pointer as an SGPR pair
__device__ __forceinline__ uint64_t uniform64(const void* p) {
  const uint64_t b = (uint64_t)(uintptr_t)p;
  return ((uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((uint32_t)(b >> 32)) << 32) |
         (uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((uint32_t)b);
}

// LDS-DMA of 64 x 16 bytes, LDS address = lds_abs + 16 * lane.  M0 is saved and restored around the instruction; the counted
// vmcnt waits of the kernels rely on this being exactly one VMEM instruction.
//   glds16_saddr: global address = wave-uniform base (SGPR pair) + per-lane byte offset (one VGPR)
//   glds16_vaddr: global address = per-lane pointer (a VGPR pair)
__device__ __forceinline__ void glds16_saddr(const void* sbase, uint32_t voff, uint32_t lds_abs) {
  const uint32_t dst = __builtin_amdgcn_readfirstlane(lds_abs);
  const uint64_t base = uniform64(sbase);
  uint32_t keep;
  asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %3\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, %2\n\ts_mov_b32 m0, %0"
               : "=&s"(keep) : "v"(voff), "s"(base), "s"(dst) : "memory");
}
__device__ __forceinline__ void glds16_vaddr(const void* g, uint32_t lds_abs) {
  const uint32_t dst = __builtin_amdgcn_readfirstlane(lds_abs);
  uint32_t keep;
  asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off\n\ts_mov_b32 m0, %0"
               : "=&s"(keep) : "v"(g), "s"(dst) : "memory");
}

// MFMA fragment (8 consecutive k per lane) from two ds_read_b64_tr_b16 transposed reads of the dynamic LDS array `smem`:
// k 0..3 at byte `off`, k 4..7 at `off + second`
__device__ __forceinline__ bf16x8 tr_frag(const char* smem, uint32_t off, uint32_t second) {
  __attribute__((address_space(3))) char* base = (__attribute__((address_space(3))) char*)smem;
  const bf16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((__attribute__((address_space(3))) bf16x4*)(base + off));
  const bf16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((__attribute__((address_space(3))) bf16x4*)(base + off + second));
  return __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
}

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d, 64);
  return v;
}

// Split-K weight gradients: workgroup -> (row slice, tile b of `tiles`).  XCD-aware order (workgroup g runs on XCD g % 8, one
// L2 per XCD): all tiles of a row slice go to ONE XCD, so the slice's H / dZ rows are fetched from HBM once and re-used by
// its workgroups through that L2.
struct SliceTile { int slice, b; };
__device__ __forceinline__ SliceTile xcd_slice_order(int ksplit, int tiles) {
  int slice, b;
  if ((ksplit & 7) == 0) {
    const int xcd = blockIdx.x & 7, id = blockIdx.x >> 3, per_xcd = ksplit >> 3;
    slice = xcd * per_xcd + id / tiles;
    b = id % tiles;
  } else {
    slice = blockIdx.x / tiles;
    b = blockIdx.x - slice * tiles;
  }
  return {slice, b};
}

// Host: hipFuncSetAttribute is per device: remember which devices of this process have had it applied (one bit per device id)
static inline bool first_launch_on_this_device(std::atomic<uint64_t>& done) {
  int dev = 0;
  (void)hipGetDevice(&dev);
  const uint64_t bit = 1ull << (dev & 63);
  return (done.fetch_or(bit) & bit) == 0;
}

}  // namespace mip360dev

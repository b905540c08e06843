// Device-side vocabulary of libmip360_hip.so: the one definition of the fragment-major layout, the accumulator row map and
// the split-K slice order; what is not specific to this library (vector types, DMA wrappers, reductions) comes from
// hip_device.h.  Every kernel file takes what it uses into its own namespace with using declarations.
#pragma once
#include "hip_device.h"

namespace mip360dev {

using namespace hipdev;      // vector types, uniform64, glds16_*, tr_frag, wave_sum, first_launch_on_this_device

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

}  // namespace mip360dev

/* lpips_hip.h -- C ABI of liblpips_hip.so: LPIPS v0.1 (VGG-16 features, linear heads, spatial mean) of 8-bit image
 * pairs on the MI355X (gfx950), from weights the caller supplies.  The definition is DESIGN.md 8.2 and, as executable
 * code, tests/lpips_reference.py; it has not been compared with the `lpips` pip package.
 *
 * Conventions as in nerfpp_hip.h and mip360_hip.h: plain C, raw DEVICE pointers, a `void* stream` (hipStream_t), return
 * LPIPS_OK or an error code with lpips_last_error(); the library is stateless and the caller owns every buffer.  The
 * `*_bytes` / `*_floats` queries and every argument check touch no HIP call and work on a host without a GPU.
 *
 * Arithmetic: the 13 convolutions are implicit GEMMs on v_mfma_f32_32x32x2_f32 (float32 operands, float32
 * accumulation, a k-ordered fma chain); the tap reductions run in float64.  No atomics: partial sums are added in a
 * fixed order, so a pair's six values depend on that pair's bytes alone and are the same bits from call to call.
 */
#ifndef LPIPS_HIP_H
#define LPIPS_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define LPIPS_ABI_VERSION 1
#define LPIPS_OK 0
#define LPIPS_ERR_ARG 1
#define LPIPS_ERR_HIP 2

#define LPIPS_N_CONV 13            /* VGG-16 `features` convolutions: 3-64 64-64 | 64-128 128-128 | 128-256 256-256 x2 |
                                      256-512 512-512 x2 | 512-512 x3; a tap after the ReLU of layers 1, 3, 6, 9, 12 */
#define LPIPS_N_TAPS 5
#define LPIPS_MIN_SIDE 16          /* four 2 x 2 pools must leave one pixel */
#define LPIPS_GROUP_BYTES (2ll << 30)   /* bound on the two feature buffers of lpips_u8: pairs are processed in groups that
                                           fit it (one pair at a time if a single pair exceeds it) */

const char* lpips_last_error(void);
int lpips_abi_version(void);

/* One layer on its own.  Operand layout of a 3 x 3 convolution: wp [Kp, Cout] float32 with row k = (ky * 3 + kx) * Cin + c,
 * Kp = 9 * Cin rounded up to a multiple of 16 (zero rows).  lpips_packed_conv_floats = Kp * Cout, or -1 (Cin < 1, Cout not
 * a positive multiple of 64).  lpips_pack_conv: w [Cout, Cin, 3, 3] (the state-dict layout) -> wp. */
int64_t lpips_packed_conv_floats(int Cin, int Cout);
int lpips_pack_conv(void* stream, int Cin, int Cout, const float* w, float* wp);
/* y [n_images, H, W, Cout] = relu(conv3x3(x [n_images, H, W, Cin], zero padding 1, stride 1) + bias); NHWC float32,
 * x, wp, y aligned to 16 bytes; y must not overlap x. */
int lpips_conv3x3_relu(void* stream, int n_images, int H, int W, int Cin, int Cout, const float* x, const float* wp,
                       const float* bias, float* y);

/* The whole network.  `flat` (float32, lpips_flat_floats() values): for each of the 13 convolutions in order
 * weight [Cout, Cin, 3, 3] then bias [Cout], then the five lin weights [C_l] (C_l = 64, 128, 256, 512, 512).
 * lpips_pack_weights writes the operand layout (lpips_packed_bytes() bytes, 16-byte aligned) once per process. */
int64_t lpips_flat_floats(void);
int64_t lpips_packed_bytes(void);
int lpips_pack_weights(void* stream, const float* flat, void* packed);

/* LPIPS of n_pairs image pairs gt_u8 / pred_u8 [n_pairs, H, W, 3] uint8.  out [n_pairs, 6] float64: d_0 .. d_4 and their
 * sum.  H, W >= 16, H * W <= 2^26, 1 <= n_pairs <= 65535; lpips_workspace_bytes returns -1 otherwise.  workspace:
 * lpips_workspace_bytes(n_pairs, H, W) bytes, aligned to 256. */
int64_t lpips_workspace_bytes(int n_pairs, int H, int W);
int lpips_u8(void* stream, int n_pairs, int H, int W, const uint8_t* gt_u8, const uint8_t* pred_u8, const void* packed,
             void* workspace, double* out);

#ifdef __cplusplus
}
#endif
#endif

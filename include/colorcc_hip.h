/* colorcc_hip.h -- C ABI of libcolorcc_hip.so: the colour correction of finished test renders against their ground-truth
 * frames (upstream's image.color_correct, nerf-methods/mipnerf360/internal/image.py:81-124) and the PSNR of the corrected
 * frames, on the MI355X (gfx950).  The definition is DESIGN.md 8.3 and, as executable code, tests/color_correct_reference.py.
 *
 * Conventions as in lpips_hip.h: plain C, raw DEVICE pointers, a `void* stream` (hipStream_t), return COLORCC_OK or an
 * error code with colorcc_last_error(); the library is stateless and the caller owns every buffer.  The `*_bytes` query and
 * every argument check touch no HIP call and work on a host without a GPU.  Both calls only enqueue: the 10 x 10 systems are
 * solved on the device.
 *
 * Arithmetic: float64 throughout, no implicit fma.  No atomics: a frame's sums are per-workgroup partials added in
 * workgroup order, and the number of workgroups of a frame depends on H * W alone, so a frame's results depend on that
 * frame's values alone and are the same bits from call to call and for any batch the frame is part of.
 */
#ifndef COLORCC_HIP_H
#define COLORCC_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define COLORCC_ABI_VERSION 1
#define COLORCC_OK 0
#define COLORCC_ERR_ARG 1
#define COLORCC_ERR_HIP 2

#define COLORCC_ITERS 5            /* fits per frame (upstream's num_iters) */
#define COLORCC_FEATURES 10        /* r*r r*g r*b g*g g*b b*b r g b 1 */
#define COLORCC_SUMS 66            /* per channel: 55 Gram entries (upper triangle, row-major: (0,0) (0,1) .. (0,9) (1,1) ..
                                      (9,9)), 10 right-hand sides, the number of rows in the mask */
#define COLORCC_OUT 17             /* out row: squared-error sum, value count H * W * 3, 5 x 3 mask counts [iteration][channel] */
#define COLORCC_MAX_PIXELS (1ll << 28)
#define COLORCC_RANK_CUTOFF 1e-13  /* eigenvalues of the unit-diagonal Gram matrix at or below this share of the largest are
                                      treated as zero (pseudo-inverse) */

const char* colorcc_last_error(void);
int colorcc_abi_version(void);

/* Bytes of the workspace of either call below (aligned to 256 by the caller).  -1 with a message for n_frames < 1 or
 * > 65535, H < 1, W < 1 or H * W > 2^28. */
int64_t colorcc_workspace_bytes(int n_frames, int H, int W);

/* The whole split in one call.  img_f32 [n_frames, H, W, 3] float32 (the renders; non-finite values count as 0),
 * ref_u8 [n_frames, H, W, 3] uint8 (the ground-truth bytes, ref = byte / 255).  Writes rgb_cc_f64 [n_frames, H, W, 3] float64
 * (the corrected frames, in [0, 1]), cc_u8 [n_frames, H, W, 3] uint8 (rgb_cc * 255, truncated: the PNG's bytes) and
 * out [n_frames, COLORCC_OUT] float64: sum((q(rgb_cc) - ref)^2) with q = rint(. * 255) / 255 if quantize != 0, else the
 * identity; H * W * 3; then mask counts.  rgb_cc_f64 or cc_u8 may be null (not written). */
int colorcc_correct(void* stream, int n_frames, int H, int W, const float* img_f32, const uint8_t* ref_u8, int quantize,
                    void* workspace, double* rgb_cc_f64, uint8_t* cc_u8, double* out);

/* The masked normal equations of iteration 0 alone: sums [n_frames, 3, COLORCC_SUMS] float64, channel c's system being
 * sum over rows in its mask of a a^T (upper triangle), a * ref_c and 1. */
int colorcc_normal_equations(void* stream, int n_frames, int H, int W, const float* img_f32, const uint8_t* ref_u8,
                             void* workspace, double* sums);

#ifdef __cplusplus
}
#endif
#endif

// extern "C" surface of libcolorcc_hip.so (include/colorcc_hip.h): argument checks (no HIP call, so a host without a GPU
// gets the same errors), the workspace layout and the launch sequence: 5 x (accumulate, solve), apply, finish.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include "../../include/colorcc_hip.h"
#define API_OK COLORCC_OK
#define API_ERR_HIP COLORCC_ERR_HIP
#define API_ERR_ARG COLORCC_ERR_ARG
#include "api_common.h"
#include "colorcc_kernels.h"

namespace {

int sizes_ok(const char* fn, int n_frames, int H, int W) {
  if (n_frames < 1 || n_frames > 65535) return fail(COLORCC_ERR_ARG, "%s: n_frames = %d, expected 1 .. 65535", fn, n_frames);
  if (H < 1 || W < 1) return fail(COLORCC_ERR_ARG, "%s: a %d x %d image has no pixel (H * W >= 1)", fn, H, W);
  if ((int64_t)H * W > COLORCC_MAX_PIXELS) return fail(COLORCC_ERR_ARG, "%s: a %d x %d image exceeds 2^28 pixels", fn, H, W);
  return COLORCC_OK;
}

int64_t align_up(int64_t v, int64_t a) { return (v + a - 1) / a * a; }

// doubles: weights [F, 5, 3, 10] | partials [F, 3, nwg, 66] | sse partials [F, nwg]
struct WsLayout { int nwg; int64_t weights, partials, sse, total; };
WsLayout ws_layout(int n_frames, int H, int W) {
  WsLayout L;
  L.nwg = colorcc_workgroups((int64_t)H * W);
  L.weights = 0;
  L.partials = L.weights + (int64_t)n_frames * COLORCC_ITERS * 3 * COLORCC_FEATURES;
  L.sse = L.partials + (int64_t)n_frames * 3 * L.nwg * COLORCC_SUMS;
  L.total = align_up((L.sse + (int64_t)n_frames * L.nwg) * 8, 256);
  return L;
}

}  // namespace

extern "C" {

const char* colorcc_last_error(void) { return g_err; }
int colorcc_abi_version(void) { return COLORCC_ABI_VERSION; }

int64_t colorcc_workspace_bytes(int n_frames, int H, int W) {
  if (sizes_ok(__func__, n_frames, H, W) != COLORCC_OK) return -1;
  return ws_layout(n_frames, H, W).total;
}

int colorcc_correct(void* stream, int n_frames, int H, int W, const float* img_f32, const uint8_t* ref_u8, int quantize,
                    void* workspace, double* rgb_cc_f64, uint8_t* cc_u8, double* out) {
  const int rc = sizes_ok(__func__, n_frames, H, W);
  if (rc != COLORCC_OK) return rc;
  REQUIRE(img_f32 && ref_u8 && workspace && out, "non-null img_f32, ref_u8, workspace, out");
  REQUIRE(((uintptr_t)img_f32 & 3) == 0, "img_f32 aligned to 4 bytes");
  REQUIRE(((uintptr_t)workspace & 255) == 0 && ((uintptr_t)out & 7) == 0 && ((uintptr_t)rgb_cc_f64 & 7) == 0,
          "workspace aligned to 256 bytes, out and rgb_cc_f64 to 8");
  const hipStream_t st = (hipStream_t)stream;
  const WsLayout L = ws_layout(n_frames, H, W);
  const int64_t n_pixels = (int64_t)H * W;
  double* ws = (double*)workspace;
  for (int it = 0; it < COLORCC_ITERS; ++it) {
    launch_colorcc_accumulate(st, n_frames, n_pixels, L.nwg, img_f32, ref_u8, ws + L.weights, it, ws + L.partials);
    launch_colorcc_solve(st, n_frames, L.nwg, ws + L.partials, it, ws + L.weights, out, nullptr);
  }
  launch_colorcc_apply(st, n_frames, n_pixels, L.nwg, img_f32, ref_u8, ws + L.weights, quantize, rgb_cc_f64, cc_u8, ws + L.sse);
  launch_colorcc_finish(st, n_frames, n_pixels, L.nwg, ws + L.sse, out);
  return check_launch("colorcc_correct");
}

int colorcc_normal_equations(void* stream, int n_frames, int H, int W, const float* img_f32, const uint8_t* ref_u8,
                             void* workspace, double* sums) {
  const int rc = sizes_ok(__func__, n_frames, H, W);
  if (rc != COLORCC_OK) return rc;
  REQUIRE(img_f32 && ref_u8 && workspace && sums, "non-null img_f32, ref_u8, workspace, sums");
  REQUIRE(((uintptr_t)img_f32 & 3) == 0, "img_f32 aligned to 4 bytes");
  REQUIRE(((uintptr_t)workspace & 255) == 0 && ((uintptr_t)sums & 7) == 0, "workspace aligned to 256 bytes, sums to 8");
  const hipStream_t st = (hipStream_t)stream;
  const WsLayout L = ws_layout(n_frames, H, W);
  double* ws = (double*)workspace;
  launch_colorcc_accumulate(st, n_frames, (int64_t)H * W, L.nwg, img_f32, ref_u8, ws + L.weights, 0, ws + L.partials);
  launch_colorcc_solve(st, n_frames, L.nwg, ws + L.partials, 0, ws + L.weights, nullptr, sums);
  return check_launch("colorcc_normal_equations");
}

}  // extern "C"

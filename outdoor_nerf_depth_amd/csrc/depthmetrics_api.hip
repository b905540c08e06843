// extern "C" surface of libdepthmetrics_hip.so (include/depthmetrics_hip.h): argument checks (no HIP call, so a host without a
// GPU gets the same errors), the workspace layout and the two launches.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include "../../include/depthmetrics_hip.h"
#define API_OK DEPTHMETRICS_OK
#define API_ERR_HIP DEPTHMETRICS_ERR_HIP
#define API_ERR_ARG DEPTHMETRICS_ERR_ARG
#include "api_common.h"
#include "depthmetrics_kernels.h"

namespace {

int sizes_ok(const char* fn, int n_frames, int64_t n_pixels) {
  if (n_frames < 1 || n_frames > DEPTHMETRICS_MAX_FRAMES)
    return fail(DEPTHMETRICS_ERR_ARG, "%s: n_frames = %d, expected 1 .. %d", fn, n_frames, DEPTHMETRICS_MAX_FRAMES);
  if (n_pixels < 1) return fail(DEPTHMETRICS_ERR_ARG, "%s: n_pixels = %lld: a frame has at least one pixel", fn, (long long)n_pixels);
  if (n_pixels > DEPTHMETRICS_MAX_PIXELS)
    return fail(DEPTHMETRICS_ERR_ARG, "%s: n_pixels = %lld exceeds 2^28 pixels per frame", fn, (long long)n_pixels);
  return DEPTHMETRICS_OK;
}

// bytes: partial [F, nwg, 9] float64
int64_t ws_bytes(int n_frames, int64_t n_pixels) {
  const int64_t raw = (int64_t)n_frames * depthmetrics_workgroups(n_pixels) * DEPTHMETRICS_ROW * (int64_t)sizeof(double);
  return (raw + 255) / 256 * 256;
}

}  // namespace

extern "C" {

const char* depthmetrics_last_error(void) { return g_err; }
int depthmetrics_abi_version(void) { return DEPTHMETRICS_ABI_VERSION; }

int64_t depthmetrics_workspace_bytes(int n_frames, int64_t n_pixels) {
  if (sizes_ok(__func__, n_frames, n_pixels) != DEPTHMETRICS_OK) return -1;
  return ws_bytes(n_frames, n_pixels);
}

int depthmetrics_frames(void* stream, int n_frames, int64_t n_pixels, const float* pred, const float* gt, double scale,
                        void* workspace, double* out, float* err_map) {
  const int rc = sizes_ok(__func__, n_frames, n_pixels);
  if (rc != DEPTHMETRICS_OK) return rc;
  const float s = (float)scale;
  if (!isfinite(scale) || !(scale > 0.0) || !isfinite(s) || !(s > 0.f))
    return fail(DEPTHMETRICS_ERR_ARG, "%s: scale = %g: expected a finite positive number that is one in float32 too", __func__, scale);
  REQUIRE(pred && gt && workspace && out, "non-null pred, gt, workspace, out");
  REQUIRE(((uintptr_t)pred & 3) == 0 && ((uintptr_t)gt & 3) == 0 && ((uintptr_t)err_map & 3) == 0,
          "pred, gt and err_map aligned to 4 bytes");
  REQUIRE(((uintptr_t)workspace & 255) == 0 && ((uintptr_t)out & 7) == 0, "workspace aligned to 256 bytes, out to 8");
  const hipStream_t st = (hipStream_t)stream;
  const int nwg = depthmetrics_workgroups(n_pixels);
  launch_depthmetrics_reduce(st, n_frames, n_pixels, nwg, pred, gt, s, (double*)workspace, err_map);
  launch_depthmetrics_finish(st, n_frames, nwg, (const double*)workspace, out);
  return check_launch("depthmetrics_frames");
}

}  // extern "C"

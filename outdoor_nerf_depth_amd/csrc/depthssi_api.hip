// extern "C" surface of libdepthssi_hip.so (include/depthssi_hip.h): argument checks (no HIP call, so a host without a GPU gets
// the same errors), the workspace layout and the two launches.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include "../../include/depthssi_hip.h"
#define API_OK DEPTHSSI_OK
#define API_ERR_HIP DEPTHSSI_ERR_HIP
#define API_ERR_ARG DEPTHSSI_ERR_ARG
#include "api_common.h"
#include "depthssi_kernels.h"

namespace {

int sizes_ok(const char* fn, int n_levels, int n_groups) {
  if (n_levels < 1 || n_levels > DEPTHSSI_MAX_LEVELS)
    return fail(DEPTHSSI_ERR_ARG, "%s: n_levels = %d, expected 1 .. %d", fn, n_levels, DEPTHSSI_MAX_LEVELS);
  if (n_groups < 1 || n_groups > DEPTHSSI_MAX_GROUPS)
    return fail(DEPTHSSI_ERR_ARG, "%s: n_groups = %d, expected 1 .. %d", fn, n_groups, DEPTHSSI_MAX_GROUPS);
  return DEPTHSSI_OK;
}

int64_t ws_bytes(int n_levels, int n_groups) {
  const int64_t raw = depthssi_ws_doubles(n_levels, n_groups) * (int64_t)sizeof(double);
  return (raw + 255) / 256 * 256;
}

}  // namespace

extern "C" {

const char* depthssi_last_error(void) { return g_err; }
int depthssi_abi_version(void) { return DEPTHSSI_ABI_VERSION; }

int64_t depthssi_workspace_bytes(int n_levels, int n_groups) {
  if (sizes_ok(__func__, n_levels, n_groups) != DEPTHSSI_OK) return -1;
  return ws_bytes(n_levels, n_groups);
}

int depthssi_levels(void* stream, int n, int n_levels, const float* const* d, const float* p, const int32_t* g, int g_stride,
                    int n_groups, int min_rays, int norm, const float* scale, float* const* grads, void* workspace, float* values,
                    float* fit, float* stats, float* fold_total, float* fold_last, float* fold_others, float* fold_n_sup) {
  const int rc = sizes_ok(__func__, n_levels, n_groups);
  if (rc != DEPTHSSI_OK) return rc;
  if (n < 1 || n > DEPTHSSI_MAX_RAYS)
    return fail(DEPTHSSI_ERR_ARG, "%s: n = %d, expected 1 .. 2^20 rays (the loss is built for training batches)", __func__, n);
  if (min_rays < 1) return fail(DEPTHSSI_ERR_ARG, "%s: min_rays = %d, expected at least 1", __func__, min_rays);
  if (norm != DEPTHSSI_NORM_ALL && norm != DEPTHSSI_NORM_SUPERVISED)
    return fail(DEPTHSSI_ERR_ARG, "%s: norm = %d, expected 0 (all rays) or 1 (supervised rays)", __func__, norm);
  REQUIRE(d && p && scale && workspace && values && fit && stats, "non-null d, p, scale, workspace, values, fit, stats");
  if (g == nullptr && n_groups != 1)
    return fail(DEPTHSSI_ERR_ARG, "%s: n_groups = %d without group ids (g is null): one group", __func__, n_groups);
  if (g != nullptr && g_stride < 1) return fail(DEPTHSSI_ERR_ARG, "%s: g_stride = %d, expected at least 1", __func__, g_stride);
  REQUIRE(aligned4(p, g), "p and g aligned to 4 bytes");
  REQUIRE(((uintptr_t)workspace & 255) == 0, "workspace aligned to 256 bytes");
  REQUIRE(aligned4(values, fit, stats, fold_total, fold_last, fold_others, fold_n_sup),
          "values, fit, stats and the folds aligned to 4 bytes");
  DepthSsiArgs a{};
  for (int l = 0; l < n_levels; ++l) {
    if (d[l] == nullptr || ((uintptr_t)d[l] & 3) != 0)
      return fail(DEPTHSSI_ERR_ARG, "%s: d[%d] is null or not aligned to 4 bytes", __func__, l);
    if (!isfinite(scale[l])) return fail(DEPTHSSI_ERR_ARG, "%s: scale[%d] = %g is not finite", __func__, l, (double)scale[l]);
    float* gl = grads ? grads[l] : nullptr;
    if (((uintptr_t)gl & 3) != 0) return fail(DEPTHSSI_ERR_ARG, "%s: grads[%d] is not aligned to 4 bytes", __func__, l);
    for (int m = 0; gl != nullptr && m < l; ++m)             // a gradient entry has one owner: two levels cannot share a buffer
      if (a.grads[m] == gl) return fail(DEPTHSSI_ERR_ARG, "%s: grads[%d] and grads[%d] are the same buffer", __func__, m, l);
    a.d[l] = d[l]; a.grads[l] = gl; a.scale[l] = scale[l];
  }
  a.n = n; a.n_levels = n_levels; a.n_groups = n_groups; a.min_rays = min_rays; a.norm = norm; a.g_stride = g ? g_stride : 1;
  a.p = p; a.g = g; a.ws = (double*)workspace; a.values = values; a.fit = fit; a.stats = stats;
  a.folds = {fold_total, fold_last, fold_others, fold_n_sup};
  const hipStream_t st = (hipStream_t)stream;
  launch_depthssi_groups(st, a);
  launch_depthssi_finish(st, a);
  return check_launch("depthssi_levels");
}

}  // extern "C"

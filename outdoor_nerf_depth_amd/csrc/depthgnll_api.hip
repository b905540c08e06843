// extern "C" surface of libdepthgnll_hip.so (include/depthgnll_hip.h): argument checks (no HIP call, so a host without a GPU gets
// the same errors), the workspace layout and the two launches.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include "../../include/depthgnll_hip.h"
#define API_OK DEPTHGNLL_OK
#define API_ERR_HIP DEPTHGNLL_ERR_HIP
#define API_ERR_ARG DEPTHGNLL_ERR_ARG
#include "api_common.h"
#include "depthgnll_kernels.h"

namespace {

int sizes_ok(const char* fn, int n_levels, int n) {
  if (n_levels < 1 || n_levels > DEPTHGNLL_MAX_LEVELS)
    return fail(DEPTHGNLL_ERR_ARG, "%s: n_levels = %d, expected 1 .. %d", fn, n_levels, DEPTHGNLL_MAX_LEVELS);
  if (n < 1 || n > DEPTHGNLL_MAX_RAYS)
    return fail(DEPTHGNLL_ERR_ARG, "%s: n = %d, expected 1 .. 2^20 rays (the loss is built for training batches)", fn, n);
  return DEPTHGNLL_OK;
}

int64_t ws_bytes(int n_levels, int n) { return (depthgnll_ws_bytes(n_levels, n) + 255) / 256 * 256; }

bool misaligned(const void* ptr) { return !aligned4(ptr); }

}  // namespace

extern "C" {

const char* depthgnll_last_error(void) { return g_err; }
int depthgnll_abi_version(void) { return DEPTHGNLL_ABI_VERSION; }

int64_t depthgnll_workspace_bytes(int n_levels, int n) {
  if (sizes_ok(__func__, n_levels, n) != DEPTHGNLL_OK) return -1;
  return ws_bytes(n_levels, n);
}

int depthgnll_levels(void* stream, int n, int n_levels, const int* n_samples, int x_is_edges, const float* const* w,
                     const float* const* x, const float* const* d, const float* p, const float* sigma, const float* limit,
                     const float* scale, float* const* g_w, float* const* g_d, void* workspace, float* values, float* stats,
                     float* fold_total, float* fold_last, float* fold_others, float* fold_n_sup) {
  const int rc = sizes_ok(__func__, n_levels, n);
  if (rc != DEPTHGNLL_OK) return rc;
  if (x_is_edges != 0 && x_is_edges != 1)
    return fail(DEPTHGNLL_ERR_ARG, "%s: x_is_edges = %d, expected 0 (sample positions) or 1 (interval edges)", __func__, x_is_edges);
  REQUIRE(n_samples && w && x && d && p && sigma && workspace && values && stats,
          "non-null n_samples, w, x, d, p, sigma, workspace, values, stats");
  REQUIRE(aligned4(p, sigma, limit), "p, sigma and limit aligned to 4 bytes");
  REQUIRE(((uintptr_t)workspace & 255) == 0, "workspace aligned to 256 bytes");
  REQUIRE(aligned4(values, stats, fold_total, fold_last, fold_others, fold_n_sup),
          "values, stats and the folds aligned to 4 bytes");
  DepthGnllArgs a{};
  for (int l = 0; l < n_levels; ++l) {
    if (n_samples[l] < 1 || n_samples[l] > DEPTHGNLL_MAX_SAMPLES)
      return fail(DEPTHGNLL_ERR_ARG, "%s: n_samples[%d] = %d, expected 1 .. %d", __func__, l, n_samples[l], DEPTHGNLL_MAX_SAMPLES);
    if (w[l] == nullptr || misaligned(w[l])) return fail(DEPTHGNLL_ERR_ARG, "%s: w[%d] is null or not aligned to 4 bytes", __func__, l);
    if (x[l] == nullptr || misaligned(x[l])) return fail(DEPTHGNLL_ERR_ARG, "%s: x[%d] is null or not aligned to 4 bytes", __func__, l);
    if (d[l] == nullptr || misaligned(d[l])) return fail(DEPTHGNLL_ERR_ARG, "%s: d[%d] is null or not aligned to 4 bytes", __func__, l);
    const float sc = scale ? scale[l] : 1.f;
    if (!isfinite(sc)) return fail(DEPTHGNLL_ERR_ARG, "%s: scale[%d] = %g is not finite", __func__, l, (double)sc);
    float* gw = g_w ? g_w[l] : nullptr;
    float* gd = g_d ? g_d[l] : nullptr;
    if (misaligned(gw)) return fail(DEPTHGNLL_ERR_ARG, "%s: g_w[%d] is not aligned to 4 bytes", __func__, l);
    if (misaligned(gd)) return fail(DEPTHGNLL_ERR_ARG, "%s: g_d[%d] is not aligned to 4 bytes", __func__, l);
    for (int m = 0; m < l; ++m) {                            // a gradient entry has one owner: two levels cannot share a buffer
      if (gw != nullptr && a.g_w[m] == gw) return fail(DEPTHGNLL_ERR_ARG, "%s: g_w[%d] and g_w[%d] are the same buffer", __func__, m, l);
      if (gd != nullptr && a.g_d[m] == gd) return fail(DEPTHGNLL_ERR_ARG, "%s: g_d[%d] and g_d[%d] are the same buffer", __func__, m, l);
    }
    a.S[l] = n_samples[l]; a.w[l] = w[l]; a.x[l] = x[l]; a.d[l] = d[l]; a.g_w[l] = gw; a.g_d[l] = gd; a.scale[l] = sc;
  }
  a.n = n; a.n_levels = n_levels; a.edges = x_is_edges; a.p = p; a.sigma = sigma; a.limit = limit;
  a.ws_loss = (double*)workspace;
  a.ws_class = (int32_t*)(a.ws_loss + (size_t)n_levels * n);
  a.values = values; a.stats = stats;
  a.folds = {fold_total, fold_last, fold_others, fold_n_sup};
  const hipStream_t st = (hipStream_t)stream;
  launch_depthgnll_rays(st, a);
  launch_depthgnll_finish(st, a);
  return check_launch("depthgnll_levels");
}

}  // extern "C"

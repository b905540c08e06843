// extern "C" surface of libraylos_hip.so (include/raylos_hip.h): argument checks (no HIP call, so a host without a GPU gets the
// same errors), the workspace layout and the two launches.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include "../../include/raylos_hip.h"
#define API_OK RAYLOS_OK
#define API_ERR_HIP RAYLOS_ERR_HIP
#define API_ERR_ARG RAYLOS_ERR_ARG
#include "api_common.h"
#include "raylos_kernels.h"

namespace {

int rays_ok(const char* fn, int n) {
  if (n < 1 || n > RAYLOS_MAX_RAYS)
    return fail(RAYLOS_ERR_ARG, "%s: n = %d, expected 1 .. 2^20 rays (the line-of-sight term is built for training batches)", fn, n);
  return RAYLOS_OK;
}

int64_t ws_bytes(int n) { return (raylos_ws_bytes(n) + 255) / 256 * 256; }

}  // namespace

extern "C" {

const char* raylos_last_error(void) { return g_err; }
int raylos_abi_version(void) { return RAYLOS_ABI_VERSION; }

int64_t raylos_workspace_bytes(int n) {
  if (rays_ok(__func__, n) != RAYLOS_OK) return -1;
  return ws_bytes(n);
}

int raylos_level(void* stream, int n, int S, const float* w, const float* z, const float* hi, const float* p,
                 const float* sigma, double lambda, float* g_w, void* workspace, float* values, float* stats,
                 float* fold_total) {
  int rc = rays_ok(__func__, n);
  if (rc != RAYLOS_OK) return rc;
  if (S < 1 || S > RAYLOS_MAX_SAMPLES) return fail(RAYLOS_ERR_ARG, "%s: S = %d, expected 1 .. %d samples per ray", __func__, S, RAYLOS_MAX_SAMPLES);
  if (!isfinite(lambda) || !(lambda > 0.0)) return fail(RAYLOS_ERR_ARG, "%s: lambda = %g, expected a finite positive value", __func__, lambda);
  REQUIRE(w && z && hi && p && sigma && workspace && values && stats, "non-null w, z, hi, p, sigma, workspace, values, stats");
  REQUIRE(aligned4(w, z, hi, p, sigma, g_w), "w, z, hi, p, sigma and g_w aligned to 4 bytes");
  REQUIRE(((uintptr_t)workspace & 255) == 0, "workspace aligned to 256 bytes");
  REQUIRE(aligned4(values, stats, fold_total), "values, stats and fold_total aligned to 4 bytes");
  const int64_t row_bytes = (int64_t)n * S * (int64_t)sizeof(float);
  REQUIRE(!overlap(g_w, row_bytes, w, row_bytes) && !overlap(g_w, row_bytes, z, row_bytes), "g_w apart from w and z (it is updated in place)");
  RayLosArgs a{};
  a.n = n; a.S = S; a.w = w; a.z = z; a.hi = hi; a.p = p; a.sigma = sigma;
  a.lambda = lambda; a.g_w = g_w;
  a.ws_los = (double*)workspace;
  a.ws_front = a.ws_los + n;
  a.ws_sup = (int32_t*)(a.ws_front + n);
  a.values = values; a.stats = stats; a.fold_total = fold_total;
  const hipStream_t st = (hipStream_t)stream;
  launch_raylos_rays(st, a);
  launch_raylos_finish(st, a);
  return check_launch("raylos_level");
}

}  // extern "C"

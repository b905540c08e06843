// extern "C" surface of librayreg_hip.so (include/rayreg_hip.h): argument checks (no HIP call, so a host without a GPU gets the
// same errors), the workspace layout and the two launches.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include "../../include/rayreg_hip.h"
#define API_OK RAYREG_OK
#define API_ERR_HIP RAYREG_ERR_HIP
#define API_ERR_ARG RAYREG_ERR_ARG
#include "api_common.h"
#include "rayreg_kernels.h"

namespace {

int rays_ok(const char* fn, int n) {
  if (n < 1 || n > RAYREG_MAX_RAYS)
    return fail(RAYREG_ERR_ARG, "%s: n = %d, expected 1 .. 2^20 rays (the regularisers are built for training batches)", fn, n);
  return RAYREG_OK;
}

int64_t ws_bytes(int n) { return (rayreg_ws_bytes(n) + 255) / 256 * 256; }

int lambda_ok(const char* fn, const char* name, double v) {
  if (!isfinite(v) || v < 0.0) return fail(RAYREG_ERR_ARG, "%s: %s = %g, expected a finite value that is not negative", fn, name, v);
  return RAYREG_OK;
}

}  // namespace

extern "C" {

const char* rayreg_last_error(void) { return g_err; }
int rayreg_abi_version(void) { return RAYREG_ABI_VERSION; }

int64_t rayreg_workspace_bytes(int n) {
  if (rays_ok(__func__, n) != RAYREG_OK) return -1;
  return ws_bytes(n);
}

int rayreg_level(void* stream, int n, int S, const float* w, const float* z, const float* lo, const float* hi, double lambda_dist,
                 double lambda_opac, float* g_w, void* workspace, float* values, float* stats, float* fold_total) {
  int rc = rays_ok(__func__, n);
  if (rc != RAYREG_OK) return rc;
  if (S < 1 || S > RAYREG_MAX_SAMPLES) return fail(RAYREG_ERR_ARG, "%s: S = %d, expected 1 .. %d samples per ray", __func__, S, RAYREG_MAX_SAMPLES);
  if ((rc = lambda_ok(__func__, "lambda_dist", lambda_dist)) != RAYREG_OK) return rc;
  if ((rc = lambda_ok(__func__, "lambda_opac", lambda_opac)) != RAYREG_OK) return rc;
  if (lambda_dist == 0.0 && lambda_opac == 0.0)
    return fail(RAYREG_ERR_ARG, "%s: lambda_dist and lambda_opac are both 0: there is nothing to compute", __func__);
  REQUIRE(w && z && lo && hi && workspace && values && stats, "non-null w, z, lo, hi, workspace, values, stats");
  REQUIRE(aligned4(w, z, lo, hi, g_w), "w, z, lo, hi and g_w aligned to 4 bytes");
  REQUIRE(((uintptr_t)workspace & 255) == 0, "workspace aligned to 256 bytes");
  REQUIRE(aligned4(values, stats, fold_total), "values, stats and fold_total aligned to 4 bytes");
  const int64_t row_bytes = (int64_t)n * S * (int64_t)sizeof(float);
  REQUIRE(!overlap(g_w, row_bytes, w, row_bytes) && !overlap(g_w, row_bytes, z, row_bytes), "g_w apart from w and z (it is updated in place)");
  RayRegArgs a{};
  a.n = n; a.S = S; a.w = w; a.z = z; a.lo = lo; a.hi = hi;
  a.lambda_dist = lambda_dist; a.lambda_opac = lambda_opac; a.g_w = g_w;
  a.ws_dist = (double*)workspace;
  a.ws_opac = a.ws_dist + n;
  a.ws_valid = (int32_t*)(a.ws_opac + n);
  a.values = values; a.stats = stats; a.fold_total = fold_total;
  const hipStream_t st = (hipStream_t)stream;
  launch_rayreg_rays(st, a);
  launch_rayreg_finish(st, a);
  return check_launch("rayreg_level");
}

}  // extern "C"

// extern "C" surface of libdepthguide_hip.so (include/depthguide_hip.h): argument checks (no HIP call, so a host without a GPU gets
// the same errors) and the one launch.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include "../../include/depthguide_hip.h"
#define API_OK DEPTHGUIDE_OK
#define API_ERR_HIP DEPTHGUIDE_ERR_HIP
#define API_ERR_ARG DEPTHGUIDE_ERR_ARG
#include "api_common.h"
#include "depthguide_kernels.h"

extern "C" {

const char* depthguide_last_error(void) { return g_err; }
int depthguide_abi_version(void) { return DEPTHGUIDE_ABI_VERSION; }

int depthguide_merge(void* stream, int n, int S_prev, int S_in, int G, const float* zp, const float* wp, const float* zin,
                     const float* lo, const float* hi, const float* prior, const float* prior_std, double std_const, double min_std,
                     const double* table, const float* v, int use_rng, uint64_t seed, uint64_t step, float* z_merged, int32_t* mode,
                     float* guide) {
  if (n < 1 || n > DEPTHGUIDE_MAX_RAYS) return fail(DEPTHGUIDE_ERR_ARG, "%s: n = %d, expected 1 .. 2^20 rays", __func__, n);
  if (S_prev < 1 || S_prev > DEPTHGUIDE_MAX_PREV)
    return fail(DEPTHGUIDE_ERR_ARG, "%s: S_prev = %d, expected 1 .. %d samples of the previous level", __func__, S_prev, DEPTHGUIDE_MAX_PREV);
  if (S_in < 1 || G < 1 || (int64_t)S_in + G > DEPTHGUIDE_MAX_MERGED)
    return fail(DEPTHGUIDE_ERR_ARG, "%s: S_in = %d, G = %d, expected at least 1 each and S_in + G <= %d", __func__, S_in, G, DEPTHGUIDE_MAX_MERGED);
  if (!isfinite(min_std) || min_std < 0.0)
    return fail(DEPTHGUIDE_ERR_ARG, "%s: min_std = %g, expected a finite value that is not negative", __func__, min_std);
  REQUIRE(zp && wp && zin && lo && hi && table && z_merged && mode, "non-null zp, wp, zin, lo, hi, table, z_merged, mode");
  REQUIRE(!(use_rng && v), "either use_rng or v, not both");
  REQUIRE(aligned4(zp, wp, zin, lo, hi, prior, prior_std), "zp, wp, zin, lo, hi, prior and prior_std aligned to 4 bytes");
  REQUIRE(aligned4(v, z_merged, mode, guide), "v, z_merged, mode and guide aligned to 4 bytes");
  REQUIRE(((uintptr_t)table & 7) == 0, "table aligned to 8 bytes");
  const int64_t in_bytes = (int64_t)n * S_in * (int64_t)sizeof(float), out_bytes = (int64_t)n * (S_in + G) * (int64_t)sizeof(float);
  REQUIRE(!overlap(z_merged, out_bytes, zin, in_bytes), "z_merged apart from zin");
  DepthGuideArgs a{};
  a.n = n; a.S_prev = S_prev; a.S_in = S_in; a.G = G;
  a.zp = zp; a.wp = wp; a.zin = zin; a.lo = lo; a.hi = hi; a.prior = prior; a.prior_std = prior_std;
  a.std_const = std_const; a.min_std = min_std; a.table = table; a.v = v;
  a.rng = nerfpp::make_rng_key(seed, step, use_rng != 0);
  a.z_merged = z_merged; a.mode = mode; a.guide = guide;
  launch_depthguide_merge((hipStream_t)stream, a);
  return check_launch("depthguide_merge");
}

}  // extern "C"

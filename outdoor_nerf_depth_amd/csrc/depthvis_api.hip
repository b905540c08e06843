// extern "C" surface of libdepthvis_hip.so (include/depthvis_hip.h): argument checks (no HIP call, so a host without a GPU
// gets the same errors), the workspace layout and the launch sequences.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include "../../include/depthvis_hip.h"
#define API_OK DEPTHVIS_OK
#define API_ERR_HIP DEPTHVIS_ERR_HIP
#define API_ERR_ARG DEPTHVIS_ERR_ARG
#include "api_common.h"
#include "depthvis_kernels.h"

namespace {

int frames_ok(const char* fn, int n_frames) {
  if (n_frames < 1 || n_frames > 65535) return fail(DEPTHVIS_ERR_ARG, "%s: n_frames = %d, expected 1 .. 65535", fn, n_frames);
  return DEPTHVIS_OK;
}

int values_ok(const char* fn, int n_frames, int64_t n) {
  if (frames_ok(fn, n_frames) != DEPTHVIS_OK) return DEPTHVIS_ERR_ARG;
  if (n < 1) return fail(DEPTHVIS_ERR_ARG, "%s: n = %lld: a frame has at least one value", fn, (long long)n);
  if (n > DEPTHVIS_MAX_N)
    return fail(DEPTHVIS_ERR_ARG, "%s: n = %lld exceeds 2^22 values per frame (the index takes 24 bits of the select's key)", fn,
                (long long)n);
  return DEPTHVIS_OK;
}

int pixels_ok(const char* fn, int n_frames, int64_t H, int64_t W) {
  if (frames_ok(fn, n_frames) != DEPTHVIS_OK) return DEPTHVIS_ERR_ARG;
  if (H < 1 || W < 1) return fail(DEPTHVIS_ERR_ARG, "%s: a %lld x %lld image has no pixel (H * W >= 1)", fn, (long long)H, (long long)W);
  if (H > DEPTHVIS_MAX_PIXELS || W > DEPTHVIS_MAX_PIXELS || H * W > DEPTHVIS_MAX_PIXELS)
    return fail(DEPTHVIS_ERR_ARG, "%s: a %lld x %lld image exceeds 2^28 pixels", fn, (long long)H, (long long)W);
  return DEPTHVIS_OK;
}

int64_t align_up(int64_t v, int64_t a) { return (v + a - 1) / a * a; }

// bytes: state [F, MAX_PS] | hist [F, nwg, MAX_PS, 256] float64 | pred [F, nwg, MAX_PS] uint64 (minmax: keys [F, nwg, 3] uint32 there)
struct WsLayout { int nwg; int64_t state, hist, pred, total; };
WsLayout ws_layout(int n_frames, int64_t n) {
  WsLayout L;
  L.nwg = depthvis_workgroups(n);
  L.state = 0;
  L.hist = L.state + (int64_t)n_frames * DEPTHVIS_MAX_PS * (int64_t)sizeof(DepthvisState);
  L.pred = L.hist + (int64_t)n_frames * L.nwg * DEPTHVIS_MAX_PS * DEPTHVIS_BLOCK * 8;
  L.total = align_up(L.pred + (int64_t)n_frames * L.nwg * DEPTHVIS_MAX_PS * 8, 256);
  return L;
}

}  // namespace

extern "C" {

const char* depthvis_last_error(void) { return g_err; }
int depthvis_abi_version(void) { return DEPTHVIS_ABI_VERSION; }

int64_t depthvis_workspace_bytes(int n_frames, int64_t n) {
  if (values_ok(__func__, n_frames, n) != DEPTHVIS_OK) return -1;
  return ws_layout(n_frames, n).total;
}

int depthvis_percentiles(void* stream, int n_frames, int64_t n, const float* value, const float* weight, int n_ps,
                         const double* ps, void* workspace, double* out) {
  const int rc = values_ok(__func__, n_frames, n);
  if (rc != DEPTHVIS_OK) return rc;
  if (n_ps < 1 || n_ps > DEPTHVIS_MAX_PS) return fail(DEPTHVIS_ERR_ARG, "%s: n_ps = %d, expected 1 .. %d", __func__, n_ps, DEPTHVIS_MAX_PS);
  REQUIRE(value && weight && ps && workspace && out, "non-null value, weight, ps, workspace, out");
  REQUIRE(((uintptr_t)value & 3) == 0 && ((uintptr_t)weight & 3) == 0, "value and weight aligned to 4 bytes");
  REQUIRE(((uintptr_t)workspace & 255) == 0 && ((uintptr_t)out & 7) == 0, "workspace aligned to 256 bytes, out to 8");
  const hipStream_t st = (hipStream_t)stream;
  const WsLayout L = ws_layout(n_frames, n);
  char* ws = (char*)workspace;
  DepthvisState* state = (DepthvisState*)(ws + L.state);
  double* hist = (double*)(ws + L.hist);
  uint64_t* pred = (uint64_t*)(ws + L.pred);
  DepthvisPs p;
  for (int i = 0; i < DEPTHVIS_MAX_PS; ++i) p.p[i] = i < n_ps ? ps[i] : 0.0;
  for (int pass = 0; pass < DEPTHVIS_PASSES; ++pass) {
    launch_depthvis_hist(st, n_frames, n, L.nwg, n_ps, pass, value, weight, state, hist);
    launch_depthvis_select(st, n_frames, L.nwg, n_ps, pass, p, hist, state);
  }
  launch_depthvis_pred(st, n_frames, n, L.nwg, n_ps, value, state, pred);
  launch_depthvis_interp(st, n_frames, n, L.nwg, n_ps, value, state, pred, out);
  return check_launch("depthvis_percentiles");
}

int depthvis_minmax(void* stream, int n_frames, int64_t n, const float* value, void* workspace, float* out) {
  const int rc = values_ok(__func__, n_frames, n);
  if (rc != DEPTHVIS_OK) return rc;
  REQUIRE(value && workspace && out, "non-null value, workspace, out");
  REQUIRE(((uintptr_t)value & 3) == 0 && ((uintptr_t)out & 3) == 0, "value and out aligned to 4 bytes");
  REQUIRE(((uintptr_t)workspace & 255) == 0, "workspace aligned to 256 bytes");
  const WsLayout L = ws_layout(n_frames, n);
  launch_depthvis_minmax((hipStream_t)stream, n_frames, n, L.nwg, value, (uint32_t*)((char*)workspace + L.pred), out);
  return check_launch("depthvis_minmax");
}

int depthvis_prepare(void* stream, int n_frames, int64_t n_pixels, const float* acc, const float* distance_mean,
                     const float* distance_median, const float* p5, const float* p95, float* acc_eff, float* triplet_value,
                     float* triplet_weight) {
  const int rc = pixels_ok(__func__, n_frames, n_pixels, 1);
  if (rc != DEPTHVIS_OK) return rc;
  REQUIRE(acc && distance_mean && acc_eff, "non-null acc, distance_mean, acc_eff");
  REQUIRE((triplet_value == nullptr) == (triplet_weight == nullptr), "triplet_value and triplet_weight both or neither");
  REQUIRE(triplet_value == nullptr || (distance_median && p5 && p95), "non-null distance_median, p5, p95 for the triplet");
  launch_depthvis_prepare((hipStream_t)stream, n_frames, n_pixels, acc, distance_mean, distance_median, p5, p95, acc_eff,
                          triplet_value, triplet_weight);
  return check_launch("depthvis_prepare");
}

int depthvis_colorize(void* stream, int n_frames, int H, int W, int mode, int cmap, int curve, const float* value,
                      const float* acc, const float* origins, const float* directions, const double* lohi,
                      const float* minmax, uint8_t* out) {
  const int rc = pixels_ok(__func__, n_frames, H, W);
  if (rc != DEPTHVIS_OK) return rc;
  if (mode < DEPTHVIS_MODE_CMAP || mode > DEPTHVIS_MODE_COORDS_MOD) return fail(DEPTHVIS_ERR_ARG, "%s: unknown mode %d", __func__, mode);
  const bool table = mode == DEPTHVIS_MODE_CMAP || mode == DEPTHVIS_MODE_MINMAX;
  const bool curved = mode == DEPTHVIS_MODE_CMAP || mode == DEPTHVIS_MODE_CMAP3;
  if (table && cmap != DEPTHVIS_CMAP_TURBO && cmap != DEPTHVIS_CMAP_JET) return fail(DEPTHVIS_ERR_ARG, "%s: unknown colour table %d", __func__, cmap);
  if (curved && (curve < DEPTHVIS_CURVE_IDENTITY || curve > DEPTHVIS_CURVE_LOG)) return fail(DEPTHVIS_ERR_ARG, "%s: unknown curve %d", __func__, curve);
  REQUIRE(value && out, "non-null value, out");
  REQUIRE(mode == DEPTHVIS_MODE_MINMAX || acc, "non-null acc for a matted mode");
  REQUIRE(!curved || (lohi && ((uintptr_t)lohi & 7) == 0), "non-null lohi aligned to 8 bytes for a cmap mode");
  REQUIRE(mode != DEPTHVIS_MODE_MINMAX || minmax, "non-null minmax for the minmax mode");
  REQUIRE(mode != DEPTHVIS_MODE_COORDS_MOD || (origins && directions), "non-null origins, directions for coords_mod");
  launch_depthvis_colorize((hipStream_t)stream, n_frames, H, W, mode, table ? cmap : 0, curve, value, acc, origins, directions, lohi,
                           minmax, out);
  return check_launch("depthvis_colorize");
}

}  // extern "C"

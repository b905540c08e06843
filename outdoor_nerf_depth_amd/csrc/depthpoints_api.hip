// extern "C" surface of libdepthpoints_hip.so (include/depthpoints_hip.h): argument checks (no HIP call, so a host without a GPU gets
// the same errors), the workspace layout and the launches.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include "../../include/depthpoints_hip.h"
#define API_OK DEPTHPOINTS_OK
#define API_ERR_HIP DEPTHPOINTS_ERR_HIP
#define API_ERR_ARG DEPTHPOINTS_ERR_ARG
#include "api_common.h"
#include "depthpoints_kernels.h"

namespace {

int64_t up256(int64_t n) { return (n + 255) / 256 * 256; }
// the workspace: zbuf [F, H, W] uint64, then (each aligned to 256) partial [F, tiles, 2] int32 and counts [F, 2] uint64
int64_t zbuf_bytes(int n_frames, int height, int width) { return up256((int64_t)n_frames * height * width * 8); }
int64_t partial_bytes(int n_frames, int height, int width) {
  return up256((int64_t)n_frames * depthpoints_tiles(height, width) * 2 * (int64_t)sizeof(int32_t));
}
int64_t counts_bytes(int n_frames) { return up256((int64_t)n_frames * 2 * 8); }

}  // namespace

extern "C" {

const char* depthpoints_last_error(void) { return g_err; }
int depthpoints_abi_version(void) { return DEPTHPOINTS_ABI_VERSION; }

int64_t depthpoints_workspace_bytes(int n_frames, int height, int width) {
  if (frames_ok(__func__, n_frames, height, width, DEPTHPOINTS_MAX_FRAMES, DEPTHPOINTS_MAX_PIXELS) != DEPTHPOINTS_OK) return -1;
  return zbuf_bytes(n_frames, height, width) + partial_bytes(n_frames, height, width) + counts_bytes(n_frames);
}

int depthpoints_splat(void* stream, int n_frames, int height, int width, const double* cams, int64_t n_points, const double* points,
                      int64_t n_obs, const int32_t* obs, double near, double far, int occl_radius, double occl_tol, double std_scale,
                      double std_floor, void* workspace, float* depth_out, float* std_out, int32_t* point, uint8_t* origin,
                      int64_t* rows) {
  const int rc = frames_ok(__func__, n_frames, height, width, DEPTHPOINTS_MAX_FRAMES, DEPTHPOINTS_MAX_PIXELS);
  if (rc != DEPTHPOINTS_OK) return rc;
  if (n_points < 0 || n_points > DEPTHPOINTS_MAX_POINTS)
    return fail(DEPTHPOINTS_ERR_ARG, "%s: n_points = %lld, expected 0 .. 2^31 - 1", __func__, (long long)n_points);
  if (n_obs < 0 || n_obs > DEPTHPOINTS_MAX_OBS)
    return fail(DEPTHPOINTS_ERR_ARG, "%s: n_obs = %lld, expected 0 .. 2^40", __func__, (long long)n_obs);
  if (!(isfinite(near) && isfinite(far) && near > 0.0 && near < far))
    return fail(DEPTHPOINTS_ERR_ARG, "%s: near = %g, far = %g: expected finite numbers with 0 < near < far", __func__, near, far);
  if (occl_radius < 0 || occl_radius > DEPTHPOINTS_MAX_RADIUS)
    return fail(DEPTHPOINTS_ERR_ARG, "%s: occl_radius = %d, expected 0 .. %d", __func__, occl_radius, DEPTHPOINTS_MAX_RADIUS);
  if (!isfinite(occl_tol) || occl_tol < 0.0)
    return fail(DEPTHPOINTS_ERR_ARG, "%s: occl_tol = %g: expected a finite number >= 0", __func__, occl_tol);
  if (!isfinite(std_scale) || !(std_scale > 0.0))
    return fail(DEPTHPOINTS_ERR_ARG, "%s: std_scale = %g: expected a finite number > 0", __func__, std_scale);
  if (!isfinite(std_floor) || std_floor < 0.0)
    return fail(DEPTHPOINTS_ERR_ARG, "%s: std_floor = %g: expected a finite number >= 0", __func__, std_floor);
  REQUIRE(cams && depth_out && workspace, "non-null cams, depth_out, workspace");
  REQUIRE(points || n_points == 0, "non-null points when n_points > 0");
  REQUIRE(obs || n_obs == 0, "n_obs = 0 when obs is null (the `all` mode)");
  REQUIRE(aligned4(depth_out, std_out, point), "depth_out, std_out and point aligned to 4 bytes");
  REQUIRE(((uintptr_t)cams & 7) == 0 && ((uintptr_t)rows & 7) == 0 && ((uintptr_t)obs & 7) == 0, "cams, rows and obs aligned to 8 bytes");
  REQUIRE(((uintptr_t)points & 15) == 0, "points aligned to 16 bytes");
  REQUIRE(((uintptr_t)workspace & 255) == 0, "workspace aligned to 256 bytes");

  const hipStream_t st = (hipStream_t)stream;
  const int64_t n = (int64_t)n_frames * height * width;
  unsigned long long* zbuf = (unsigned long long*)workspace;
  int32_t* partial = rows ? (int32_t*)((char*)workspace + zbuf_bytes(n_frames, height, width)) : nullptr;
  unsigned long long* counts =
      rows ? (unsigned long long*)((char*)workspace + zbuf_bytes(n_frames, height, width) + partial_bytes(n_frames, height, width)) : nullptr;
  hipError_t e = hipMemsetAsync(zbuf, 0xff, (size_t)n * 8, st);              // every key empty (all ones)
  if (e != hipSuccess) return fail(DEPTHPOINTS_ERR_HIP, "%s: the fill of the z-buffer: %s", __func__, hipGetErrorString(e));
  if (counts) {
    e = hipMemsetAsync(counts, 0, (size_t)n_frames * 2 * 8, st);
    if (e != hipSuccess) return fail(DEPTHPOINTS_ERR_HIP, "%s: the fill of the counters: %s", __func__, hipGetErrorString(e));
  }
  const DepthPointsRange rg = {near, far};
  if (obs != nullptr) {
    for_chunks((n_obs + DEPTHPOINTS_BLOCK - 1) / DEPTHPOINTS_BLOCK, depthprior::MAX_GRID, [&](int64_t g0, int64_t n_wg) {
      launch_depthpoints_scatter_obs(st, n_frames, height, width, g0, n_wg, cams, n_points, points, n_obs, obs, rg, zbuf, counts);
    });
  } else {
    for_chunks((int64_t)n_frames * depthpoints_point_tiles(n_points), depthprior::MAX_GRID, [&](int64_t g0, int64_t n_wg) {
      launch_depthpoints_scatter_all(st, height, width, g0, n_wg, cams, n_points, points, rg, zbuf, counts);
    });
  }
  const int64_t tiles = depthpoints_tiles(height, width);
  for_chunks((int64_t)n_frames * tiles, depthprior::MAX_GRID, [&](int64_t g0, int64_t n_wg) {
    launch_depthpoints_resolve(st, height, width, g0, n_wg, cams, points, zbuf, occl_radius, 1.0 + occl_tol, std_scale, std_floor,
                               depth_out, std_out, point, origin, partial);
  });
  if (rows) launch_depthpoints_rows(st, n_frames, tiles, partial, counts, rows);
  return check_launch("depthpoints_splat");
}

}  // extern "C"

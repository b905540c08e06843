// extern "C" surface of libdepthacc_hip.so (include/depthacc_hip.h): argument checks (no HIP call, so a host without a GPU gets the
// same errors), the workspace layout and the launches.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include "../../include/depthacc_hip.h"
#define API_OK DEPTHACC_OK
#define API_ERR_HIP DEPTHACC_ERR_HIP
#define API_ERR_ARG DEPTHACC_ERR_ARG
#include "api_common.h"
#include "depthacc_kernels.h"

namespace {

// the workspace: zbuf [F, H, W] uint64, then (aligned to 256) partial [F, tiles, 4] int32
int64_t zbuf_bytes(int n_frames, int height, int width) {
  return ((int64_t)n_frames * height * width * 8 + 255) / 256 * 256;
}
int64_t ws_bytes(int n_frames, int height, int width) {
  const int64_t partial = (int64_t)n_frames * depthacc_tiles(height, width) * 4 * (int64_t)sizeof(int32_t);
  return zbuf_bytes(n_frames, height, width) + (partial + 255) / 256 * 256;
}

}  // namespace

extern "C" {

const char* depthacc_last_error(void) { return g_err; }
int depthacc_abi_version(void) { return DEPTHACC_ABI_VERSION; }

int64_t depthacc_workspace_bytes(int n_frames, int height, int width) {
  if (frames_ok(__func__, n_frames, height, width, DEPTHACC_MAX_FRAMES, DEPTHACC_MAX_PIXELS) != DEPTHACC_OK) return -1;
  return ws_bytes(n_frames, height, width);
}

int depthacc_accumulate(void* stream, int n_frames, int height, int width, int n_views, const float* depth, const double* cams,
                        const int32_t* nbr, int occl_radius, double occl_tol, void* workspace, float* depth_out, uint8_t* origin,
                        int32_t* src, int64_t* rows) {
  const int rc = frames_ok(__func__, n_frames, height, width, DEPTHACC_MAX_FRAMES, DEPTHACC_MAX_PIXELS);
  if (rc != DEPTHACC_OK) return rc;
  if (n_views < 0 || n_views > DEPTHACC_MAX_VIEWS)
    return fail(DEPTHACC_ERR_ARG, "%s: n_views = %d, expected 0 .. %d", __func__, n_views, DEPTHACC_MAX_VIEWS);
  if (occl_radius < 0 || occl_radius > DEPTHACC_MAX_RADIUS)
    return fail(DEPTHACC_ERR_ARG, "%s: occl_radius = %d, expected 0 .. %d", __func__, occl_radius, DEPTHACC_MAX_RADIUS);
  if (!isfinite(occl_tol) || occl_tol < 0.0)
    return fail(DEPTHACC_ERR_ARG, "%s: occl_tol = %g: expected a finite number >= 0", __func__, occl_tol);
  REQUIRE(depth && cams && depth_out && workspace, "non-null depth, cams, depth_out, workspace");
  REQUIRE(nbr || n_views == 0, "non-null nbr when n_views > 0");
  REQUIRE(aligned4(depth, depth_out, src, nbr), "depth, depth_out, src and nbr aligned to 4 bytes");
  REQUIRE(((uintptr_t)cams & 7) == 0 && ((uintptr_t)rows & 7) == 0, "cams and rows aligned to 8 bytes");
  REQUIRE(((uintptr_t)workspace & 255) == 0, "workspace aligned to 256 bytes");
  const int64_t n = (int64_t)n_frames * height * width;
  if (overlap(depth, 4 * n, depth_out, 4 * n))
    return fail(DEPTHACC_ERR_ARG, "%s: depth_out overlaps depth: the launches read depth throughout", __func__);
  if (overlap(depth, 4 * n, origin, n))
    return fail(DEPTHACC_ERR_ARG, "%s: origin overlaps depth: the launches read depth throughout", __func__);
  if (overlap(depth, 4 * n, src, 4 * n))
    return fail(DEPTHACC_ERR_ARG, "%s: src overlaps depth: the launches read depth throughout", __func__);
  if (overlap(depth, 4 * n, rows, 8ll * DEPTHACC_ROW * n_frames))
    return fail(DEPTHACC_ERR_ARG, "%s: rows overlaps depth: the launches read depth throughout", __func__);
  if (overlap(depth, 4 * n, workspace, ws_bytes(n_frames, height, width)))
    return fail(DEPTHACC_ERR_ARG, "%s: workspace overlaps depth: the launches read depth throughout", __func__);

  const hipStream_t st = (hipStream_t)stream;
  unsigned long long* zbuf = (unsigned long long*)workspace;
  int32_t* partial = rows ? (int32_t*)((char*)workspace + zbuf_bytes(n_frames, height, width)) : nullptr;
  const hipError_t e = hipMemsetAsync(zbuf, 0xff, (size_t)n * 8, st);      // every key empty (all ones)
  if (e != hipSuccess) return fail(DEPTHACC_ERR_HIP, "%s: the fill of the z-buffer: %s", __func__, hipGetErrorString(e));
  const int64_t scatter_wg = (int64_t)n_frames * n_views * depthacc_scatter_tiles(height, width);
  for_chunks(scatter_wg, depthprior::MAX_GRID, [&](int64_t g0, int64_t n_wg) {
    launch_depthacc_scatter(st, n_frames, height, width, n_views, g0, n_wg, depth, cams, nbr, zbuf);
  });
  const int64_t tiles = depthacc_tiles(height, width), resolve_wg = (int64_t)n_frames * tiles;
  for_chunks(resolve_wg, depthprior::MAX_GRID, [&](int64_t g0, int64_t n_wg) {
    launch_depthacc_resolve(st, height, width, g0, n_wg, depth, zbuf, occl_radius, 1.0 + occl_tol, depth_out, origin, src, partial);
  });
  if (rows) launch_depthacc_rows(st, n_frames, tiles, partial, rows);
  return check_launch("depthacc_accumulate");
}

}  // extern "C"

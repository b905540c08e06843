// extern "C" surface of libdepthcons_hip.so (include/depthcons_hip.h): argument checks (no HIP call, so a host without a GPU
// gets the same errors), the workspace layout and the launches.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include "../../include/depthcons_hip.h"
#define API_OK DEPTHCONS_OK
#define API_ERR_HIP DEPTHCONS_ERR_HIP
#define API_ERR_ARG DEPTHCONS_ERR_ARG
#include "api_common.h"
#include "depthcons_kernels.h"

namespace {

// bytes: partial [F, tiles, 4] int32
int64_t ws_bytes(int n_frames, int height, int width) {
  const int64_t raw = (int64_t)n_frames * depthcons_tiles(height, width) * 4 * (int64_t)sizeof(int32_t);
  return (raw + 255) / 256 * 256;
}

}  // namespace

extern "C" {

const char* depthcons_last_error(void) { return g_err; }
int depthcons_abi_version(void) { return DEPTHCONS_ABI_VERSION; }

int64_t depthcons_workspace_bytes(int n_frames, int height, int width) {
  if (frames_ok(__func__, n_frames, height, width, DEPTHCONS_MAX_FRAMES, DEPTHCONS_MAX_PIXELS) != DEPTHCONS_OK) return -1;
  return ws_bytes(n_frames, height, width);
}

int depthcons_check(void* stream, int n_frames, int height, int width, int n_views, const float* depth, const double* cams,
                    const int32_t* nbr, double pix_tol, double rel_tol, int min_views, int keep_unverified, double std_floor,
                    void* workspace, float* depth_out, float* std_out, uint8_t* counts, int64_t* rows) {
  const int rc = frames_ok(__func__, n_frames, height, width, DEPTHCONS_MAX_FRAMES, DEPTHCONS_MAX_PIXELS);
  if (rc != DEPTHCONS_OK) return rc;
  if (n_views < 0 || n_views > DEPTHCONS_MAX_VIEWS)
    return fail(DEPTHCONS_ERR_ARG, "%s: n_views = %d, expected 0 .. %d", __func__, n_views, DEPTHCONS_MAX_VIEWS);
  if (!isfinite(pix_tol) || pix_tol < 0.0) return fail(DEPTHCONS_ERR_ARG, "%s: pix_tol = %g: expected a finite number >= 0", __func__, pix_tol);
  if (!isfinite(rel_tol) || rel_tol < 0.0) return fail(DEPTHCONS_ERR_ARG, "%s: rel_tol = %g: expected a finite number >= 0", __func__, rel_tol);
  if (!isfinite(std_floor) || std_floor < 0.0)
    return fail(DEPTHCONS_ERR_ARG, "%s: std_floor = %g: expected a finite number >= 0", __func__, std_floor);
  if (min_views < 1) return fail(DEPTHCONS_ERR_ARG, "%s: min_views = %d: expected at least 1", __func__, min_views);
  if (keep_unverified != 0 && keep_unverified != 1)
    return fail(DEPTHCONS_ERR_ARG, "%s: keep_unverified = %d: expected 0 or 1", __func__, keep_unverified);
  REQUIRE(depth && cams && depth_out, "non-null depth, cams, depth_out");
  REQUIRE(nbr || n_views == 0, "non-null nbr when n_views > 0");
  REQUIRE(workspace || !rows, "non-null workspace when rows is given");
  REQUIRE(((uintptr_t)depth & 3) == 0 && ((uintptr_t)depth_out & 3) == 0 && ((uintptr_t)std_out & 3) == 0 && ((uintptr_t)nbr & 3) == 0,
          "depth, depth_out, std_out and nbr aligned to 4 bytes");
  REQUIRE(((uintptr_t)cams & 7) == 0 && ((uintptr_t)rows & 7) == 0, "cams and rows aligned to 8 bytes");
  REQUIRE(((uintptr_t)workspace & 255) == 0, "workspace aligned to 256 bytes");
  const int64_t n = (int64_t)n_frames * height * width;
  if (overlap(depth, 4 * n, depth_out, 4 * n))
    return fail(DEPTHCONS_ERR_ARG, "%s: depth_out overlaps depth: the neighbours of a pixel read depth", __func__);
  if (overlap(depth, 4 * n, std_out, 4 * n))
    return fail(DEPTHCONS_ERR_ARG, "%s: std_out overlaps depth: the neighbours of a pixel read depth", __func__);
  if (overlap(depth, 4 * n, counts, 2 * n))
    return fail(DEPTHCONS_ERR_ARG, "%s: counts overlaps depth: the neighbours of a pixel read depth", __func__);
  if (overlap(depth, 4 * n, rows, 8ll * DEPTHCONS_ROW * n_frames))
    return fail(DEPTHCONS_ERR_ARG, "%s: rows overlaps depth: the neighbours of a pixel read depth", __func__);
  if (overlap(depth, 4 * n, rows ? workspace : nullptr, ws_bytes(n_frames, height, width)))
    return fail(DEPTHCONS_ERR_ARG, "%s: workspace overlaps depth: the neighbours of a pixel read depth", __func__);

  const hipStream_t st = (hipStream_t)stream;
  DepthconsParams prm;
  prm.pix_tol2 = pix_tol * pix_tol;
  prm.rel_tol = rel_tol;
  prm.std_floor = std_floor;
  prm.min_views = min_views;
  prm.keep_unverified = keep_unverified;
  int32_t* partial = rows ? (int32_t*)workspace : nullptr;
  const int64_t tiles = depthcons_tiles(height, width);
  constexpr int64_t MAX_GRID = depthprior::MAX_GRID;
  if (tiles <= MAX_GRID) {                                   // whole frames per launch
    for_chunks(n_frames, MAX_GRID / tiles < 65535 ? MAX_GRID / tiles : 65535, [&](int64_t f0, int64_t n_launch_frames) {
      launch_depthcons_check(st, n_frames, height, width, n_views, (int)f0, (int)n_launch_frames, 0, tiles, depth, cams, nbr, prm,
                             depth_out, std_out, counts, partial);
    });
  } else {                                                   // a frame of more tiles than a launch takes
    for (int f0 = 0; f0 < n_frames; ++f0)
      for_chunks(tiles, MAX_GRID, [&](int64_t t0, int64_t n_tiles) {
        launch_depthcons_check(st, n_frames, height, width, n_views, f0, 1, t0, n_tiles, depth, cams, nbr, prm, depth_out, std_out,
                               counts, partial);
      });
  }
  if (rows) launch_depthcons_rows(st, n_frames, tiles, partial, rows);
  return check_launch("depthcons_check");
}

}  // extern "C"

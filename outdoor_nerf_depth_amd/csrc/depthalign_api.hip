// extern "C" surface of libdepthalign_hip.so (include/depthalign_hip.h): argument checks (no HIP call, so a host without a GPU gets
// the same errors), the workspace layout and the launches.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include "../../include/depthalign_hip.h"
#define API_OK DEPTHALIGN_OK
#define API_ERR_HIP DEPTHALIGN_ERR_HIP
#define API_ERR_ARG DEPTHALIGN_ERR_ARG
#include "api_common.h"
#include "depthalign_kernels.h"

namespace {

int64_t up256(int64_t n) { return (n + 255) / 256 * 256; }

// the workspace: ts [F, H * W] float64, then (each aligned to 256) xs [F, H * W] float32, counts [F, tiles] int32, offsets [F, tiles]
// int32, n_pairs [F] int32
int64_t ts_bytes(int n_frames, int height, int width) { return up256((int64_t)n_frames * height * width * 8); }
int64_t xs_bytes(int n_frames, int height, int width) { return up256((int64_t)n_frames * height * width * 4); }
int64_t counts_bytes(int n_frames, int height, int width) { return up256((int64_t)n_frames * depthalign_tiles(height, width) * 4); }
int64_t ws_bytes(int n_frames, int height, int width) {
  return ts_bytes(n_frames, height, width) + xs_bytes(n_frames, height, width) + 2 * counts_bytes(n_frames, height, width) + up256((int64_t)n_frames * 4);
}

}  // namespace

extern "C" {

const char* depthalign_last_error(void) { return g_err; }
int depthalign_abi_version(void) { return DEPTHALIGN_ABI_VERSION; }

int64_t depthalign_workspace_bytes(int n_frames, int height, int width) {
  if (frames_ok(__func__, n_frames, height, width, DEPTHALIGN_MAX_FRAMES, DEPTHALIGN_MAX_PIXELS) != DEPTHALIGN_OK) return -1;
  return ws_bytes(n_frames, height, width);
}

int depthalign_fit_apply(void* stream, int n_frames, int height, int width, const float* prior, const float* anchor, int space,
                         int iters, double c, int min_points, double max_depth, int keep_anchor, double std_floor, void* workspace,
                         float* depth_out, float* std_out, double* rows) {
  const int rc = frames_ok(__func__, n_frames, height, width, DEPTHALIGN_MAX_FRAMES, DEPTHALIGN_MAX_PIXELS);
  if (rc != DEPTHALIGN_OK) return rc;
  if (space != DEPTHALIGN_SPACE_DEPTH && space != DEPTHALIGN_SPACE_DISPARITY)
    return fail(DEPTHALIGN_ERR_ARG, "%s: space = %d, expected 0 (depth) or 1 (disparity)", __func__, space);
  if (iters < 0 || iters > DEPTHALIGN_MAX_ITERS)
    return fail(DEPTHALIGN_ERR_ARG, "%s: iters = %d, expected 0 .. %d", __func__, iters, DEPTHALIGN_MAX_ITERS);
  if (!isfinite(c) || !(c > 0.0)) return fail(DEPTHALIGN_ERR_ARG, "%s: c = %g: expected a finite number > 0", __func__, c);
  if (min_points < 2) return fail(DEPTHALIGN_ERR_ARG, "%s: min_points = %d, expected at least 2", __func__, min_points);
  if (!(max_depth > 0.0)) return fail(DEPTHALIGN_ERR_ARG, "%s: max_depth = %g: expected a number > 0 (+inf: no limit)", __func__, max_depth);
  if (keep_anchor != 0 && keep_anchor != 1) return fail(DEPTHALIGN_ERR_ARG, "%s: keep_anchor = %d, expected 0 or 1", __func__, keep_anchor);
  if (!isfinite(std_floor) || std_floor < 0.0)
    return fail(DEPTHALIGN_ERR_ARG, "%s: std_floor = %g: expected a finite number >= 0", __func__, std_floor);
  REQUIRE(prior && anchor && depth_out && rows && workspace, "non-null prior, anchor, depth_out, rows, workspace");
  REQUIRE(aligned4(prior, anchor, depth_out, std_out), "prior, anchor, depth_out and std_out aligned to 4 bytes");
  REQUIRE(((uintptr_t)rows & 7) == 0, "rows aligned to 8 bytes");
  REQUIRE(((uintptr_t)workspace & 255) == 0, "workspace aligned to 256 bytes");
  const int64_t n = (int64_t)n_frames * height * width, row_bytes = 8ll * DEPTHALIGN_ROW * n_frames;
  const struct { const void* p; int64_t bytes; const char* name; } in[2] = {{prior, 4 * n, "prior"}, {anchor, 4 * n, "anchor"}},
      out[4] = {{depth_out, 4 * n, "depth_out"}, {std_out, 4 * n, "std_out"}, {rows, row_bytes, "rows"},
                {workspace, ws_bytes(n_frames, height, width), "workspace"}};
  for (int o = 0; o < 4; ++o) {
    for (int i = 0; i < 2; ++i)
      if (overlap(in[i].p, in[i].bytes, out[o].p, out[o].bytes))
        return fail(DEPTHALIGN_ERR_ARG, "%s: %s overlaps %s: the launches read %s throughout", __func__, out[o].name, in[i].name, in[i].name);
    for (int q = 0; q < o; ++q)
      if (overlap(out[q].p, out[q].bytes, out[o].p, out[o].bytes))
        return fail(DEPTHALIGN_ERR_ARG, "%s: %s overlaps %s", __func__, out[o].name, out[q].name);
  }

  const hipStream_t st = (hipStream_t)stream;
  char* ws = (char*)workspace;
  double* ts = (double*)ws;
  float* xs = (float*)(ws + ts_bytes(n_frames, height, width));
  int32_t* counts = (int32_t*)((char*)xs + xs_bytes(n_frames, height, width));
  int32_t* offsets = (int32_t*)((char*)counts + counts_bytes(n_frames, height, width));
  int32_t* n_pairs = (int32_t*)((char*)offsets + counts_bytes(n_frames, height, width));
  const DepthAlignParams prm = {space, iters, min_points, keep_anchor, c, max_depth, std_floor};
  const int64_t tiles = depthalign_tiles(height, width), n_wg = (int64_t)n_frames * tiles;
  for (int pass = 0; pass < 2; ++pass) {                      // the tiles' counts; their scan; the pairs in pixel order
    for_chunks(n_wg, depthprior::MAX_GRID, [&](int64_t g0, int64_t n) {
      launch_depthalign_tiles(st, height, width, g0, n, space, prior, anchor, counts, offsets, pass == 0 ? nullptr : xs, ts);
    });
    if (pass == 0) launch_depthalign_scan(st, n_frames, tiles, counts, offsets, n_pairs);
  }
  launch_depthalign_fit(st, n_frames, (int64_t)height * width, xs, ts, n_pairs, prm, rows);
  launch_depthalign_apply(st, n_frames, (int64_t)height * width, prior, anchor, rows, prm, depth_out, std_out);
  return check_launch("depthalign_fit_apply");
}

}  // extern "C"

// extern "C" surface of libdepthmvs_hip.so (include/depthmvs_hip.h): argument checks (no HIP call, so a host without a GPU gets the
// same errors), the workspace layout and the launches.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include "../../include/depthmvs_hip.h"
#define API_OK DEPTHMVS_OK
#define API_ERR_HIP DEPTHMVS_ERR_HIP
#define API_ERR_ARG DEPTHMVS_ERR_ARG
#include "api_common.h"
#include "depthmvs_kernels.h"

namespace {

int64_t up256(int64_t n) { return (n + 255) / 256 * 256; }

// the workspace, every part aligned to 256: census [F, H, W] uint32; partial [F, tiles, 4] int32
struct Layout {
  int64_t census, partial, bytes;
};
Layout layout(int n_frames, int height, int width) {
  Layout l;
  l.census = 0;
  l.partial = up256(4 * (int64_t)n_frames * height * width);
  l.bytes = l.partial + up256((int64_t)n_frames * depthmvs_tiles(height, width) * 4 * (int64_t)sizeof(int32_t));
  return l;
}

}  // namespace

extern "C" {

const char* depthmvs_last_error(void) { return g_err; }
int depthmvs_abi_version(void) { return DEPTHMVS_ABI_VERSION; }

int64_t depthmvs_workspace_bytes(int n_frames, int height, int width) {
  if (frames_ok(__func__, n_frames, height, width, DEPTHMVS_MAX_FRAMES, DEPTHMVS_MAX_PIXELS) != DEPTHMVS_OK) return -1;
  return layout(n_frames, height, width).bytes;
}

int depthmvs_sweep(void* stream, int n_frames, int height, int width, int n_views, int n_planes, const uint8_t* rgb,
                   const double* cams, const int32_t* nbr, const double* inv_depth, int best_views, int agg_radius, double uniqueness,
                   double std_planes, void* workspace, float* depth, float* std, uint8_t* status, uint8_t* plane, uint16_t* cost,
                   uint16_t* second, uint32_t* census, int64_t* rows) {
  const int rc = frames_ok(__func__, n_frames, height, width, DEPTHMVS_MAX_FRAMES, DEPTHMVS_MAX_PIXELS);
  if (rc != DEPTHMVS_OK) return rc;
  if (n_views < 1 || n_views > DEPTHMVS_MAX_VIEWS)
    return fail(DEPTHMVS_ERR_ARG, "%s: n_views = %d, expected 1 .. %d", __func__, n_views, DEPTHMVS_MAX_VIEWS);
  if (n_planes < DEPTHMVS_MIN_PLANES || n_planes > DEPTHMVS_MAX_PLANES)
    return fail(DEPTHMVS_ERR_ARG, "%s: n_planes = %d, expected %d .. %d", __func__, n_planes, DEPTHMVS_MIN_PLANES, DEPTHMVS_MAX_PLANES);
  if (best_views < 1 || best_views > n_views)
    return fail(DEPTHMVS_ERR_ARG, "%s: best_views = %d, expected 1 .. n_views = %d", __func__, best_views, n_views);
  if (agg_radius < 0 || agg_radius > DEPTHMVS_MAX_RADIUS)
    return fail(DEPTHMVS_ERR_ARG, "%s: agg_radius = %d, expected 0 .. %d", __func__, agg_radius, DEPTHMVS_MAX_RADIUS);
  if (!(uniqueness > 0.0 && uniqueness <= 1.0))
    return fail(DEPTHMVS_ERR_ARG, "%s: uniqueness = %g: expected a number in (0, 1]", __func__, uniqueness);
  if (!(std_planes > 0.0 && std_planes < INFINITY))
    return fail(DEPTHMVS_ERR_ARG, "%s: std_planes = %g: expected a finite number > 0", __func__, std_planes);
  REQUIRE(rgb && cams && nbr && inv_depth && workspace, "non-null rgb, cams, nbr, inv_depth, workspace");
  REQUIRE(depth && std && status, "non-null depth, std, status");
  REQUIRE(aligned4(depth, std, nbr, census), "depth, std, nbr and census aligned to 4 bytes");
  REQUIRE(((uintptr_t)cost & 1) == 0 && ((uintptr_t)second & 1) == 0, "cost and second aligned to 2 bytes");
  REQUIRE(((uintptr_t)cams & 7) == 0 && ((uintptr_t)inv_depth & 7) == 0 && ((uintptr_t)rows & 7) == 0,
          "cams, inv_depth and rows aligned to 8 bytes");
  REQUIRE(((uintptr_t)workspace & 255) == 0, "workspace aligned to 256 bytes");
  const int64_t px = (int64_t)height * width, n = (int64_t)n_frames * px;
  const Layout l = layout(n_frames, height, width);
  const struct { const char* name; const void* p; int64_t bytes; } ins[] = {
      {"rgb", rgb, 3 * n}, {"cams", cams, 8ll * DEPTHMVS_CAM * n_frames}, {"nbr", nbr, 4ll * n_views * n_frames},
      {"inv_depth", inv_depth, 8ll * n_planes}};
  const struct { const char* name; const void* p; int64_t bytes; } outs[] = {
      {"depth", depth, 4 * n}, {"std", std, 4 * n}, {"status", status, n}, {"plane", plane, n}, {"cost", cost, 2 * n},
      {"second", second, 2 * n}, {"census", census, 4 * n}, {"rows", rows, 8ll * DEPTHMVS_ROW * n_frames},
      {"workspace", workspace, l.bytes}};
  for (const auto& o : outs)
    for (const auto& i : ins)
      if (overlap(i.p, i.bytes, o.p, o.bytes))
        return fail(DEPTHMVS_ERR_ARG, "%s: %s overlaps %s: the launches read %s throughout", __func__, o.name, i.name, i.name);
  for (size_t i = 0; i < sizeof(outs) / sizeof(outs[0]); ++i)
    for (size_t j = i + 1; j < sizeof(outs) / sizeof(outs[0]); ++j)
      if (overlap(outs[i].p, outs[i].bytes, outs[j].p, outs[j].bytes))
        return fail(DEPTHMVS_ERR_ARG, "%s: %s overlaps %s", __func__, outs[i].name, outs[j].name);

  const hipStream_t st = (hipStream_t)stream;
  char* ws = (char*)workspace;
  uint32_t* cen = census ? census : (uint32_t*)(ws + l.census);
  for_chunks(n, depthprior::MAX_GRID * DEPTHMVS_BLOCK, [&](int64_t i0, int64_t n_px) {
    launch_depthmvs_census(st, rgb, height, width, i0, n_px, cen);
  });
  const int64_t tiles = depthmvs_tiles(height, width), n_wg = (int64_t)n_frames * tiles;
  DepthmvsSweep a;
  a.cams = cams; a.nbr = nbr; a.inv_depth = inv_depth; a.census = cen;
  a.depth = depth; a.std = std; a.status = status; a.plane = plane; a.cost = cost; a.second = second;
  a.partial = rows ? (int32_t*)(ws + l.partial) : nullptr;
  a.n_frames = n_frames; a.height = height; a.width = width; a.tiles_x = (int)depthprior::tiles_x(width, DEPTHMVS_TILE_W);
  a.n_views = n_views; a.n_planes = n_planes; a.best_views = best_views; a.radius = agg_radius;
  a.tiles = tiles; a.uniqueness = uniqueness; a.std_planes = std_planes;
  a.slab = nullptr; a.slab_f0 = 0; a.dp = 0;
  for_chunks(n_wg, depthprior::MAX_GRID, [&](int64_t g0, int64_t n) { launch_depthmvs_sweep(st, a, g0, n); });
  if (rows) launch_depthmvs_rows(st, n_frames, tiles, px, a.partial, rows);
  return check_launch("depthmvs_sweep");
}

}  // extern "C"

// extern "C" surface of libdepthsgm_hip.so (include/depthsgm_hip.h): argument checks (no HIP call, so a host without a GPU gets the
// same errors), the workspace layout, the loop over chunks of slab_frames frames and the launches.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include "../../include/depthsgm_hip.h"
#define API_OK DEPTHSGM_OK
#define API_ERR_HIP DEPTHSGM_ERR_HIP
#define API_ERR_ARG DEPTHSGM_ERR_ARG
#include "api_common.h"
#include "depthsgm_kernels.h"

namespace {

int64_t up256(int64_t n) { return (n + 255) / 256 * 256; }

// the workspace, every part aligned to 256: census [F, H, W] uint32; partial [F, tiles, 4] int32; cslab [s, H, W, dp] uint16;
// sslab [s, H, W, dp] uint32, s = min(slab_frames, F)
struct Layout {
  int64_t census, partial, cslab, sslab, bytes;
  int slab_frames, dp;
};
Layout layout(int n_frames, int height, int width, int n_planes, int slab_frames) {
  Layout l;
  l.slab_frames = slab_frames < n_frames ? slab_frames : n_frames;
  l.dp = depthsgm_dp(n_planes);
  const int64_t entries = (int64_t)l.slab_frames * height * width * l.dp;
  l.census = 0;
  l.partial = up256(4 * (int64_t)n_frames * height * width);
  l.cslab = l.partial + up256((int64_t)n_frames * depthmvs_tiles(height, width) * 4 * (int64_t)sizeof(int32_t));
  l.sslab = l.cslab + up256(2 * entries);
  l.bytes = l.sslab + up256(4 * entries);
  return l;
}

int sizes_ok(const char* fn, int n_frames, int height, int width, int n_planes, int slab_frames) {
  const int rc = frames_ok(fn, n_frames, height, width, DEPTHMVS_MAX_FRAMES, DEPTHMVS_MAX_PIXELS);
  if (rc != DEPTHSGM_OK) return rc;
  if (n_planes < DEPTHMVS_MIN_PLANES || n_planes > DEPTHMVS_MAX_PLANES)
    return fail(DEPTHSGM_ERR_ARG, "%s: n_planes = %d, expected %d .. %d", fn, n_planes, DEPTHMVS_MIN_PLANES, DEPTHMVS_MAX_PLANES);
  if (slab_frames < 1) return fail(DEPTHSGM_ERR_ARG, "%s: slab_frames = %d, expected at least 1", fn, slab_frames);
  return DEPTHSGM_OK;
}

// the directions in the order of the definition; the first smooth_paths of them run
const int DIRS[8][2] = {{1, 0}, {-1, 0}, {0, 1}, {0, -1}, {1, 1}, {-1, -1}, {1, -1}, {-1, 1}};

}  // namespace

extern "C" {

const char* depthsgm_last_error(void) { return g_err; }
int depthsgm_abi_version(void) { return DEPTHSGM_ABI_VERSION; }

int64_t depthsgm_workspace_bytes(int n_frames, int height, int width, int n_planes, int slab_frames) {
  if (sizes_ok(__func__, n_frames, height, width, n_planes, slab_frames) != DEPTHSGM_OK) return -1;
  return layout(n_frames, height, width, n_planes, slab_frames).bytes;
}

int depthsgm_sweep(void* stream, int n_frames, int height, int width, int n_views, int n_planes, const uint8_t* rgb,
                   const double* cams, const int32_t* nbr, const double* inv_depth, int best_views, int agg_radius, double uniqueness,
                   double std_planes, int smooth_paths, int p1, int p2, int smooth_edge, int slab_frames, void* workspace, float* depth,
                   float* std, uint8_t* status, uint8_t* plane, uint32_t* cost, uint32_t* second, uint32_t* census, int64_t* rows) {
  const int rc = frames_ok(__func__, n_frames, height, width, DEPTHMVS_MAX_FRAMES, DEPTHMVS_MAX_PIXELS);
  if (rc != DEPTHSGM_OK) return rc;
  if (n_views < 1 || n_views > DEPTHMVS_MAX_VIEWS)
    return fail(DEPTHSGM_ERR_ARG, "%s: n_views = %d, expected 1 .. %d", __func__, n_views, DEPTHMVS_MAX_VIEWS);
  if (n_planes < DEPTHMVS_MIN_PLANES || n_planes > DEPTHMVS_MAX_PLANES)
    return fail(DEPTHSGM_ERR_ARG, "%s: n_planes = %d, expected %d .. %d", __func__, n_planes, DEPTHMVS_MIN_PLANES, DEPTHMVS_MAX_PLANES);
  if (best_views < 1 || best_views > n_views)
    return fail(DEPTHSGM_ERR_ARG, "%s: best_views = %d, expected 1 .. n_views = %d", __func__, best_views, n_views);
  if (agg_radius < 0 || agg_radius > DEPTHMVS_MAX_RADIUS)
    return fail(DEPTHSGM_ERR_ARG, "%s: agg_radius = %d, expected 0 .. %d", __func__, agg_radius, DEPTHMVS_MAX_RADIUS);
  if (!(uniqueness > 0.0 && uniqueness <= 1.0))
    return fail(DEPTHSGM_ERR_ARG, "%s: uniqueness = %g: expected a number in (0, 1]", __func__, uniqueness);
  if (!(std_planes > 0.0 && std_planes < INFINITY))
    return fail(DEPTHSGM_ERR_ARG, "%s: std_planes = %g: expected a finite number > 0", __func__, std_planes);
  if (smooth_paths != 4 && smooth_paths != 8)
    return fail(DEPTHSGM_ERR_ARG, "%s: smooth_paths = %d, expected 4 or 8", __func__, smooth_paths);
  if (p1 < 1 || p1 > p2 || p2 > DEPTHSGM_MAX_P2)
    return fail(DEPTHSGM_ERR_ARG, "%s: p1 = %d, p2 = %d: expected 1 <= p1 <= p2 <= %d", __func__, p1, p2, DEPTHSGM_MAX_P2);
  if (smooth_edge < 0 || smooth_edge > DEPTHSGM_MAX_EDGE)
    return fail(DEPTHSGM_ERR_ARG, "%s: smooth_edge = %d, expected 0 .. %d", __func__, smooth_edge, DEPTHSGM_MAX_EDGE);
  if (slab_frames < 1) return fail(DEPTHSGM_ERR_ARG, "%s: slab_frames = %d, expected at least 1", __func__, slab_frames);
  REQUIRE(rgb && cams && nbr && inv_depth && workspace, "non-null rgb, cams, nbr, inv_depth, workspace");
  REQUIRE(depth && std && status, "non-null depth, std, status");
  REQUIRE(aligned4(depth, std, nbr, census, cost, second), "depth, std, nbr, census, cost and second aligned to 4 bytes");
  REQUIRE(((uintptr_t)cams & 7) == 0 && ((uintptr_t)inv_depth & 7) == 0 && ((uintptr_t)rows & 7) == 0,
          "cams, inv_depth and rows aligned to 8 bytes");
  REQUIRE(((uintptr_t)workspace & 255) == 0, "workspace aligned to 256 bytes");
  const int64_t px = (int64_t)height * width, n = (int64_t)n_frames * px;
  const Layout l = layout(n_frames, height, width, n_planes, slab_frames);
  const struct { const char* name; const void* p; int64_t bytes; } ins[] = {
      {"rgb", rgb, 3 * n}, {"cams", cams, 8ll * DEPTHMVS_CAM * n_frames}, {"nbr", nbr, 4ll * n_views * n_frames},
      {"inv_depth", inv_depth, 8ll * n_planes}};
  const struct { const char* name; const void* p; int64_t bytes; } outs[] = {
      {"depth", depth, 4 * n}, {"std", std, 4 * n}, {"status", status, n}, {"plane", plane, n}, {"cost", cost, 4 * n},
      {"second", second, 4 * n}, {"census", census, 4 * n}, {"rows", rows, 8ll * DEPTHMVS_ROW * n_frames},
      {"workspace", workspace, l.bytes}};
  for (const auto& o : outs)
    for (const auto& i : ins)
      if (overlap(i.p, i.bytes, o.p, o.bytes))
        return fail(DEPTHSGM_ERR_ARG, "%s: %s overlaps %s: the launches read %s throughout", __func__, o.name, i.name, i.name);
  for (size_t i = 0; i < sizeof(outs) / sizeof(outs[0]); ++i)
    for (size_t j = i + 1; j < sizeof(outs) / sizeof(outs[0]); ++j)
      if (overlap(outs[i].p, outs[i].bytes, outs[j].p, outs[j].bytes))
        return fail(DEPTHSGM_ERR_ARG, "%s: %s overlaps %s", __func__, outs[i].name, outs[j].name);

  const hipStream_t st = (hipStream_t)stream;
  char* ws = (char*)workspace;
  uint32_t* cen = census ? census : (uint32_t*)(ws + l.census);
  for_chunks(n, depthprior::MAX_GRID * DEPTHMVS_BLOCK, [&](int64_t i0, int64_t n_px) {
    launch_depthsgm_census(st, rgb, height, width, i0, n_px, cen);
  });
  const int64_t tiles = depthmvs_tiles(height, width);
  uint16_t* cslab = (uint16_t*)(ws + l.cslab);
  uint32_t* sslab = (uint32_t*)(ws + l.sslab);
  int32_t* partial = rows ? (int32_t*)(ws + l.partial) : nullptr;
  DepthmvsSweep a;
  a.cams = cams; a.nbr = nbr; a.inv_depth = inv_depth; a.census = cen;
  a.depth = nullptr; a.std = nullptr; a.status = nullptr; a.plane = nullptr; a.cost = nullptr; a.second = nullptr; a.partial = nullptr;
  a.n_frames = n_frames; a.height = height; a.width = width; a.tiles_x = (int)depthprior::tiles_x(width, DEPTHMVS_TILE_W);
  a.n_views = n_views; a.n_planes = n_planes; a.best_views = best_views; a.radius = agg_radius;
  a.tiles = tiles; a.uniqueness = uniqueness; a.std_planes = std_planes;
  a.slab = cslab; a.dp = l.dp;
  DepthsgmPaths p;
  p.cslab = cslab; p.sslab = sslab; p.height = height; p.width = width; p.n_planes = n_planes; p.dp = l.dp;
  p.p1 = p1; p.p2 = p2; p.edge = smooth_edge;
  DepthsgmSelect s;
  s.cslab = cslab; s.sslab = sslab; s.inv_depth = inv_depth; s.depth = depth; s.std = std; s.status = status; s.plane = plane;
  s.cost = cost; s.second = second; s.partial = partial; s.height = height; s.width = width; s.tiles_x = a.tiles_x;
  s.n_planes = n_planes; s.dp = l.dp; s.tiles = tiles; s.uniqueness = uniqueness; s.std_planes = std_planes;
  for (int f0 = 0; f0 < n_frames; f0 += l.slab_frames) {
    const int frames = n_frames - f0 < l.slab_frames ? n_frames - f0 : l.slab_frames;
    a.slab_f0 = f0;
    for_chunks(frames * tiles, depthprior::MAX_GRID, [&](int64_t g0, int64_t n_wg) { launch_depthsgm_slab(st, a, f0 * tiles + g0, n_wg); });
    p.rgb = rgb + 3 * f0 * px;
    p.frames = frames;
    for (int r = 0; r < smooth_paths; ++r) {
      p.dx = DIRS[r][0]; p.dy = DIRS[r][1]; p.first = r == 0;
      p.lines = depthsgm_lines(height, width, p.dx, p.dy);
      const int64_t waves = frames * p.lines;
      for_chunks((waves + DEPTHSGM_PATH_WAVES - 1) / DEPTHSGM_PATH_WAVES, depthprior::MAX_GRID,
                 [&](int64_t g0, int64_t n_wg) { launch_depthsgm_paths(st, p, g0, n_wg); });
    }
    s.f0 = f0;
    for_chunks(frames * tiles, depthprior::MAX_GRID, [&](int64_t g0, int64_t n_wg) { launch_depthsgm_select(st, s, g0, n_wg); });
  }
  if (rows) launch_depthsgm_rows(st, n_frames, tiles, px, partial, rows);
  return check_launch("depthsgm_sweep");
}

}  // extern "C"

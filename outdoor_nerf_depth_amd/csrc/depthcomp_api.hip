// extern "C" surface of libdepthcomp_hip.so (include/depthcomp_hip.h): argument checks (no HIP call, so a host without a GPU gets the
// same errors), the workspace layout and the launches.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include "../../include/depthcomp_hip.h"
#define API_OK DEPTHCOMP_OK
#define API_ERR_HIP DEPTHCOMP_ERR_HIP
#define API_ERR_ARG DEPTHCOMP_ERR_ARG
#include "api_common.h"
#include "depthcomp_kernels.h"

namespace {

int64_t up256(int64_t n) { return (n + 255) / 256 * 256; }

// the workspace, every part aligned to 256: the second state z, c, v [F, H, W] float32; a stand-in for conf, float32; the second
// state's pass and a stand-in for pass, uint8; partial [F, tiles, 4] int32
struct Layout {
  int64_t z, c, v, conf, pass2, pass, partial, bytes;
};
Layout layout(int n_frames, int height, int width) {
  const int64_t n = (int64_t)n_frames * height * width, f = up256(4 * n), b = up256(n);
  Layout l;
  l.z = 0;
  l.c = f;
  l.v = 2 * f;
  l.conf = 3 * f;
  l.pass2 = 4 * f;
  l.pass = 4 * f + b;
  l.partial = 4 * f + 2 * b;
  l.bytes = l.partial + up256((int64_t)n_frames * depthcomp_tiles(height, width) * 4 * (int64_t)sizeof(int32_t));
  return l;
}

}  // namespace

extern "C" {

const char* depthcomp_last_error(void) { return g_err; }
int depthcomp_abi_version(void) { return DEPTHCOMP_ABI_VERSION; }

int64_t depthcomp_workspace_bytes(int n_frames, int height, int width) {
  if (frames_ok(__func__, n_frames, height, width, DEPTHCOMP_MAX_FRAMES, DEPTHCOMP_MAX_PIXELS) != DEPTHCOMP_OK) return -1;
  return layout(n_frames, height, width).bytes;
}

int depthcomp_complete(void* stream, int n_frames, int height, int width, const float* depth, const uint8_t* rgb, const float* std_in,
                       const double* w_space, const double* w_colour, int radius, int iters, int min_points, double min_conf,
                       double max_rel_spread, double decay, void* workspace, float* depth_out, float* std_out, float* conf,
                       uint8_t* origin, uint8_t* pass, int64_t* rows) {
  const int rc = frames_ok(__func__, n_frames, height, width, DEPTHCOMP_MAX_FRAMES, DEPTHCOMP_MAX_PIXELS);
  if (rc != DEPTHCOMP_OK) return rc;
  if (radius < 1 || radius > DEPTHCOMP_MAX_RADIUS)
    return fail(DEPTHCOMP_ERR_ARG, "%s: radius = %d, expected 1 .. %d", __func__, radius, DEPTHCOMP_MAX_RADIUS);
  if (iters < 1 || iters > DEPTHCOMP_MAX_ITERS)
    return fail(DEPTHCOMP_ERR_ARG, "%s: iters = %d, expected 1 .. %d", __func__, iters, DEPTHCOMP_MAX_ITERS);
  if (min_points < 1 || min_points > DEPTHCOMP_MAX_POINTS)
    return fail(DEPTHCOMP_ERR_ARG, "%s: min_points = %d, expected 1 .. %d", __func__, min_points, DEPTHCOMP_MAX_POINTS);
  if (!(min_conf >= 0.0 && min_conf <= 1.0))
    return fail(DEPTHCOMP_ERR_ARG, "%s: min_conf = %g: expected a number in [0, 1]", __func__, min_conf);
  if (!(max_rel_spread >= 0.0))
    return fail(DEPTHCOMP_ERR_ARG, "%s: max_rel_spread = %g: expected a number >= 0 (+inf: no gate)", __func__, max_rel_spread);
  if (!(decay > 0.0 && decay <= 1.0))
    return fail(DEPTHCOMP_ERR_ARG, "%s: decay = %g: expected a number in (0, 1]", __func__, decay);
  REQUIRE(depth && rgb && w_space && w_colour && workspace, "non-null depth, rgb, w_space, w_colour, workspace");
  REQUIRE(depth_out && std_out && origin, "non-null depth_out, std_out, origin");
  REQUIRE(aligned4(depth, std_in, depth_out, std_out, conf), "depth, std_in, depth_out, std_out and conf aligned to 4 bytes");
  REQUIRE(((uintptr_t)w_space & 7) == 0 && ((uintptr_t)w_colour & 7) == 0 && ((uintptr_t)rows & 7) == 0,
          "w_space, w_colour and rows aligned to 8 bytes");
  REQUIRE(((uintptr_t)workspace & 255) == 0, "workspace aligned to 256 bytes");
  const int64_t n = (int64_t)n_frames * height * width;
  const Layout l = layout(n_frames, height, width);
  const int side = 2 * radius + 1;
  const struct { const char* name; const void* p; int64_t bytes; } ins[] = {
      {"depth", depth, 4 * n}, {"rgb", rgb, 3 * n}, {"std_in", std_in, 4 * n}, {"w_space", w_space, 8ll * side * side},
      {"w_colour", w_colour, 8ll * DEPTHCOMP_COLOUR_TABLE}};
  const struct { const char* name; const void* p; int64_t bytes; } outs[] = {
      {"depth_out", depth_out, 4 * n}, {"std_out", std_out, 4 * n}, {"conf", conf, 4 * n}, {"origin", origin, n},
      {"pass", pass, n}, {"rows", rows, 8ll * DEPTHCOMP_ROW * n_frames}, {"workspace", workspace, l.bytes}};
  for (const auto& o : outs)
    for (const auto& i : ins)
      if (overlap(i.p, i.bytes, o.p, o.bytes))
        return fail(DEPTHCOMP_ERR_ARG, "%s: %s overlaps %s: the launches read %s throughout", __func__, o.name, i.name, i.name);
  for (size_t i = 0; i < sizeof(outs) / sizeof(outs[0]); ++i)
    for (size_t j = i + 1; j < sizeof(outs) / sizeof(outs[0]); ++j)
      if (overlap(outs[i].p, outs[i].bytes, outs[j].p, outs[j].bytes))
        return fail(DEPTHCOMP_ERR_ARG, "%s: %s overlaps %s", __func__, outs[i].name, outs[j].name);

  const hipStream_t st = (hipStream_t)stream;
  char* ws = (char*)workspace;
  // the passes alternate between the outputs (X) and the workspace (Y) so that the last one writes the outputs
  const DepthcompState X = {depth_out, conf ? conf : (float*)(ws + l.conf), std_out, pass ? pass : (uint8_t*)(ws + l.pass)};
  const DepthcompState Y = {(float*)(ws + l.z), (float*)(ws + l.c), (float*)(ws + l.v), (uint8_t*)(ws + l.pass2)};
  const int64_t tiles = depthcomp_tiles(height, width), n_wg = (int64_t)n_frames * tiles;
  int32_t* partial = rows ? (int32_t*)(ws + l.partial) : nullptr;
  DepthcompPass a;
  a.depth = depth; a.rgb = rgb; a.std_in = std_in; a.w_space = w_space; a.w_colour = w_colour;
  a.height = height; a.width = width; a.tiles_x = (int)depthprior::tiles_x(width, DEPTHCOMP_TILE_W); a.tiles = tiles;
  a.radius = radius; a.min_points = min_points; a.min_conf = min_conf; a.max_rel_spread = max_rel_spread; a.decay = decay;
  for (int k = 1; k <= iters; ++k) {
    const bool last = k == iters, to_x = (iters - k) % 2 == 0;
    a.k = k;
    a.in = to_x ? Y : X;                                     // (not read by the first pass)
    a.out = to_x ? X : Y;
    if (last) a.out = DepthcompState{depth_out, conf, std_out, pass};
    a.origin = last ? origin : nullptr;
    a.partial = last ? partial : nullptr;
    for_chunks(n_wg, depthprior::MAX_GRID, [&](int64_t g0, int64_t n) { launch_depthcomp_pass(st, a, k == 1, last, g0, n); });
  }
  if (rows) launch_depthcomp_rows(st, n_frames, tiles, (int64_t)height * width, partial, rows);
  return check_launch("depthcomp_complete");
}

}  // extern "C"

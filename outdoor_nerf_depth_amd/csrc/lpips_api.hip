// extern "C" surface of liblpips_hip.so (include/lpips_hip.h): argument checks (no HIP call, so a host without a GPU gets
// the same errors), the layouts of the packed weights and of the workspace, and the launch sequence of the network.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include "../../include/lpips_hip.h"
#define API_OK LPIPS_OK
#define API_ERR_HIP LPIPS_ERR_HIP
#define API_ERR_ARG LPIPS_ERR_ARG
#include "api_common.h"
#include "lpips_kernels.h"

namespace {

constexpr int CIN[LPIPS_N_CONV] = {3, 64, 64, 128, 128, 256, 256, 256, 512, 512, 512, 512, 512};
constexpr int COUT[LPIPS_N_CONV] = {64, 64, 128, 128, 256, 256, 256, 512, 512, 512, 512, 512, 512};
constexpr int TAP_AFTER[LPIPS_N_TAPS] = {1, 3, 6, 9, 12};     // a tap (and, except the last, a pool) follows these layers
constexpr int TAP_C[LPIPS_N_TAPS] = {64, 128, 256, 512, 512};

int64_t align_up(int64_t v, int64_t a) { return (v + a - 1) / a * a; }

struct PackedLayout { int64_t w[LPIPS_N_CONV], b[LPIPS_N_CONV], lin[LPIPS_N_TAPS], total; };   // float offsets
struct FlatLayout { int64_t w[LPIPS_N_CONV], b[LPIPS_N_CONV], lin[LPIPS_N_TAPS], total; };
PackedLayout packed_layout() {
  PackedLayout L;
  int64_t off = 0;
  for (int i = 0; i < LPIPS_N_CONV; ++i) {
    L.w[i] = off; off += (int64_t)lpips_kp(CIN[i]) * COUT[i];
    L.b[i] = off; off += COUT[i];
  }
  for (int l = 0; l < LPIPS_N_TAPS; ++l) { L.lin[l] = off; off += TAP_C[l]; }
  L.total = off;
  return L;
}
FlatLayout flat_layout() {
  FlatLayout L;
  int64_t off = 0;
  for (int i = 0; i < LPIPS_N_CONV; ++i) {
    L.w[i] = off; off += (int64_t)COUT[i] * CIN[i] * 9;
    L.b[i] = off; off += COUT[i];
  }
  for (int l = 0; l < LPIPS_N_TAPS; ++l) { L.lin[l] = off; off += TAP_C[l]; }
  L.total = off;
  return L;
}

int sizes_ok(const char* fn, int n_pairs, int H, int W) {
  if (n_pairs < 1 || n_pairs > 65535) return fail(LPIPS_ERR_ARG, "%s: n_pairs = %d, expected 1 .. 65535", fn, n_pairs);
  if (H < LPIPS_MIN_SIDE || W < LPIPS_MIN_SIDE)
    return fail(LPIPS_ERR_ARG, "%s: a %d x %d image is too small for the four 2 x 2 pools of VGG-16 (H >= 16 and W >= 16)", fn, H, W);
  if ((int64_t)H * W > (1ll << 26)) return fail(LPIPS_ERR_ARG, "%s: a %d x %d image exceeds 2^26 pixels", fn, H, W);
  return LPIPS_OK;
}

// pairs per group, feature-buffer floats per group, partials per pair
struct WsLayout { int group; int64_t buf_floats; int64_t part_stride; int64_t part_off; int64_t total; LpipsFinishArgs fin; };
WsLayout ws_layout(int n_pairs, int H, int W) {
  WsLayout L;
  const int64_t per_pair = (int64_t)2 * H * W * 64;                 // floats of one 64-channel full-resolution map pair
  int64_t g = LPIPS_GROUP_BYTES / (2 * per_pair * 4);
  if (g < 1) g = 1;
  if (g > n_pairs) g = n_pairs;
  L.group = (int)g;
  L.buf_floats = align_up(g * per_pair, 64);
  int h = H, w = W, off = 0;
  for (int l = 0; l < LPIPS_N_TAPS; ++l) {
    L.fin.off[l] = off;
    L.fin.nblk[l] = lpips_tap_blocks(h, w);
    L.fin.npix[l] = (double)h * (double)w;
    off += L.fin.nblk[l];
    h /= 2; w /= 2;
  }
  L.part_stride = off;
  L.part_off = 2 * L.buf_floats * 4;
  L.total = align_up(L.part_off + (int64_t)n_pairs * L.part_stride * 8, 256);
  return L;
}

}  // namespace

extern "C" {

const char* lpips_last_error(void) { return g_err; }
int lpips_abi_version(void) { return LPIPS_ABI_VERSION; }

int64_t lpips_packed_conv_floats(int Cin, int Cout) {
  if (Cin < 1 || Cin > 4096 || Cout < 64 || Cout > 4096 || Cout % 64 != 0) {
    fail(LPIPS_ERR_ARG, "%s: Cin = %d, Cout = %d: expected 1 <= Cin <= 4096 and Cout a multiple of 64 up to 4096", __func__, Cin, Cout);
    return -1;
  }
  return (int64_t)lpips_kp(Cin) * Cout;
}

int lpips_pack_conv(void* stream, int Cin, int Cout, const float* w, float* wp) {
  if (lpips_packed_conv_floats(Cin, Cout) < 0) return LPIPS_ERR_ARG;
  REQUIRE(w && wp, "non-null w, wp");
  launch_lpips_pack_conv((hipStream_t)stream, Cin, Cout, w, wp);
  return check_launch("lpips_pack_conv");
}

int lpips_conv3x3_relu(void* stream, int n_images, int H, int W, int Cin, int Cout, const float* x, const float* wp,
                       const float* bias, float* y) {
  if (lpips_packed_conv_floats(Cin, Cout) < 0) return LPIPS_ERR_ARG;
  REQUIRE(n_images >= 1 && H >= 1 && W >= 1, "n_images, H, W >= 1");
  REQUIRE((int64_t)n_images * H * W <= (1ll << 30), "n_images * H * W <= 2^30");
  REQUIRE(x && wp && bias && y, "non-null x, wp, bias, y");
  REQUIRE((((uintptr_t)x | (uintptr_t)wp | (uintptr_t)y) & 15) == 0, "x, wp, y aligned to 16 bytes");
  REQUIRE(x != y, "y must not overlap x");
  launch_lpips_conv3x3_relu((hipStream_t)stream, n_images, H, W, Cin, Cout, x, wp, bias, y);
  return check_launch("lpips_conv3x3_relu");
}

int64_t lpips_flat_floats(void) { return flat_layout().total; }
int64_t lpips_packed_bytes(void) { return packed_layout().total * 4; }

int lpips_pack_weights(void* stream, const float* flat, void* packed) {
  REQUIRE(flat && packed, "non-null flat, packed");
  REQUIRE(((uintptr_t)packed & 15) == 0, "packed aligned to 16 bytes");
  const FlatLayout F = flat_layout();
  const PackedLayout P = packed_layout();
  float* dst = (float*)packed;
  const hipStream_t st = (hipStream_t)stream;
  for (int i = 0; i < LPIPS_N_CONV; ++i) {
    launch_lpips_pack_conv(st, CIN[i], COUT[i], flat + F.w[i], dst + P.w[i]);
    if (hipMemcpyAsync(dst + P.b[i], flat + F.b[i], (size_t)COUT[i] * 4, hipMemcpyDeviceToDevice, st) != hipSuccess)
      return check_launch("lpips_pack_weights (bias)");
  }
  if (hipMemcpyAsync(dst + P.lin[0], flat + F.lin[0], (size_t)(P.total - P.lin[0]) * 4, hipMemcpyDeviceToDevice, st) != hipSuccess)
    return check_launch("lpips_pack_weights (lin)");
  return check_launch("lpips_pack_weights");
}

int64_t lpips_workspace_bytes(int n_pairs, int H, int W) {
  if (sizes_ok(__func__, n_pairs, H, W) != LPIPS_OK) return -1;
  return ws_layout(n_pairs, H, W).total;
}

int lpips_u8(void* stream, int n_pairs, int H, int W, const uint8_t* gt_u8, const uint8_t* pred_u8, const void* packed,
             void* workspace, double* out) {
  const int rc = sizes_ok(__func__, n_pairs, H, W);
  if (rc != LPIPS_OK) return rc;
  REQUIRE(gt_u8 && pred_u8 && packed && workspace && out, "non-null gt_u8, pred_u8, packed, workspace, out");
  REQUIRE(((uintptr_t)packed & 15) == 0, "packed aligned to 16 bytes");
  REQUIRE(((uintptr_t)workspace & 255) == 0 && ((uintptr_t)out & 7) == 0, "workspace aligned to 256 bytes, out to 8");
  const hipStream_t st = (hipStream_t)stream;
  const WsLayout L = ws_layout(n_pairs, H, W);
  const PackedLayout P = packed_layout();
  const float* pk = (const float*)packed;
  float* buf[2] = {(float*)workspace, (float*)workspace + L.buf_floats};
  double* part = (double*)((char*)workspace + L.part_off);
  const size_t frame = (size_t)H * W * 3;
  for (int g0 = 0; g0 < n_pairs; g0 += L.group) {
    const int gp = n_pairs - g0 < L.group ? n_pairs - g0 : L.group, ni = 2 * gp;
    int cur = 0, h = H, w = W, tap = 0;
    launch_lpips_prep(st, gp, H, W, gt_u8 + (size_t)g0 * frame, pred_u8 + (size_t)g0 * frame, buf[cur]);
    for (int i = 0; i < LPIPS_N_CONV; ++i) {
      launch_lpips_conv3x3_relu(st, ni, h, w, CIN[i], COUT[i], buf[cur], pk + P.w[i], pk + P.b[i], buf[cur ^ 1]);
      cur ^= 1;
      if (i == TAP_AFTER[tap]) {
        launch_lpips_tap(st, gp, h, w, TAP_C[tap], buf[cur], pk + P.lin[tap], part + (size_t)g0 * L.part_stride + L.fin.off[tap],
                         L.part_stride);
        if (++tap < LPIPS_N_TAPS) {
          launch_lpips_pool(st, ni, h, w, COUT[i], buf[cur], buf[cur ^ 1]);
          cur ^= 1;
          h /= 2; w /= 2;
        } else {
          break;
        }
      }
    }
    const int e = check_launch("lpips_u8");
    if (e != LPIPS_OK) return e;
  }
  launch_lpips_finish(st, n_pairs, part, L.part_stride, L.fin, out);
  return check_launch("lpips_u8 (finish)");
}

}  // extern "C"

// The preamble of a C ABI file (*_api.hip): the thread's last error text, fail, check_launch, REQUIRE and aligned4.  The including file
// defines its library's three return codes first,
//     #define API_OK      <LIB>_OK
//     #define API_ERR_HIP <LIB>_ERR_HIP
//     #define API_ERR_ARG <LIB>_ERR_ARG
// and its <lib>_last_error() returns g_err.  Everything here has internal linkage: one copy per shared object, none exported.
#pragma once
#include <hip/hip_runtime.h>
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>
#if !defined(API_OK) || !defined(API_ERR_HIP) || !defined(API_ERR_ARG)
#error "define API_OK, API_ERR_HIP and API_ERR_ARG before including api_common.h"
#endif

namespace {

thread_local char g_err[512] = "";

int fail(int code, const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
  return code;
}

int check_launch(const char* what) {
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return fail(API_ERR_HIP, "%s: %s", what, hipGetErrorString(e));
  return API_OK;
}

#define REQUIRE(cond, what) \
  do { if (!(cond)) return fail(API_ERR_ARG, "%s: requirement failed: %s", __func__, what); } while (0)

// every pointer of the list is a multiple of 4 bytes (a null one is)
template <typename... P>
bool aligned4(const P*... p) { return ((... | (uintptr_t)p) & 3) == 0; }

// The frames of a depth-prior call (depthcons, depthacc, depthalign, depthcomp, depthmvs, depthpoints): 1 .. max_frames frames of
// 1 .. max_pixels = 2^28 pixels each.  No HIP call: a host without a GPU gets the same errors.
int frames_ok(const char* fn, int n_frames, int height, int width, int max_frames, int64_t max_pixels) {
  if (n_frames < 1 || n_frames > max_frames) return fail(API_ERR_ARG, "%s: n_frames = %d, expected 1 .. %d", fn, n_frames, max_frames);
  if (height < 1 || width < 1)
    return fail(API_ERR_ARG, "%s: height = %d, width = %d: a frame has at least one pixel", fn, height, width);
  if ((int64_t)height * width > max_pixels)
    return fail(API_ERR_ARG, "%s: height * width = %lld exceeds 2^28 pixels per frame", fn, (long long)height * width);
  return API_OK;
}

// do [a, a + na) and [b, b + nb) bytes share a byte?
bool overlap(const void* a, int64_t na, const void* b, int64_t nb) {
  const uintptr_t pa = (uintptr_t)a, pb = (uintptr_t)b;
  return a != nullptr && b != nullptr && pa < pb + (uintptr_t)nb && pb < pa + (uintptr_t)na;
}

// f(g0, n) for the chunks [g0, g0 + n) of at most max_grid that cover [0, n_wg), in order: the workgroups of one launch each
template <typename F>
void for_chunks(int64_t n_wg, int64_t max_grid, F f) {
  for (int64_t g0 = 0; g0 < n_wg; g0 += max_grid) f(g0, n_wg - g0 < max_grid ? n_wg - g0 : max_grid);
}

}  // namespace

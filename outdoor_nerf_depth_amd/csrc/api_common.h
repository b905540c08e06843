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

}  // namespace

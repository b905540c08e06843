// The launcher of libdepthguide_hip.so (depthguide_kernels.hip) and what it reads.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/depthguide_hip.h"
// The one definition of the Philox generator (RngKey, philox_uniform), included, not copied.  Its stream-id comment ends at stream 4,
// the pixel draw: stream 5 = the stratified quantiles of the depth-guided fine samples (DEPTHGUIDE_RNG_STREAM; not in the reference).
// The id is recorded here and in include/nerfpp_hip.h because nerfpp_common.h is one of the sources the committed counter profile
// is keyed to (bench.py: load_pmc_traffic), so a comment there would withhold the bench line's traffic figures.
#include "nerfpp_common.h"

constexpr int DEPTHGUIDE_RAYS_PER_BLOCK = 4;   // one wave per ray, four waves per workgroup (as sample_pdf_kernel)

// passed by value
struct DepthGuideArgs {
  int n, S_prev, S_in, G;
  const float* zp; const float* wp; const float* zin; const float* lo; const float* hi;
  const float* prior; const float* prior_std;  // null: no prior / the constant
  double std_const, min_std;
  const double* table;                         // [DEPTHGUIDE_TABLE_K + 1]
  const float* v;                              // null with rng.enabled = 0: 0.5
  nerfpp::RngKey rng;
  float* z_merged; int32_t* mode; float* guide;
};

void launch_depthguide_merge(hipStream_t st, const DepthGuideArgs& a);

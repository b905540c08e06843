// The launchers of libdepthmvs_hip.so: the census, the sweep with its running state in registers (SLAB = false) and the rows sum, all
// defined in depthmvs_sweep.h.
#include "depthmvs_sweep.h"

using namespace depthmvs_dev;

void launch_depthmvs_census(hipStream_t st, const uint8_t* rgb, int height, int width, int64_t i0, int64_t n, uint32_t* census) {
  depthmvs_census_kernel<<<(unsigned)((n + BLOCK - 1) / BLOCK), BLOCK, 0, st>>>(rgb, height, width, i0, n, census);
}

void launch_depthmvs_sweep(hipStream_t st, const DepthmvsSweep& a, int64_t wg0, int64_t n_wg) {
  depthmvs_sweep_kernel<false><<<(unsigned)n_wg, BLOCK, 0, st>>>(a, wg0);
}

void launch_depthmvs_rows(hipStream_t st, int n_frames, int64_t tiles, int64_t frame_px, const int32_t* partial, int64_t* rows) {
  depthmvs_rows_kernel<<<n_frames, 64, 0, st>>>(tiles, frame_px, partial, rows);
}

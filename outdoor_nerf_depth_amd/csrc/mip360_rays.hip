// MipNeRF-360 front-end kernels for gfx950: camera rays with mip-NeRF cone radii for one frame, the device-side training
// batch of datasets.Dataset._next_train (batching = 'all_images', patch_size = 1), and the distance percentiles of
// render.volumetric_rendering.  float32, VALU-light and store-bound: one thread per ray (rays) or one wave per ray
// (percentiles).  Compiled with -ffp-contract=off so the arithmetic order is the one written out below.
//
// Upstream lines (nerf-methods/mipnerf360/internal/): camera_utils.py:430-631 (pixels_to_rays, PERSPECTIVE, no NDC,
// _radial_and_tangential_undistort), datasets.py:387-486 (_make_ray_batch, _next_train), render.py:180,204-214 and
// stepfun.py:133-152,306-317 (integrate_weights, weighted_percentile).
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include "mip360_launch.h"

namespace mip360_rays {

constexpr int TPB = 256;       // rays per block of the two ray kernels
constexpr int RPB = 4;         // rays per 256-thread block of the percentile kernel (one wave each)

// ---- counter-based generator of the training batch ----------------------------------------------------------------
// Philox4x32-10 (Salmon et al., SC'11), the generator of nerfpp_sample_pixels: key = the 64-bit seed, counter = (ray index,
// stream id, sampler counter lo, hi).  Stream 0 gives the pixel draw (word 0 -> frame, 1 -> x, 2 -> y), stream 1 + l the
// jitter of sampling level l (word 0).
struct Words { uint32_t w[4]; };
__device__ __forceinline__ uint32_t mulhi32(uint32_t a, uint32_t b) { return (uint32_t)(((uint64_t)a * b) >> 32); }
__device__ __forceinline__ Words philox(uint64_t seed, uint64_t counter, uint32_t stream, uint32_t idx) {
  uint32_t c0 = idx, c1 = stream, c2 = (uint32_t)counter, c3 = (uint32_t)(counter >> 32);
  uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const uint32_t h0 = mulhi32(0xD2511F53u, c0), l0 = 0xD2511F53u * c0;
    const uint32_t h1 = mulhi32(0xCD9E8D57u, c2), l1 = 0xCD9E8D57u * c2;
    const uint32_t n0 = h1 ^ c1 ^ k0, n2 = h0 ^ c3 ^ k1;
    c0 = n0; c1 = l1; c2 = n2; c3 = l0;
    k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
  }
  Words o;
  o.w[0] = c0; o.w[1] = c1; o.w[2] = c2; o.w[3] = c3;
  return o;
}
// uniform integer in [0, m): multiply-shift of a 32-bit word (bias < m / 2^32)
__device__ __forceinline__ int draw_below(uint32_t w, int m) { return (int)(((uint64_t)w * (uint32_t)m) >> 32); }
// uniform float in [0, 1): the top 24 bits, as torch.rand maps a word
__device__ __forceinline__ float unit_float(uint32_t w) { return (float)(w >> 8) * 5.9604644775390625e-8f; }

// ---- pixels_to_rays (camera_utils.py:520-631) for one pixel ----------------------------------------------------------
struct Cam {
  float p[9];      // pixtocam, row-major
  float c[12];     // camtoworld [3, 4], row-major
  float k[6];      // k1 k2 k3 k4 p1 p2
  float has_dist;
};
static_assert(sizeof(Cam) == MIP360_CAM_FLOATS * sizeof(float), "camera table row");

// _radial_and_tangential_undistort (camera_utils.py:473-509) with _compute_residual_and_jacobian (:430-470): ten Newton steps
__device__ void undistort(const Cam& cm, float& x, float& y) {
  const float xd = x, yd = y;
  const float k1 = cm.k[0], k2 = cm.k[1], k3 = cm.k[2], k4 = cm.k[3], p1 = cm.k[4], p2 = cm.k[5];
  for (int it = 0; it < 10; ++it) {
    const float r = x * x + y * y;
    const float d = 1.0f + r * (k1 + r * (k2 + r * (k3 + r * k4)));
    const float fx = d * x + 2 * p1 * x * y + p2 * (r + 2 * x * x) - xd;
    const float fy = d * y + 2 * p2 * x * y + p1 * (r + 2 * y * y) - yd;
    const float d_r = (k1 + r * (2.0f * k2 + r * (3.0f * k3 + r * 4.0f * k4)));
    const float d_x = 2.0f * x * d_r;
    const float d_y = 2.0f * y * d_r;
    const float fx_x = d + d_x * x + 2.0f * p1 * y + 6.0f * p2 * x;
    const float fx_y = d_y * x + 2.0f * p1 * x + 2.0f * p2 * y;
    const float fy_x = d_x * y + 2.0f * p2 * y + 2.0f * p1 * x;
    const float fy_y = d + d_y * y + 2.0f * p2 * x + 6.0f * p1 * y;
    const float den = fy_x * fx_y - fx_x * fy_y;
    const float xn = fx * fy_y - fy * fx_y;
    const float yn = fy * fx_x - fx * fy_x;
    const bool ok = fabsf(den) > 1e-9f;
    x = x + (ok ? xn / den : 0.f);
    y = y + (ok ? yn / den : 0.f);
  }
}

// camera-space direction of pixel coordinate (u, v) (half-pixel offset already added): pixtocam, then the undistortion
__device__ void camera_dir(const Cam& cm, float u, float v, float out[3]) {
  float x = cm.p[0] * u + cm.p[1] * v + cm.p[2];
  float y = cm.p[3] * u + cm.p[4] * v + cm.p[5];
  float z = cm.p[6] * u + cm.p[7] * v + cm.p[8];
  if (cm.has_dist != 0.f) {
    undistort(cm, x, y);
    z = 1.f;
  }
  out[0] = x; out[1] = y; out[2] = z;
}

// OpenCV -> OpenGL flip (diag(1, -1, -1)), then the camera-to-world rotation
__device__ void to_world(const Cam& cm, const float c[3], float out[3]) {
  const float x = c[0], y = -c[1], z = -c[2];
  out[0] = cm.c[0] * x + cm.c[1] * y + cm.c[2] * z;
  out[1] = cm.c[4] * x + cm.c[5] * y + cm.c[6] * z;
  out[2] = cm.c[8] * x + cm.c[9] * y + cm.c[10] * z;
}

struct Ray { float o[3], d[3], v[3], radius; };

// The radius needs |d(x+1) - d| and |d(y+1) - d|: differences of nearly equal vectors (about 1 / focal of |d|).  Upstream forms
// them after the rotation; here the same quantities are formed before it (the flip and the rotation are linear, and without
// distortion so is pixtocam: the +x / +y differences are exactly its first / second column), which keeps float32 from losing
// log2(focal) bits to cancellation.  With distortion the undistorted neighbours are subtracted in camera space.
__device__ Ray pixel_ray(const Cam& cm, int px, int py) {
  Ray r;
  float c[3], ex[3], ey[3];
  const float u = (float)px + .5f, v = (float)py + .5f;
  camera_dir(cm, u, v, c);
  if (cm.has_dist != 0.f) {
    float cx[3], cy[3];
    camera_dir(cm, (float)(px + 1) + .5f, v, cx);           // the +x and +y neighbours for the cone radius
    camera_dir(cm, u, (float)(py + 1) + .5f, cy);
    ex[0] = cx[0] - c[0]; ex[1] = cx[1] - c[1]; ex[2] = 0.f;
    ey[0] = cy[0] - c[0]; ey[1] = cy[1] - c[1]; ey[2] = 0.f;
  } else {
    ex[0] = cm.p[0]; ex[1] = cm.p[3]; ex[2] = cm.p[6];
    ey[0] = cm.p[1]; ey[1] = cm.p[4]; ey[2] = cm.p[7];
  }
  float wx[3], wy[3];
  to_world(cm, c, r.d);
  to_world(cm, ex, wx);
  to_world(cm, ey, wy);
  r.o[0] = cm.c[3]; r.o[1] = cm.c[7]; r.o[2] = cm.c[11];
  const float nd = sqrtf(r.d[0] * r.d[0] + r.d[1] * r.d[1] + r.d[2] * r.d[2]);
  r.v[0] = r.d[0] / nd; r.v[1] = r.d[1] / nd; r.v[2] = r.d[2] / nd;
  const float dx_norm = sqrtf(wx[0] * wx[0] + wx[1] * wx[1] + wx[2] * wx[2]);
  const float dy_norm = sqrtf(wy[0] * wy[0] + wy[1] * wy[1] + wy[2] * wy[2]);
  r.radius = (0.5f * (dx_norm + dy_norm)) * 2.0f / 3.4641016151377544f;     // sqrt(12)
  return r;
}

// [n, 3] outputs through LDS: each thread stages its ray's three values, the block then writes its 3 * 256 floats as
// contiguous lanes (one 12-byte store per thread would touch three times as many cache-line pieces per instruction)
__device__ __forceinline__ void store3(float (*lds)[3 * TPB], int slot, const float a[3], float* __restrict__ out,
                                       int64_t ray0, int64_t n) {
  lds[slot][threadIdx.x * 3] = a[0];
  lds[slot][threadIdx.x * 3 + 1] = a[1];
  lds[slot][threadIdx.x * 3 + 2] = a[2];
  __syncthreads();
  const int64_t total = 3 * (n - ray0 < TPB ? n - ray0 : TPB);
  for (int j = threadIdx.x; j < total; j += TPB) out[ray0 * 3 + j] = lds[slot][j];
}

__device__ __forceinline__ void write_ray(float (*lds)[3 * TPB], const Ray& r, bool live, int64_t ray0, int64_t n,
                                          float* origins, float* directions, float* viewdirs, float* radii, float* near_out,
                                          float* far_out, float t_near, float t_far) {
  const int64_t i = ray0 + threadIdx.x;
  store3(lds, 0, r.o, origins, ray0, n);
  store3(lds, 1, r.d, directions, ray0, n);
  store3(lds, 2, r.v, viewdirs, ray0, n);
  if (live) {
    radii[i] = r.radius;
    near_out[i] = t_near;
    far_out[i] = t_far;
  }
}

__global__ __launch_bounds__(TPB) void frame_rays_kernel(const Cam* __restrict__ cams, int cam, int width, int64_t p0, int64_t n,
                                                        float t_near, float t_far, float* __restrict__ origins,
                                                        float* __restrict__ directions, float* __restrict__ viewdirs,
                                                        float* __restrict__ radii, float* __restrict__ near_out,
                                                        float* __restrict__ far_out) {
  __shared__ float lds[3][3 * TPB];
  const int64_t ray0 = (int64_t)blockIdx.x * TPB;
  const int64_t i = ray0 + threadIdx.x;
  const bool live = i < n;
  Ray r{};
  if (live) {
    const int64_t p = p0 + i;
    r = pixel_ray(cams[cam], (int)(p % width), (int)(p / width));
  }
  write_ray(lds, r, live, ray0, n, origins, directions, viewdirs, radii, near_out, far_out, t_near, t_far);
}

struct BatchArgs {
  const Cam* cams; int n_frames, H, W; uint64_t seed, counter; int64_t n;
  const uint8_t* rgb_u8; const float* depth_sup; const float* depth_gt; float t_near, t_far; int num_levels;
  float *origins, *directions, *viewdirs, *radii, *near_out, *far_out, *rgb, *sup_out, *gt_out; int32_t* pix; float* jitter01;
};

__global__ __launch_bounds__(TPB) void sample_batch_kernel(BatchArgs a) {
  __shared__ float lds[3][3 * TPB];
  const int64_t ray0 = (int64_t)blockIdx.x * TPB;
  const int64_t i = ray0 + threadIdx.x;
  const bool live = i < a.n;
  Ray r{};
  float c[3] = {0.f, 0.f, 0.f};
  if (live) {
    const Words w = philox(a.seed, a.counter, 0u, (uint32_t)i);
    const int cam = draw_below(w.w[0], a.n_frames), x = draw_below(w.w[1], a.W), y = draw_below(w.w[2], a.H);
    r = pixel_ray(a.cams[cam], x, y);
    const int64_t px = ((int64_t)cam * a.H + y) * a.W + x;
    // np.float32(u8 / 255.): the float64 quotient rounded once to float32
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) c[ch] = (float)((double)a.rgb_u8[px * 3 + ch] / 255.0);
    a.sup_out[i] = a.depth_sup[px];
    if (a.depth_gt) a.gt_out[i] = a.depth_gt[px];
    a.pix[i * 3] = cam; a.pix[i * 3 + 1] = x; a.pix[i * 3 + 2] = y;
    for (int l = 0; l < a.num_levels; ++l) a.jitter01[(int64_t)l * a.n + i] = unit_float(philox(a.seed, a.counter, 1u + l, (uint32_t)i).w[0]);
  }
  write_ray(lds, r, live, ray0, a.n, a.origins, a.directions, a.viewdirs, a.radii, a.near_out, a.far_out, a.t_near, a.t_far);
  __syncthreads();                                           // (the LDS slots are reused for the colours)
  store3(lds, 0, c, a.rgb, ray0, a.n);
}

// ---- distance percentiles (render.py:204-214) ------------------------------------------------------------------------
// t_aug = [tdist, t_far] (S + 2 edges), w_aug = [weights, max(0, 1 - acc)]; integrate_weights drops the last bin, so
// cw = [0, min(1, cumsum(weights)), 1] and the background weight never enters.  np.interp(p, cw, t_aug): j = the last
// edge with cw[j] <= p (cw is non-decreasing, cw[0] = 0 <= p < 1 = cw[S + 1]), then t[j] + slope * (p - cw[j]).
// A percentile inside a low-weight bin divides by a small cw[j + 1] - cw[j], so the prefix sums are formed in cumsum's
// sequential order (lane j adds the weights of lanes 0 .. j-1 one by one, read with shuffles; adding 0 beyond j changes no
// bit) and the interpolation is done in double, as np.interp does.
__global__ __launch_bounds__(256) void percentiles_kernel(int64_t n, int S, const float* __restrict__ tdist,
                                                          const float* __restrict__ weights, const float* __restrict__ t_far,
                                                          float* __restrict__ out) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int64_t ray = (int64_t)blockIdx.x * RPB + wave;
  if (ray >= n) return;
  const float w = lane < S ? weights[ray * S + lane] : 0.f;
  float excl = 0.f;
  for (int k = 0; k < S; ++k) {
    const float wk = __shfl(w, k, 64);
    excl += k < lane ? wk : 0.f;
  }
  // edge j = lane: cw[0] = 0, cw[j] = min(1, sum_{k<j} w_k) for 1 <= j <= S, cw[S + 1] = 1
  const float cw = lane == 0 ? 0.f : (lane <= S ? fminf(1.f, excl) : 1.f);
  const float t = lane <= S ? tdist[ray * (S + 1) + lane] : (lane == S + 1 ? t_far[ray] : 0.f);
  const double ps[3] = {0.05, 0.5, 0.95};
  float res[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const uint64_t below = __ballot(lane <= S + 1 && (double)cw <= ps[k]);
    const int j = __popcll(below) - 1;
    const double c0 = __shfl(cw, j, 64), c1 = __shfl(cw, j + 1, 64);
    const double t0 = __shfl(t, j, 64), t1 = __shfl(t, j + 1, 64);
    const double slope = (t1 - t0) / (c1 - c0);
    res[k] = (float)(slope * (ps[k] - c0) + t0);
  }
  if (lane < 3) out[ray * 3 + lane] = lane == 0 ? res[0] : (lane == 1 ? res[1] : res[2]);
}

}  // namespace mip360_rays

using namespace mip360_rays;

void mip360_launch_frame_rays(hipStream_t st, const float* cams, int cam, int width, int64_t p0, int64_t n, float t_near,
                              float t_far, float* origins, float* directions, float* viewdirs, float* radii, float* near_out,
                              float* far_out) {
  hipLaunchKernelGGL(frame_rays_kernel, dim3((unsigned)((n + TPB - 1) / TPB)), dim3(TPB), 0, st, (const Cam*)cams, cam, width, p0, n,
                     t_near, t_far, origins, directions, viewdirs, radii, near_out, far_out);
}

void mip360_launch_sample_batch(hipStream_t st, const float* cams, int n_frames, int H, int W, uint64_t seed, uint64_t counter,
                                int64_t n, const uint8_t* rgb_u8, const float* depth_sup, const float* depth_gt, float t_near,
                                float t_far, int num_levels, float* origins, float* directions, float* viewdirs, float* radii,
                                float* near_out, float* far_out, float* rgb, float* sup_out, float* gt_out, int32_t* pix,
                                float* jitter01) {
  BatchArgs a{(const Cam*)cams, n_frames, H, W, seed, counter, n, rgb_u8, depth_sup, depth_gt, t_near, t_far, num_levels,
              origins, directions, viewdirs, radii, near_out, far_out, rgb, sup_out, gt_out, pix, jitter01};
  hipLaunchKernelGGL(sample_batch_kernel, dim3((unsigned)((n + TPB - 1) / TPB)), dim3(TPB), 0, st, a);
}

void mip360_launch_distance_percentiles(hipStream_t st, int64_t n, int S, const float* tdist, const float* weights,
                                        const float* t_far, float* out) {
  hipLaunchKernelGGL(percentiles_kernel, dim3((unsigned)((n + RPB - 1) / RPB)), dim3(256), 0, st, n, S, tdist, weights, t_far, out);
}

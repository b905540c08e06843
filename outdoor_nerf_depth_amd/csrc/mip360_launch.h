// Host-side launchers of libmip360_hip.so: defined next to their kernels in the mip360_*.hip files, called from mip360_api.hip.
// Every file that defines one includes this header, so the compiler checks the definition against the declaration.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/mip360_hip.h"

void mip360_launch_resample(hipStream_t st, int n, int m_in, const float* sd, const float* w, float dil, float anneal,
                            float pad, int ns, const float* jit, float s_near, float s_far, const float* tn,
                            const float* tf, float* sd_out, float* td_out);
void mip360_launch_cast_encode(hipStream_t st, int n, int S, const float* td, const float* o, const float* d,
                               const float* radii, const float* basis_t, void* enc, int bf16, int ld);
void mip360_launch_render(hipStream_t st, int n, int S, const float* density, const float* rgbs, const float* td,
                          const float* dirs, int opaque, float bg, float* w, float* rgb, float* acc, float* dm, float* depth);
void mip360_launch_render_bwd(hipStream_t st, int n, int S, const float* density, const float* rgbs, const float* td,
                              const float* dirs, int opaque, float bg, const float* g_w, const float* g_rgb,
                              const float* g_dm, float* g_density, float* g_rgbs);
void mip360_launch_losses(hipStream_t st, int n, int s_nerf, int s_prop, int n_prop, const float* rgb, const float* rgb_gt,
                          const float* dm, const float* sup, const float* sd_nerf, const float* w_nerf,
                          const float* const* sd_prop, const float* const* w_prop, int charb, float charb_pad,
                          float data_mult, int depth_type, float lambda_depth, float depth_weight, float inter_mult,
                          float dist_mult, float* scalars, float* g_rgb, float* g_dm, float* g_w_nerf,
                          float* const* g_w_prop, float* ws, float prop_depth_weight, const float* const* dm_prop,
                          float* const* g_dm_prop);
void mip360_launch_depth_klurf(hipStream_t st, int type, int n, int S, const float* w, const float* td, const float* sup,
                               const float* dm, const float* dirs, float sigma, float scale, float* out, float* g_w,
                               float* g_dm, float* accum);
void mip360_launch_depth_rays(hipStream_t st, int type, int n, int n_levels, const int* S, const float* const* w,
                              const float* const* td, const float* sup, const float* const* dm, const float* dirs, float sigma,
                              const float* scale, float* values, float* const* g_w, float* const* g_dm, float* scalars,
                              float* ws);
int mip360_launch_linear_fm(hipStream_t st, int M, int N, int K, const void* A, int lda, const void* W, int ldw, const float* bias,
                            int act, void* C, int ldc, void* mask);
int mip360_launch_grad_weight_fm(hipStream_t st, int M, int I, int O, const void* H, int ldh, const void* dZ, int lddz, int ksplit,
                                 float* slabs, int ldc, float* bias_slabs);
int mip360_launch_grad_weight_fm_multi(hipStream_t st, int n, int M, int ksplit, const int* I, const int* O, const void* const* H, const int* ldh,
                                       const void* const* dZ, const int* lddz, float* const* slabs);
int mip360_launch_rowdot_fm(hipStream_t st, int M, int K, const void* A, int lda, const void* w, const float* bias, int act, float act_param,
                            float* out, int ldo);
int mip360_launch_grad_weight_col_fm(hipStream_t st, int M, int I, const void* H, int ldh, const void* dZ, int lddz, int zcol, int ksplit,
                                     float* slabs, int ldc, float* bias_slabs);
int mip360_launch_to_fm(hipStream_t st, int rows, int cols, const void* src, int ld_src, void* dst, int ld_dst, int col0_dst);
int mip360_launch_from_fm(hipStream_t st, int rows, int cols, const void* src, int ld_src, int col0_src, void* dst, int ld_dst);
void mip360_launch_linear(hipStream_t st, int M, int N, int K, const void* A, int lda, const void* W, int ldw, const float* bias,
                          int act, float act_param, void* C16, int ldc, float* C32, int ldc32, const void* aux, int ldaux,
                          void* mask, int ldmask);
bool mip360_grad_weight_is_wide(int M, int I, int O, int ldh, int lddz);
void mip360_launch_grad_weight_reduce(hipStream_t st, int rows, int I_slab, int O, int ksplit, const float* slabs, float* out, int ldc,
                                      float scale, float* bias_out);
void mip360_launch_grad_weight(hipStream_t st, int M, int I, int O, const void* H, int ldh, const void* dZ, int lddz, int ksplit,
                               float* slabs, float* out, int ldc, float scale, float* bias_out);
void mip360_launch_col_sum(hipStream_t st, int M, int O, const void* dZ, int ld, int nslice, float* partial, float* out,
                           float scale);
void mip360_launch_head_backward(hipStream_t st, int64_t rows, const float* density, const float* g_density, const float* rgb,
                                 const float* g_rgb, float pad, void* d_raw, int ld_raw, int raw_col, int raw_zero_to,
                                 void* d_pre);
void mip360_launch_sumsq(hipStream_t st, int64_t n, const float* g, float* partial, int nblocks);
void mip360_launch_clip_mult(hipStream_t st, int n_partial, const float* partial, float max_norm, float* out);
void mip360_launch_adam(hipStream_t st, int64_t n, float* p, const float* g, float* m, float* v, const float* gmult, float lr,
                        float b1, float b2, float eps, float bc1, float bc2);
void mip360_launch_pack_weight_batch(hipStream_t st, int n, const mip360_pack_desc* descs);
void mip360_launch_pack_weight(hipStream_t st, int n_in, int n_out, const float* k, void* fwd, int ld_fwd, void* bwd, int ld_bwd,
                               void* fwd_fm, int ld_fwd_fm, void* bwd_fm, int ld_bwd_fm, int bwd_rows, int bwd_col0);
int mip360_launch_outer_masked_fm(hipStream_t st, int M, int N, const void* z, const void* w, const void* mask, void* out, int ldc);
int mip360_launch_prop_mlp_fm(hipStream_t st, int rows, const void* x_fm, int ldx, int x_col0, const void* const* w_fm, const int* ldw,
                              const float* const* bias, void* const* h_fm, void* const* masks, const void* wd, const float* bd,
                              float act_param, float* density);
int mip360_launch_prop_mlp_bwd_fm(hipStream_t st, int rows, const void* z, const void* wd, const void* const* masks,
                                  const void* const* wb_fm, const int* ldwb, void* const* dz_fm);
int mip360_launch_view_branch_fm(hipStream_t st, int rows, int n_samples, const void* bott_fm, const void* dir_table, const void* w1_fm,
                                 int ldw1, const float* b1, const void* w2_fm, int ldw2, const float* b2, float rgb_padding,
                                 void* view_in, int ld_view, void* h, int ld_h, float* rgb);
int mip360_launch_view_branch_bwd_fm(hipStream_t st, int rows, const float* density, const float* g_density, const float* rgb,
                                     const float* g_rgb, float rgb_padding, const void* h, int ld_h, const void* wb3_fm, int ldwb3,
                                     const void* wb2_fm, int ldwb2, void* d_pre, void* d_hz, int ld_dhz, void* heads_fm);
void mip360_launch_dir_encode(hipStream_t st, int n, int S, const float* viewdirs, void* out, int ld, int col0, int width);
void mip360_launch_dir_glo_encode(hipStream_t st, int n, int S, const float* viewdirs, const float* embed, int E, int G,
                                  const int32_t* cam_idx, int cam_stride, void* out, int ld, int col0, int width);
void mip360_launch_glo_backward(hipStream_t st, int n_rays, int S, int G, int E, const void* d_hz, int ld_dhz, const void* wb_view,
                                int ld_wb, int row0, const int32_t* cam_idx, int cam_stride, float* partial, float* g_embed);
void mip360_launch_frame_rays(hipStream_t st, const float* cams, int cam, int width, int64_t p0, int64_t n, float t_near,
                              float t_far, float* origins, float* directions, float* viewdirs, float* radii, float* near_out,
                              float* far_out);
void mip360_launch_sample_batch(hipStream_t st, const float* cams, int n_frames, int H, int W, uint64_t seed, uint64_t counter,
                                int64_t n, const uint8_t* rgb_u8, const float* depth_sup, const float* depth_gt, float t_near,
                                float t_far, int num_levels, float* origins, float* directions, float* viewdirs, float* radii,
                                float* near_out, float* far_out, float* rgb, float* sup_out, float* gt_out, int32_t* pix,
                                float* jitter01);
void mip360_launch_distance_percentiles(hipStream_t st, int64_t n, int S, const float* tdist, const float* weights,
                                        const float* t_far, float* out);

// Host-side launchers, workspace queries and shape predicates of every kernel source, declared once: capi.hip calls
// them, and every source that defines one includes this header, so the compiler checks the definition against it.
// Default arguments appear here and nowhere else.
// cost_volume.hip, cost_volume_mfma.hip and warp.hip (and common.h) do NOT include it: _hip.source_sha256() hashes
// exactly those four files and profiles/traffic.json is stamped with that hash, so they stay byte-identical; their
// launchers (cost_volume_launch, warp_launch) are declared below all the same.
#pragma once
#include "common.h"

namespace qpwc {

// cost_volume.hip, warp.hip
int cost_volume_launch(const void* prv, const void* nxt, const void* flo, void* out, int B, int H, int W, int C, int r,
                       int layout, int dtype, int64_t ops, float slope, bool fuse, bool pad84, hipStream_t s);
int warp_launch(const void* img, const void* flo, void* out, int B, int H, int W, int C, int flo_bcast_mask, int layout,
                int dtype, int mode, hipStream_t s);

// epe.hip
int epe_workspace_floats();
int epe_launch(const float* a, const float* b, float* out, float* ws, int B, int H, int W, int layout, hipStream_t s);
int epe_multi_workspace_floats();
int epe_multi_launch(const void* const* a, const void* const* b, const int64_t* npix, const int64_t* plane,
                     const int* pred_dtype, int n_levels, float* out, float* ws, hipStream_t s);
int cost_volume_to_flow_launch(const void* cvol, float* flow, int B, int H, int W, int D, int64_t pix_stride, int layout,
                               int dtype, hipStream_t s);

// layout.hip
int layout_transpose_launch(const void* in, void* out, int B, int H, int W, int C, int to_layout, int dtype,
                            hipStream_t s);
int copy_pixels_launch(const void* src, void* dst, int B, int H, int W, int64_t row_bytes, int64_t sb, int64_t sy,
                       int64_t sx, int64_t db, int64_t dy, int64_t dx, hipStream_t s);

// optflow.hip (sepconv_x3.inc), sepconv_f16.hip, pointwise.hip
int dwconv3x3_launch(const void* const* srcs, const int* chans, const int64_t* strides, int n_src, int act,
                     const void* weight, void* out, int B, int H, int W, int dtype, hipStream_t s);
int sepconv3x3_launch(const void* const* srcs, const int* chans, const int64_t* strides, int n_src, int act,
                      const void* dw, const void* pw, const void* bias, void* out, int B, int H, int W, int F,
                      hipStream_t s);
int sepconv3x3_x3_launch(const void* const* srcs, const int* chans, const int64_t* strides, int n_src, int act,
                         const void* dw, const void* pw3, const void* bias, void* out, int B, int H, int W, int F,
                         hipStream_t s);
int sepconv3x3_f16_launch(const void* const* srcs, const int* chans, const int64_t* strides, int n_src, int act,
                          const void* dw, const void* pw, const void* bias, void* out, int B, int H, int W, int F,
                          hipStream_t s);
int pointwise_bias_launch(const void* y, const void* w, const void* bias, void* out, int64_t M, int C, int cpad, int F,
                          hipStream_t s);
int flow_head_param_floats();
int flow_head_launch(const void* z, const void* params, void* out, int B, int H, int W, float scale, int dtype,
                     int out_layout, hipStream_t s);
int flow_head_up_launch(const void* z, const void* params, void* out, void* out_up, void* out_up_f32, int B, int H,
                        int W, float scale, float up_scale, int dtype, hipStream_t s);
int optflow_tail_launch(const void* z2, const void* dw3, const void* pw3, const void* b3, const void* dw4,
                        const void* pw4, const void* b4, const void* head, void* out, int B, int H, int W, float scale,
                        int act_in, int out_layout, hipStream_t s);
int upsample2x_flow_launch(const void* in, void* out, int B, int h, int w, float scale, int dtype, int in_layout,
                           int out_layout, hipStream_t s);
int bias_mish_launch(void* x, const void* bias, int64_t n_pixels, int C, int dtype, hipStream_t s);
int bias_mish_pad_launch(const void* src, const void* bias, void* dst, int B, int H, int W, int C, int pad_h, int pad_w,
                         int64_t dst_pixel_stride, int dtype, hipStream_t s);
int split_frames_pad_launch(const void* in, void* out, int B, int H, int W, int pad_h, int pad_w, int dtype,
                            hipStream_t s);

// occlusion.hip
int invert_flow_launch(const void* flow, void* out, int B, int H, int W, int layout, int dtype, hipStream_t s);
int occlusion_launch(const void* flow, void* out, int B, int H, int W, int layout, int dtype, hipStream_t s);

// encoder.hip, encoder_x3.hip
int first_conv_mish_launch(const void* x, const void* weight, const void* bias, void* out, int B, int H, int W,
                           int layout, int dtype, hipStream_t s);
int conv3x3_mish_launch(const void* x, const void* weight, const void* bias, void* out, int B, int H, int W, int C,
                        int pad_h, int pad_w, hipStream_t s);
int conv3x3_mish_x3_launch(const void* x, const void* w3, const void* bias, void* out, int B, int H, int W, int C,
                           int pad_h, int pad_w, hipStream_t s);
int conv3x3_mish_f16_launch(const void* x, const void* weight, const void* bias, void* out, int B, int H, int W, int C,
                            int pad_h, int pad_w, hipStream_t s);
int conv3x3s2_mish_launch(const void* x, const void* weight, const void* bias, void* out, int B, int H, int W,
                          hipStream_t s);
int conv3x3s2_mish_any_launch(const void* x, const void* weight, const void* bias, void* out, int B, int H, int W,
                              int CI, hipStream_t s);
int conv3x3s2_mish_x3_launch(const void* x, const void* w3, const void* bias, void* out, int B, int H, int W, int CI,
                             hipStream_t s);
int conv3x3s2_mish_f16_launch(const void* x, const void* weight, const void* bias, void* out, int B, int H, int W,
                              int CI, hipStream_t s);
int upconv4x4s2_mish_launch(const void* x, const void* weight, const void* bias, void* out, int B, int H, int W, int C,
                            int F, int out_pixel_stride, hipStream_t s, const void* skip = nullptr,
                            int64_t skip_bs = 0, int64_t skip_rs = 0, int64_t skip_ps = 0);
int upconv4x4s2_mish_f16_launch(const void* x, const void* weight, const void* bias, void* out, int B, int H, int W,
                                int C, int F, int out_pixel_stride, hipStream_t s, const void* skip = nullptr,
                                int64_t skip_bs = 0, int64_t skip_rs = 0, int64_t skip_ps = 0);
int upconv4x4s2_mish_x3_launch(const void* x, const void* w3, const void* bias, void* out, int B, int H, int W, int C,
                               int F, int out_pixel_stride, hipStream_t s);
int split_bf16x3_launch(const void* src, void* out, int64_t n, hipStream_t s);

// backward.hip
int cost_volume_bwd_launch(const void* prv, const void* nxt, const void* out, const void* gout, void* gprv, void* gnxt,
                           int B, int H, int W, int C, int r, int dtype, float slope, hipStream_t s);
int warp_bwd_launch(const void* img, const void* flo, const void* gout, void* gimg, void* gflo, void* ws, int B, int H,
                    int W, int C, int dtype, int mode, hipStream_t s);

// loss.hip
int64_t loss_workspace_floats(int n_levels);
const char* loss_fwd_kernel(int kind, int H, int W, const int* h, const int* w, int n, const void* gt);
int loss_fwd_launch(int kind, float p0, float p1, const float* gt, int B, int H, int W, int C, int layout,
                    const void* const* pred, const int* h, const int* w, const int* pred_dtype, int n, float* out,
                    void* const* dpred, void* const* gt_out, float* ws, hipStream_t s);
int loss_bwd_launch(const void* const* dpred, const float* grad_losses, void* const* grad_pred, const int64_t* n_elems,
                    const int* pred_dtype, int n, hipStream_t s);

// sepconv_bwd.hip
int64_t sepconv3x3_bwd_workspace_floats(int B, int H, int W, int C, int F);
bool sepconv3x3_bwd_shape_ok(int B, int H, int W, int C, int F);
int sepconv3x3_bwd_launch(const void* const* srcs, const int* chans, const int64_t* strides, int n_src, int flags,
                          const void* dw, const void* pw, const void* bias, const void* gout, void* const* gsrc,
                          void* gdw, void* gpw, void* gbias, void* ws, int B, int H, int W, int F, hipStream_t s);

// conv_bwd.hip
int64_t conv3x3_same_bwd_workspace_floats(int B, int H, int W, int cin, int cout, int s);
bool conv3x3_same_shape_ok(int B, int H, int W, int cin, int cout, int s);
int conv3x3_same_fwd_launch(const void* x, const void* w, const void* bias, void* out, int B, int H, int W, int cin,
                            int cout, int stride, int mish, hipStream_t s);
int conv3x3_same_bwd_launch(const void* x, const void* w, const void* bias, const void* gout, void* gx, void* gw,
                            void* gb, void* ws, int B, int H, int W, int cin, int cout, int stride, int mish,
                            hipStream_t s);

// upconv_bwd.hip
int64_t upconv4x4s2_bwd_workspace_floats(int B, int H, int W, int C, int F);
bool upconv4x4s2_bwd_shape_ok(int B, int H, int W, int C, int F);
int upconv4x4s2_bwd_launch(const void* x, const void* w, const void* bias, const void* gout, int64_t gout_stride,
                           void* gx, void* gw, void* gb, void* ws, int B, int H, int W, int C, int F, int mish,
                           hipStream_t s);

// flow_head_bwd.hip
int64_t flow_head_stats_workspace_floats(int B, int H, int W);
int64_t flow_head_bwd_workspace_floats(int B, int H, int W);
int flow_head_stats_launch(const void* z, const void* w1, const void* b1, const void* gamma, const void* beta,
                           const void* wf, void* moving_mean, void* moving_var, float momentum, float eps, void* params,
                           void* stats, void* ws, int B, int H, int W, hipStream_t s);
int flow_head_bwd_launch(const void* z, const void* params, const void* stats, float eps, int training, float scale,
                         const void* gout, void* gz, void* gw1, void* gb1, void* ggamma, void* gbeta, void* gwf,
                         void* ws, int B, int H, int W, hipStream_t s);
int upsample2x_flow_bwd_launch(const void* gout, void* gin, int B, int h, int w, float scale, hipStream_t s);

// augment.hip
int64_t augment_workspace_floats(int B, int h, int w);
bool augment_shape_ok(int B, int H, int W, int h, int w);
const char* augment_fwd_kernel(int h, int w, const void* out_ims, const void* out_flo);
int augment_fwd_launch(const void* ims, bool u8, const float* flo, int B, int H, int W, const int* iparams,
                       const float* fparams, int h, int w, int flags, int layout, float* out_ims, float* out_flo,
                       float* ws, hipStream_t s);
// the sparse-ground-truth pipeline (include/qpwc_sparse_augment.h); out_align: what out_ims and out_flo must be aligned
// to in the form the shape takes, out_valid to a quarter of it
const char* augment_sparse_fwd_kernel(int h, int w);
size_t augment_sparse_out_align(int h, int w);
int augment_sparse_fwd_launch(const void* ims, bool u8, const float* flo, const unsigned char* valid, int B, int H, int W,
                              const int* iparams, const float* fparams, int h, int w, int flags, int layout,
                              float* out_ims, float* out_flo, unsigned char* out_valid, float* ws, hipStream_t s);

// interp.hip
int64_t image_head_bwd_workspace_floats(int64_t M);
int image_head_fwd_launch(const void* z, const void* w2, const void* b2, void* out, int64_t M, hipStream_t s);
int image_head_bwd_launch(const void* z, const void* w2, const void* gout, void* gz, void* gw2, void* gb2, void* ws,
                          int64_t M, hipStream_t s);
int upsample2x_image_launch(const void* in, void* out, int B, int h, int w, int C, float scale, hipStream_t s);
int upsample2x_image_bwd_launch(const void* gout, void* gin, int B, int h, int w, int C, float scale, hipStream_t s);
int avgpool_pyramid_max_levels();
int64_t avgpool_pyramid_tiles(int B, int H, int W, int levels, int* tw_out);
int avgpool_pyramid_launch(const void* x, void* out, int B, int H, int W, int C, int levels, hipStream_t s);

// optim.hip (include/qpwc_optim.h)
int64_t agc_adam_max_units();
const char* agc_adam_step_kernel(int64_t n_units);
int agc_adam_step_launch(const void* tensors, int n_tensors, const void* units, int64_t n_units, float alpha,
                         float beta1, float beta2, float epsilon, float clip_factor, float agc_eps, hipStream_t s);


// triplet.hip (include/qpwc_triplet.h)
const char* augment_triplet_fwd_kernel(int h, int w, const void* out_pair, const void* out_mid);
int augment_triplet_fwd_launch(const void* a, const void* b, const void* c, bool u8, int B, int H, int W,
                               const int* iparams, const float* fparams, int h, int w, int flags, int layout,
                               float* out_pair, float* out_mid, hipStream_t s);

// vis.hip (include/qpwc_vis.h)
bool flow_to_image_shape_ok(int n, int B, const int* h, const int* w, const int* oh, const int* ow);
int64_t flow_to_image_workspace_floats(int n, int B, const int* h, const int* w);
const char* flow_to_image_fwd_kernel(int n, const int* oh, const int* ow, const void* const* outs);
int flow_to_image_fwd_launch(const void* const* flows, const int* f16, const int* h, const int* w, int n, int B,
                             int in_layout, void* const* outs, const int* oh, const int* ow, bool u8, int out_layout,
                             float* ws, hipStream_t s);
struct VisMaxLevels;   // vis_common.h
int flow_mag_max_launch(const VisMaxLevels& m, int blocks, int in_layout, float* ws, hipStream_t s);

// quality.hip (include/qpwc_quality.h)
bool image_quality_shape_ok(int B, int H, int W, int C);
int64_t image_quality_workspace_floats(int B, int H, int W, int C);
const char* image_quality_fwd_kernel();
int image_quality_fwd_launch(const void* truth, bool f16_t, const void* pred, bool f16_p, int B, int H, int W, int C,
                             int layout, float off_t, float off_p, int flags, float max_val, float* out, double* state,
                             float* ws, hipStream_t s);

// masked_loss.hip (include/qpwc_masked_loss.h)
int64_t masked_loss_workspace_floats(int n_levels);
const char* masked_loss_fwd_kernel(int kind, int H, int W, const int* h, const int* w, int n);
int masked_loss_fwd_launch(int kind, float p0, float p1, const float* gt, const unsigned char* valid, int B, int H, int W,
                           int layout, const void* const* pred, const int* h, const int* w, const int* pred_dtype, int n,
                           float* out, int64_t* counts, void* const* dpred, void* const* gt_out, void* const* valid_out,
                           float* ws, hipStream_t s);
int masked_loss_bwd_launch(int kind, const void* const* dpred, const int64_t* counts, const float* grad_losses,
                           void* const* grad_pred, const int64_t* n_elems, const int* pred_dtype, int n, hipStream_t s);

// unsup_loss.hip (include/qpwc_unsup_loss.h)
int64_t unsup_loss_total_tiles(int B, const int* h, const int* w, int n);
int64_t unsup_loss_workspace_floats(int B, const int* h, const int* w, int n);
const char* unsup_loss_fwd_kernel(int kind);
int unsup_loss_fwd_launch(int kind, float q, float eps, float smooth_weight, float edge, float eps_s,
                          const void* const* prv, const void* const* nxt, const void* const* flow,
                          const void* const* occluded, int B, const int* h, const int* w, const int* flow_dtype,
                          int layout, int n, float* out_losses, float* out_photo, float* out_smooth, int64_t* out_counts,
                          float* ws, hipStream_t s);
int unsup_loss_bwd_launch(int kind, float smooth_weight, float eps_s, const void* const* flow, const float* ws,
                          const int64_t* counts, const float* grad_losses, void* const* grad_flow, int B, const int* h,
                          const int* w, const int* flow_dtype, int layout, int n, hipStream_t s);

// image_loss.hip (include/qpwc_image_loss.h)
int64_t image_loss_total_tiles(int B, const int* h, const int* w, int n);
int64_t image_loss_workspace_floats(int B, int C, const int* h, const int* w, int n);
const char* image_loss_fwd_kernel();
int image_loss_fwd_launch(float ssim_weight, float q, float eps, float max_val, float offset, const void* const* truth,
                          const void* const* pred, int B, int C, const int* h, const int* w, const int* pred_dtype,
                          int layout, int n, float* out_losses, float* out_dssim, float* out_charb, float* ws,
                          hipStream_t s);
int image_loss_bwd_launch(float ssim_weight, float q, float eps, float offset, const void* const* truth,
                          const void* const* pred, const float* ws, const float* grad_losses, void* const* grad_pred,
                          int B, int C, const int* h, const int* w, const int* pred_dtype, int layout, int n,
                          hipStream_t s);

// flow_quality.hip (include/qpwc_flow_quality.h)
bool flow_quality_shape_ok(int B, int H, int W);
int64_t flow_quality_workspace_floats(int B, int H, int W);
const char* flow_quality_fwd_kernel();
int flow_quality_fwd_launch(const float* truth, const void* pred, bool f16, const unsigned char* valid,
                            const unsigned char* occluded, int B, int H, int W, int layout, float out_abs,
                            float out_rel, float t0, float t1, float t2, float s0, float s1, float* out, double* state,
                            float* ws, hipStream_t s);

// review.hip (include/qpwc_review.h)
bool review_shape_ok(int n_flows, int B, int H, int W, int h, int w);
int64_t review_workspace_floats(int n_flows, int B, int h, int w);
bool review_panels_vec(int n_flows, int H, int W, int h, int w);
const char* review_panels_fwd_kernel(int n_flows, int H, int W, int h, int w);
int inference_panels_launch(const void* ims, bool f16, const float* flo, const float* flo_pred, int B, int H, int W,
                            int in_layout, void* const* outs, bool u8, int out_layout, int grid, float* ws,
                            hipStream_t s);
int interpolation_panels_launch(const void* img_pair, const void* img1, const void* pred, bool f16, const float* flow,
                                int B, int H, int W, int h, int w, int in_layout, void* const* outs, bool u8,
                                int out_layout, int grid, float* ws, hipStream_t s);

}  // namespace qpwc

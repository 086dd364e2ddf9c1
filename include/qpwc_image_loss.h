/* qpwc_image_loss.h -- the frame interpolator's structural training loss of libqpwc_hip.so: per level a weighted sum of
 * the structural dissimilarity (1 - SSIM) / 2 and a Charbonnier (smooth L1) term between a predicted image and its
 * target.  1..8 levels, each with its own target: one forward launch for all levels plus a fixed-order fold, one backward
 * launch.  The SSIM is qpwc_quality.h's (tf.image.ssim's defaults and no others), without clipping, so that the gradient
 * survives outside [0, max_val].
 * Goes beyond the reference, which trains the interpolator on AutoResizeMseLoss alone (qpwcnet/app/pre_train.py) and
 * scores it by SSIM.
 * The conventions and the QPWC_E_* codes are those of qpwc.h; "the first defect in this order" as qpwc_masked_loss.h.
 * Non-finite images are outside the contract: the result is unspecified, no access leaves a buffer.
 */
#ifndef QPWC_IMAGE_LOSS_H_
#define QPWC_IMAGE_LOSS_H_

#include "qpwc.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Floats of workspace qpwc_image_loss_fwd needs and qpwc_image_loss_bwd reads: 2 per tile of 16 x 32 pixels (the tile's
 * partial sums of s and of the Charbonnier term; tiles per level = B * ceil(h / 16) * ceil(w / 32)), then per level, in
 * level order, 3 planes of B * C * max(h - 10, 0) * max(w - 10, 0) floats (below).  A QPWC_E_* code (negative) for
 * arguments it refuses (QPWC_E_NULL, QPWC_E_SHAPE, by the rules below). */
int64_t qpwc_image_loss_workspace_floats(int B, int C, const int* h, const int* w, int n_levels);

/* truth[l]: fp32, the level's target; pred[l]: fp32 or fp16 by pred_dtype[l], widened to fp32 on load; both
 * (B,h[l],w[l],C) / (B,C,h[l],w[l]) by the one `layout`, dense.  All arithmetic is fp32 unless said otherwise, every
 * product and sum separately rounded except where an fmaf is named.  Per level, with t the target and p the prediction:
 *   vt = t + offset, vp = p + offset         (no clipping)
 *   g, conv, c1, c2   exactly those of qpwc_quality.h: the 11 taps of the sigma-1.5 Gaussian normalised in double and
 *                     rounded to fp32; conv the VALID depthwise correlation with g (x) g as a row pass (along w) followed
 *                     by a column pass, each an fmaf chain over k = 0..10 from 0; c1 = (0.01 max_val)^2 and
 *                     c2 = (0.03 max_val)^2 in double on the host, rounded to fp32
 *   mt = conv(vt), mp = conv(vp)
 *   A  = 2 mt mp + c1,                         Bd = mt^2 + mp^2 + c1
 *   Cn = 2 conv(vt vp) - 2 mt mp + c2,         D  = conv(vt^2 + vp^2) - (mt^2 + mp^2) + c2
 *   s  = (A / Bd) * (Cn / D)                   at each of the N = B * C * (h - 10) * (w - 10) positions
 *   dssim_l = (1 - mean s) / 2;                h < 11 or w < 11: N = 0, dssim_l = 0 and an all-zero SSIM gradient
 *   charb_l = the mean over all M = B * C * h * w elements of ((p - t)^2 + eps^2)^q     (powf)
 *   loss_l  = ssim_weight * dssim_l + (1 - ssim_weight) * charb_l
 * The means: fp32 partial sums per tile, folded in double in a fixed order; dssim_l, charb_l and loss_l are formed in
 * double and rounded to fp32.  out_losses, out_dssim, out_charb: float[n_levels].
 * Saved for the backward, in `workspace` behind the partial sums, per level 3 planes of (B,C,h-10,w-10) floats, with
 * l = A / Bd and cs = Cn / D at each position:
 *   Pa = 2 (mt - l mp) / Bd * cs + l * 2 (cs mp - mt) / D        d s / d mp
 *   Pb = -l cs / D                                               d s / d conv(vp^2)
 *   Pc = 2 l / D                                                 d s / d conv(vt vp)
 * Kernels: image_loss_fwd_kernel, one workgroup per (level, image, tile of 16 x 32 pixels) through a per-level prefix
 * table in its arguments; a tile owns the Charbonnier terms of its pixels and the SSIM positions with the same indices
 * (those below (h - 10, w - 10)); per channel the (16 + 10) x (32 + 10) patch of vt and vp goes through LDS, then the row
 * pass of the four quantities and the column pass.  Then image_loss_fold_kernel, one workgroup.  Grids depend on the
 * shapes only, sums are in a fixed order, no atomics: two calls give the same bits.  No form is chosen by alignment;
 * every global access is element-wise.  Extents up to 2^31 - 1 are indexed without a 32-bit sum that could wrap; a grid of
 * more workgroups than the HIP runtime launches answers QPWC_E_LAUNCH, nothing is enqueued.
 * `workspace` holds qpwc_image_loss_workspace_floats floats and needs no initialisation.
 * Errors, all before any HIP call, the first defect in this order: QPWC_E_NULL (truth, pred, h, w, pred_dtype, out_losses,
 * out_dssim, out_charb, workspace), QPWC_E_SHAPE (n_levels outside 1..8; C outside 1..4; an extent < 1; more than
 * 2^31 - 1 elements in a level or tiles in all), QPWC_E_LAYOUT, QPWC_E_RANGE (NaN anywhere; ssim_weight outside [0, 1];
 * q <= 0; eps <= 0; max_val <= 0 or not finite; offset not finite), QPWC_E_DTYPE, QPWC_E_NULL (a NULL truth[l] or
 * pred[l]), QPWC_E_ALIGN (truth 4 bytes, a pred its element size, out_losses, out_dssim, out_charb, workspace 4),
 * QPWC_E_ALIAS (an output or the workspace overlapping an input or another output). */
int qpwc_image_loss_fwd(float ssim_weight, float q, float eps, float max_val, float offset, const void* const* truth,
                        const void* const* pred, int B, int C, const int* h, const int* w, const int* pred_dtype,
                        int layout, int n_levels, void* out_losses, void* out_dssim, void* out_charb, void* workspace,
                        void* stream);

/* The forward kernel qpwc_image_loss_fwd takes for these arguments (host only): it has one, "image_loss_fwd_kernel"; ""
 * for arguments it refuses. */
const char* qpwc_image_loss_fwd_kernel(int B, int C, const int* h, const int* w, int n_levels);

/* grad_pred[l] = grad_losses[l] * d loss_l / d pred[l] in pred_dtype[l] and `layout`, every level in one launch
 * (image_loss_bwd_kernel, the forward's grid).  A gather: per pixel r and channel
 *   T.(r) = sum_j g(r_y - j_y) g(r_x - j_x) P.(j)   over the positions j with r - 10 <= j <= r on both axes, P. = 0
 *           outside the (h - 10) x (w - 10) positions, for each of Pa, Pb, Pc: the tile's patch of each plane with origin
 *           (tile origin - 10) goes through LDS, then a row pass and a column pass, fmaf chains over k = 0..10 from 0
 *   d loss_l / d p(r) = (-ssim_weight / (2 N)) * (Ta + 2 vp(r) Tb + vt(r) Tc)
 *                       + ((1 - ssim_weight) 2 q / M) * (p - t) ((p - t)^2 + eps^2)^(q - 1)
 * the two factors in parentheses formed in double and rounded to fp32; the sum is multiplied by grad_losses[l] last.
 * N = 0 or ssim_weight = 0: no SSIM term is formed; ssim_weight = 1: no Charbonnier term is formed.  No atomics, every
 * element of grad_pred is written exactly once.  truth, pred, workspace: what qpwc_image_loss_fwd read and wrote, with the
 * same parameters, shapes and layout; grad_losses (float[n_levels]) is read on the device.
 * Errors: QPWC_E_NULL (truth, pred, workspace, grad_losses, grad_pred, h, w, pred_dtype), QPWC_E_SHAPE, QPWC_E_LAYOUT,
 * QPWC_E_RANGE (ssim_weight, q, eps, offset as above), QPWC_E_DTYPE, QPWC_E_NULL (a NULL truth[l], pred[l] or
 * grad_pred[l]), QPWC_E_ALIGN (truth, workspace and grad_losses 4 bytes, a pred and a grad_pred its element size),
 * QPWC_E_ALIAS (a grad_pred overlapping an input or another grad_pred). */
int qpwc_image_loss_bwd(float ssim_weight, float q, float eps, float offset, const void* const* truth,
                        const void* const* pred, const void* workspace, const void* grad_losses, void* const* grad_pred,
                        int B, int C, const int* h, const int* w, const int* pred_dtype, int layout, int n_levels,
                        void* stream);

#ifdef __cplusplus
}
#endif
#endif /* QPWC_IMAGE_LOSS_H_ */

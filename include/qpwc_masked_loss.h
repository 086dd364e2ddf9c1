/* qpwc_masked_loss.h -- the flow training losses of libqpwc_hip.so over the valid pixels only: the masked twins of
 * qpwc_loss_fwd / qpwc_loss_bwd (qpwc.h) for FlowMseLossV2, FlowMseLoss and FlowMseLossFineTune, for ground truth that is
 * sparse (KITTI) or has unknown pixels (Sintel).  1..8 prediction levels against ONE full-resolution ground truth: one
 * forward launch for all levels plus a fixed-order fold, one backward launch.
 * Goes beyond the reference, whose losses are dense (qpwcnet/train/loss.py) and whose input pipeline sets non-finite
 * ground truth to zero instead (qpwcnet/app/optical_flow/train.py:88-92).
 * The conventions and the QPWC_E_* codes are those of qpwc.h; the validity rule is qpwc_flow_quality.h's.
 */
#ifndef QPWC_MASKED_LOSS_H_
#define QPWC_MASKED_LOSS_H_

#include "qpwc.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Floats of workspace qpwc_masked_loss_fwd needs: n_levels * 2048 partial sums and as many 32-bit partial counts
 * (n_levels * 4096); a QPWC_E_* code (negative) for arguments it refuses (QPWC_E_MODE, QPWC_E_NULL, QPWC_E_SHAPE, by the
 * rules below). */
int64_t qpwc_masked_loss_workspace_floats(int kind, int B, int H, int W, int C, const int* h, const int* w, int n_levels);

/* kind: QPWC_LOSS_FLOW_MSE_V2 (p0 = the Huber delta), QPWC_LOSS_FLOW_MSE or QPWC_LOSS_FLOW_FINETUNE (p0 = q, p1 = eps).
 * y_true: fp32 (B,H,W,2) / (B,2,H,W) by `layout`, dense.  valid: NULL, or dense uint8 (B,H,W).  y_pred[l]: fp32 or fp16
 * by pred_dtype[l], (B,h[l],w[l],2) / (B,2,h[l],w[l]) in the same layout; NULL (taken as zero) where gt_out[l] or
 * valid_out[l] is given.
 *   v(b,y,x)  = 1 iff |y_true| <= 1e9 in both components (false for NaN and +-inf) and, with a mask, valid[b,y,x] != 0.
 *               A pixel with v = 0 is selected out: whatever it holds reaches no arithmetic.
 * Per level pixel p, all in fp32:
 *   area kind (FLOW_MSE_V2; H % h == 0 and W % w == 0), over p's (H/h) x (W/w) block:
 *               n = sum v, m_p = (n >= 1), gt_p = (sum over the valid pixels of y_true / n) * ((float)h / (float)H)
 *               (masked_loss_tile_kernel forms sum * (((float)h / (float)H) / n): one division, and for a full block of a
 *               power-of-two area the dense loss's value bit for bit)
 *   bilinear kinds, the four corners of the half-pixel sample point, every product and sum separately rounded:
 *               fy = max(((float)H / h) * (y + 0.5f) - 0.5f, 0), y0 = (int)fy, y1 = min(y0 + 1, H - 1),
 *               ly1 = fy - y0, ly0 = 1 - ly1, the same along x; w_k = ly * lx of corner k;
 *               S = sum over the valid corners of w_k, m_p = (S > 0),
 *               gt_p = (sum over the valid corners of w_k * y_true_k / S) * ((float)h / (float)H)
 *   term_p    = the dense loss's per-pixel term of (gt_p, y_pred_p) where m_p (FLOW_MSE_V2: the sum of its two Huber
 *               terms of s * y_pred and s * gt, s = 2 / (w + h)); 0, with a derivative of exactly 0, where not -- also
 *               where the prediction there is NaN or Inf.
 *   count_l   = sum_p m_p over the batch, an exact integer
 *   loss_l    = sum_p term_p / max(count_l, 1); FLOW_MSE_V2 / (2 * max(count_l, 1)): the mean over elements
 * With every pixel valid loss_l and the gradients are the dense loss's to fp32 rounding; count_l = 0 gives loss_l = 0 and
 * an all-zero gradient.
 * out_losses: float[n_levels].  out_counts: int64[n_levels].  Per level, optional (the array NULL: none):
 *   dpred[l]     fp32, shaped like y_pred[l]: d term_p / d y_pred_p, NOT divided by the count (qpwc_masked_loss_bwd does
 *                that); every level's buffer when the array is given
 *   gt_out[l]    fp32, shaped like y_pred[l]: gt_p, 0 where m_p = 0; NULL entries are skipped
 *   valid_out[l] uint8 (B,h[l],w[l]): m_p; NULL entries are skipped
 * Kernels: masked_loss_tile_kernel for the area kind when H and W are multiples of 32 and the factors are nested powers of
 * two <= 32 with (H/h)(W/w) >= 4, none repeated -- y_true and the mask are read once for all levels; otherwise
 * masked_loss_pixel_kernel, one thread per level pixel; then masked_loss_fold_kernel.  Grids depend on the shapes only,
 * sums are in a fixed order, no atomics: two calls give the same bits.  No form is chosen by alignment.
 * `workspace` holds qpwc_masked_loss_workspace_floats floats and needs no initialisation.
 * Errors, all before any HIP call, the first defect in this order: QPWC_E_NULL (y_true, y_pred, pred_dtype, out_losses,
 * out_counts, workspace, h or w), QPWC_E_MODE (kind not one of the three; QPWC_LOSS_AUTORESIZE_MSE is refused),
 * QPWC_E_SHAPE (n_levels outside 1..8; an extent < 1; C != 2; more than 2^31 - 1 pixels per image at any resolution; the
 * area kind with H % h or W % w != 0), QPWC_E_LAYOUT, QPWC_E_RANGE (FLOW_MSE_V2 with delta < 0 or NaN), QPWC_E_DTYPE,
 * QPWC_E_NULL (a level with neither a prediction nor gt_out / valid_out; a NULL entry of a given dpred), QPWC_E_ALIGN
 * (y_true 16 bytes, valid 4, a prediction its element size, out_losses, workspace, dpred and gt_out 4, out_counts 8),
 * QPWC_E_ALIAS (an output or the workspace overlapping an input, the mask or another output). */
int qpwc_masked_loss_fwd(int kind, float p0, float p1, const void* y_true, const void* valid, int B, int H, int W, int C,
                         int layout, const void* const* y_pred, const int* h, const int* w, const int* pred_dtype,
                         int n_levels, void* out_losses, void* out_counts, void* const* dpred, void* const* gt_out,
                         void* const* valid_out, void* workspace, void* stream);

/* The forward kernel qpwc_masked_loss_fwd takes for these arguments (host only): "masked_loss_tile_kernel" or
 * "masked_loss_pixel_kernel"; "" for arguments it refuses. */
const char* qpwc_masked_loss_fwd_kernel(int kind, int B, int H, int W, int C, const int* h, const int* w, int n_levels);

/* grad_pred[l] = grad_losses[l] * dpred[l] / max(counts[l], 1) (FLOW_MSE_V2: / (2 * max(counts[l], 1))) in pred_dtype[l],
 * every level in one launch (masked_loss_bwd_kernel).  dpred and counts: what qpwc_masked_loss_fwd wrote, with the same
 * kind; counts is read on the device, the host never sees it.  grad_losses: float[n_levels] on the device.  n_elems[l]:
 * the elements of level l.
 * Errors: QPWC_E_NULL, QPWC_E_MODE, QPWC_E_SHAPE (n_levels outside 1..8, n_elems[l] < 1), QPWC_E_DTYPE, QPWC_E_ALIGN
 * (dpred[l] 16 bytes, grad_pred[l] 16 (fp32) / 8 (fp16), grad_losses 4, counts 8), QPWC_E_ALIAS (a grad_pred overlapping
 * dpred, counts, grad_losses or another grad_pred). */
int qpwc_masked_loss_bwd(int kind, const void* const* dpred, const void* counts, const void* grad_losses,
                         void* const* grad_pred, const int64_t* n_elems, const int* pred_dtype, int n_levels,
                         void* stream);

#ifdef __cplusplus
}
#endif
#endif /* QPWC_MASKED_LOSS_H_ */

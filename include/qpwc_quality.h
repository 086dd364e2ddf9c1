/* qpwc_quality.h -- image quality of libqpwc_hip.so: per-image MSE, PSNR and SSIM of a batch of predicted frames against
 * the true ones, in two launches, with an optional running sum on the device for an evaluation loop.
 * Replaces, for the frame interpolator,
 *     tf.image.psnr / tf.image.ssim (defaults) as metrics of InterpolatorModel       (qpwcnet/app/pre_train.py:71, :197)
 *     the 8-bit export `(255 * np.clip(x + 0.5, 0, 1)).astype(np.uint8)`            (qpwcnet/app/pre_train_test.py:61-77)
 * The conventions and the QPWC_E_* codes are those of qpwc.h.
 */
#ifndef QPWC_QUALITY_H_
#define QPWC_QUALITY_H_

#include "qpwc.h"

#ifdef __cplusplus
extern "C" {
#endif

/* flags of qpwc_image_quality_fwd; both together give what QPWC_QUALITY_U8 alone gives */
#define QPWC_QUALITY_CLIP 1 /* v = min(max(v, 0), max_val) */
#define QPWC_QUALITY_U8 2   /* v = truncf(255.0f * min(max(v, 0), 1)); max_val must be 255.0f */

/* Floats of workspace qpwc_image_quality_fwd needs: B * ceil((H - 10) / 16) * ceil((W - 10) / 32) * (C + 1), one sum of
 * s per channel and one sum of squared errors per (image, tile of 16 x 32 SSIM positions); a QPWC_E_* code (negative)
 * for arguments it refuses (QPWC_E_SHAPE, by the rules below). */
int64_t qpwc_image_quality_workspace_floats(int B, int H, int W, int C);

/* truth, pred: (B,H,W,C) / (B,C,H,W) by the one `layout`, dense, each fp32 or fp16 by its own dtype (QPWC_F32 /
 * QPWC_F16; fp16 is widened to fp32 first); they may be one buffer.  All arithmetic is fp32 unless said otherwise, every
 * product and sum below separately rounded except where an fmaf is named.  For image n, with t the truth and p the
 * prediction:
 *   value   v = x + offset  (offset_truth for t, offset_pred for p)
 *           QPWC_QUALITY_CLIP: v = min(max(v, 0), max_val)
 *           QPWC_QUALITY_U8  : v = truncf(255.0f * min(max(v, 0), 1)): the sum is rounded to fp32 before the product and
 *                              the product before the truncation (no fused multiply-add across them); the 8-bit export
 *                              of pre_train_test.py
 *   mse[n]  the mean of (vt - vp)^2 over all H * W * C elements: fp32 partial sums per tile (fmaf), folded in double
 *   psnr[n] = 20 log10(max_val) - 10 log10(mse[n]), in double from the double mse; +inf for mse == 0 (tf.image.psnr)
 *   ssim[n] tf.image.ssim's defaults and no others: filter_size 11, filter_sigma 1.5, k1 0.01, k2 0.03
 *           g[k] = exp(-(k - 5)^2 / 4.5) / sum_k exp(-(k - 5)^2 / 4.5), k = 0..10, in double on the host, rounded to fp32
 *           conv = the VALID depthwise correlation with g (x) g, as a row pass (along W) followed by a column pass, each
 *                  an fmaf chain over k = 0..10 from 0: (H - 10) x (W - 10) outputs per channel
 *           c1 = (0.01 max_val)^2, c2 = (0.03 max_val)^2, in double on the host, rounded to fp32
 *           mt = conv(vt), mp = conv(vp)
 *           num0 = 2 mt mp,  den0 = mt^2 + mp^2
 *           num1 = 2 conv(vt vp),  den1 = conv(vt^2 + vp^2)      (the sum of the squares is formed before the row pass)
 *           s = (num0 + c1) / (den0 + c1) * ((num1 - num0 + c2) / (den1 - den0 + c2))
 *           the mean of s over the (H - 10)(W - 10) positions of each channel, then over the C channels: fp32 partial
 *           sums per tile and channel, folded in double
 * out: float[3 * B]: out[n] = mse, out[B + n] = psnr, out[2 B + n] = ssim, each the double result rounded to fp32.
 * state: NULL, or double[4] = {sum of mse, sum of psnr, sum of ssim, images}: the second launch adds this call's B images
 * to it in image order, in double, each term the fp32 value it wrote to `out` (the count grows by B) -- the running mean
 * of an evaluation loop with no value read back per batch.  The caller zeroes it once.
 * Non-finite inputs are outside the contract: the result is unspecified, no access leaves a buffer.
 * Two launches, no atomics, nothing kept between calls except `state` (two runs on the same inputs are bit-identical; a
 * captured graph replays them unchanged): quality_tile_kernel, one workgroup per (image, tile of 16 x 32 SSIM positions),
 * all channels, writes its partial sums to `ws`; quality_fold_kernel, one workgroup, sums every image's partials in
 * tile order and writes `out` and `state`.  `ws` holds qpwc_image_quality_workspace_floats floats and needs no
 * initialisation.
 * Errors, all before any HIP call, the first defect in this order: QPWC_E_NULL (truth, pred, out or ws), QPWC_E_DTYPE,
 * QPWC_E_LAYOUT, QPWC_E_SHAPE (B < 1; C outside 1..4; H < 11 or W < 11; B * H * W * C or the workgroups of either launch
 * above 2^31 - 1), QPWC_E_RANGE (max_val not finite or <= 0; an offset not finite; QPWC_QUALITY_U8 with max_val != 255),
 * QPWC_E_MODE (flags outside 0..3), QPWC_E_ALIGN (inputs 4 bytes (fp32) / 2 (fp16), out and ws 4, state 8), QPWC_E_ALIAS
 * (out, ws or state overlapping an input or each other). */
int qpwc_image_quality_fwd(const void* truth, int truth_dtype, const void* pred, int pred_dtype, int B, int H, int W,
                           int C, int layout, float offset_truth, float offset_pred, int flags, float max_val,
                           void* out, void* state, void* ws, void* stream);

/* The tile kernel's form for this shape (host only): it has one, "quality_tile_kernel"; "" for arguments
 * qpwc_image_quality_fwd refuses. */
const char* qpwc_image_quality_fwd_kernel(int B, int H, int W, int C);

#ifdef __cplusplus
}
#endif
#endif /* QPWC_QUALITY_H_ */

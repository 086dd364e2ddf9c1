/* qpwc_flow_quality.h -- flow evaluation metrics of libqpwc_hip.so: per-image end-point error with its matched /
 * unmatched and speed splits, the KITTI outlier rate Fl-all, the accuracy at three thresholds and the average angular
 * error of a batch of predicted flows against the ground truth, over the valid pixels only, in two launches, with
 * optional running sums on the device for an evaluation loop.
 * Replaces, for the flow model,
 *     epe_error as a metric of `compile`                                  (qpwcnet/app/optical_flow/train.py:247-253, 299, 374)
 *     the scrubbing of non-finite ground truth that precedes it            (qpwcnet/app/optical_flow/train.py:88-92)
 * The conventions and the QPWC_E_* codes are those of qpwc.h.
 */
#ifndef QPWC_FLOW_QUALITY_H_
#define QPWC_FLOW_QUALITY_H_

#include "qpwc.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Floats of workspace qpwc_flow_quality_fwd needs: B * ceil(H * W / 4096) * 15, the partial sums of one (image, chunk of
 * 4096 consecutive pixels); a QPWC_E_* code (negative) for arguments it refuses (QPWC_E_SHAPE, by the rules below). */
int64_t qpwc_flow_quality_workspace_floats(int B, int H, int W);

/* truth (fp32), pred (fp32 or fp16 by pred_dtype: QPWC_F32 / QPWC_F16; fp16 is widened to fp32 first): (B,H,W,2) /
 * (B,2,H,W) by the one `layout`, dense; they may be one buffer.  valid, occluded: NULL, or dense uint8 (B,H,W).
 * All per-pixel arithmetic is fp32, every product and sum separately rounded (no fused multiply-add).  For a pixel with
 * ground truth (u, v) and prediction (u', v'):
 *   du = u - u', dv = v - v'
 *   e   = sqrtf(du du + dv dv)                                            the end-point error
 *   m   = sqrtf(u u + v v)                                                the ground-truth speed
 *   c   = u v' - v u'
 *   ang = atan2f(sqrtf((du du + dv dv) + c c), (u u' + v v') + 1) * 57.29577951308232f
 *         the angle in degrees between (u, v, 1) and (u', v', 1) in its well-conditioned form
 *   valid    iff |u| <= 1e9 and |v| <= 1e9 (false for NaN and +-inf: the .flo "unknown" convention and the non-finite
 *            pixels train.py scrubs) and, with a `valid` mask, valid[pixel] != 0
 *   outlier  iff e > out_abs and e > out_rel * m                          (KITTI Fl-all: 3 px and 5 %)
 *   accurate iff e < t0, e < t1, e < t2                                   (three counts)
 *   occluded iff an `occluded` mask is given and occluded[pixel] != 0
 *   speed bin 0: m < s0;  1: s0 <= m < s1;  2: m >= s1                    (Sintel: 10 and 40 px)
 * Per (image, chunk) the first launch sums, over the chunk's valid pixels only, 15 quantities in fp32 (the counts are
 * exact: a chunk has 4096 pixels), in this order:
 *   n_valid, sum e, sum ang, n_outlier, n_t0, n_t1, n_t2, n_occ, sum e (occluded), n_s0, sum e (bin 0), n_s1,
 *   sum e (bin 1), n_s2, sum e (bin 2)
 * and the second adds an image's chunks in double.
 * out: float[12 * B], quantity-major (out[q * B + n]), each value formed in double and rounded to fp32:
 *    0 epe      sum e / n_valid                  6 epe_noc  (sum e - sum e (occluded)) / (n_valid - n_occ)
 *    1 aae      sum ang / n_valid                7 epe_occ  sum e (occluded) / n_occ
 *    2 fl       n_outlier / n_valid              8 epe_s0   sum e (bin 0) / n_s0
 *    3 acc_t0   n_t0 / n_valid                   9 epe_s1   sum e (bin 1) / n_s1
 *    4 acc_t1   n_t1 / n_valid                  10 epe_s2   sum e (bin 2) / n_s2
 *    5 acc_t2   n_t2 / n_valid                  11 valid    n_valid / (H W)
 * A ratio over an empty set is NaN (0 / 0): without an `occluded` mask epe_noc == epe and epe_occ is NaN.
 * state: NULL, or double[17] = {the 15 sums above over every image seen, images, pixels}: the second launch adds this
 * call's images to state[0..14] in image order, in double, B to state[15] and B H W to state[16] -- the pixel-weighted
 * totals of an evaluation loop with no value read back per batch; every entry is additive over calls and over ranks.
 * The caller zeroes it once.
 * A non-finite prediction at a valid pixel is outside the contract: the result is unspecified, no access leaves a buffer.
 * Two launches, no atomics, nothing kept between calls except `state` (two runs on the same inputs are bit-identical; a
 * captured graph replays them unchanged): flow_quality_tile_kernel, one workgroup of 256 threads per (image, chunk of
 * 4096 consecutive pixels in the order y W + x, the lanes striding the chunk), writes its 15 partial sums to `ws` --
 * which lane sums which pixel does not depend on the layout, so both layouts give the same bits; flow_quality_fold_kernel,
 * one workgroup, a wave per image: lane l adds chunks l, l + 64, ... in chunk order in double, a wave reduction, then
 * `out` and `state`.  `ws` holds qpwc_flow_quality_workspace_floats floats and needs no initialisation.  The flows of
 * the (B,H,W,2) layout are loaded as one 8-byte (fp32) / 4-byte (fp16) pixel; no form is chosen by alignment.
 * Errors, all before any HIP call, the first defect in this order: QPWC_E_NULL (truth, pred, out or ws), QPWC_E_DTYPE,
 * QPWC_E_LAYOUT, QPWC_E_SHAPE (B, H or W < 1; B * H * W or the workgroups of either launch above 2^31 - 1), QPWC_E_RANGE
 * (any of the seven parameters not finite; out_abs, t0 or s0 <= 0; out_rel < 0; not t0 < t1 < t2; not s0 < s1),
 * QPWC_E_ALIGN ((B,H,W,2) flows 8 bytes (fp32) / 4 (fp16), (B,2,H,W) flows 4 / 2, out and ws 4, state 8), QPWC_E_ALIAS
 * (out, ws or state overlapping an input, a mask or each other). */
int qpwc_flow_quality_fwd(const void* truth, const void* pred, int pred_dtype, const void* valid, const void* occluded,
                          int B, int H, int W, int layout, float out_abs, float out_rel, float t0, float t1, float t2,
                          float s0, float s1, void* out, void* state, void* ws, void* stream);

/* The tile kernel's form for this shape (host only): it has one, "flow_quality_tile_kernel"; "" for arguments
 * qpwc_flow_quality_fwd refuses. */
const char* qpwc_flow_quality_fwd_kernel(int B, int H, int W);

#ifdef __cplusplus
}
#endif
#endif /* QPWC_FLOW_QUALITY_H_ */

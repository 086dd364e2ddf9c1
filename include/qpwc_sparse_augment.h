/* qpwc_sparse_augment.h -- the training input pipeline of libqpwc_hip.so for sparse ground truth: qpwc_augment_fwd
 * (qpwc.h) with a flow that is resampled over its valid pixels only and a level-0 validity mask beside it, for KITTI's
 * sparse flow and Sintel's unknown pixels.  One launch, two with the colour stage; nothing is read back to the host.
 * Goes beyond the reference, whose input pipeline is dense: it resamples the flow with the frames' bilinear and sets
 * non-finite ground truth to zero afterwards (qpwcnet/app/optical_flow/train.py:88-92).
 * The conventions and the QPWC_E_* codes are those of qpwc.h; the validity rule is qpwc_flow_quality.h's, the weights
 * over the valid corners are qpwc_masked_loss.h's bilinear rule.
 */
#ifndef QPWC_SPARSE_AUGMENT_H_
#define QPWC_SPARSE_AUGMENT_H_

#include "qpwc.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ims, ims_dtype, flo, B, H, W, iparams, fparams, h, w, flags, layout, out_ims and workspace: those of qpwc_augment_fwd,
 * and out_ims has its bits.  workspace: qpwc_augment_workspace_floats(B, h, w) floats, read and written with
 * QPWC_AUGMENT_COLOR only.  valid: NULL, or dense uint8 (B,H,W).
 *   v(b,y,x)  = 1 iff |flo| <= 1e9 in both components (false for NaN and +-inf) and, with a mask, valid[b,y,x] != 0.
 *               A pixel with v = 0 is selected out: whatever it holds reaches no arithmetic and changes no output bit.
 * Per output pixel the four corners 00, 01, 10, 11 (row, column) and the weights tx, ty are qpwc_augment_fwd's: the
 * clamped floor and ceil of the fp32 source coordinate along each axis, the flips applied to the indices.  n = the
 * number of corners with v = 1 (a corner that a clamp or t = 0 makes the same pixel twice counts twice), all in fp32,
 * every product and sum separately rounded:
 *   n = 4       (u, v) = the bilinear value of qpwc_augment_fwd times (mu, mv): the dense pipeline's bits
 *   1 <= n <= 3 w_k = ly_k * lx_k, ly_0 = 1 - ty, ly_1 = ty, lx_0 = 1 - tx, lx_1 = tx; S = the sum of w_k over the
 *               valid corners in the order 00, 01, 10, 11; (u, v) = (the sum of w_k * flo_k in that order) / S times
 *               (mu, mv).  S > 0: a corner's weight is 0 only where t = 0, and there its neighbour is the same pixel.
 *   n = 0       (u, v) = (0, 0)
 * out_flo: fp32 (B,h,w,2) / (B,2,h,w) by `layout`: finite where out_valid is 1, exactly 0 where it is 0; it takes no NaN
 * scrub, and QPWC_AUGMENT_RAW changes the frames only.  out_valid: uint8 (B,h,w) in both layouts, 1 iff n >= 1: what
 * qpwc_masked_loss_fwd and qpwc_flow_quality_fwd take as `valid`.
 * Kernels: augment_sparse_pixel_kernel, one output pixel per lane and 256 per workgroup, in the <vec4> form when
 * h * w % 4 == 0 (the outputs leave through LDS as 16-byte pieces, the mask as 4-byte pieces) and in the <scalar> form
 * otherwise; then augment_contrast_kernel with QPWC_AUGMENT_COLOR.  The form depends on the shape only, never on an
 * address; no atomics: two calls give the same bits.
 * Errors, all before any HIP call, the first defect in this order: QPWC_E_MODE (unknown flags), QPWC_E_NULL (ims, flo,
 * iparams, fparams, out_ims, out_flo, out_valid; workspace with QPWC_AUGMENT_COLOR), QPWC_E_DTYPE (ims_dtype not
 * QPWC_U8 or QPWC_F32), QPWC_E_LAYOUT, QPWC_E_SHAPE (an extent < 1; a pixel count or the launch grid overflowing 32
 * bits), QPWC_E_ALIGN (ims 2 bytes (uint8) / 8 (fp32), flo 8, iparams, fparams and workspace 4; out_ims and out_flo 16
 * and out_valid 4 in the <vec4> form, 4 and 1 in the <scalar> form), QPWC_E_ALIAS (an output or the workspace
 * overlapping an input, the mask, or another output: out_valid against every one of them). */
int qpwc_augment_sparse_fwd(const void* ims, int ims_dtype, const void* flo, const void* valid, int B, int H, int W,
                            const void* iparams, const void* fparams, int h, int w, int flags, int layout, void* out_ims,
                            void* out_flo, void* out_valid, void* workspace, void* stream);

/* The form of qpwc_augment_sparse_fwd's first launch for a (h, w) output (host only):
 * "augment_sparse_pixel_kernel<vec4>" or "augment_sparse_pixel_kernel<scalar>"; "" for shapes it refuses. */
const char* qpwc_augment_sparse_fwd_kernel(int B, int h, int w);

#ifdef __cplusplus
}
#endif
#endif /* QPWC_SPARSE_AUGMENT_H_ */

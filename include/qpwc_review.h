/* qpwc_review.h -- the inference review panels of libqpwc_hip.so: every picture the reference's two test scripts show
 * for a batch, from the network's tensors, in two launches per call.
 * Replaces
 *     the ten pictures of qpwcnet/app/optical_flow/test_infer.py:104-154            (qpwc_inference_panels_fwd)
 *     the seven pictures of qpwcnet/app/frame_interpolation/pre_train_test.py:45-79, 121-163, with _show's alignment
 *     grid and its 8-bit export                                                     (qpwc_interpolation_panels_fwd)
 * built there from tf_warp (qpwcnet/core/warp.py:100-151), flow_to_image (qpwcnet/core/vis.py:37-76) and element-wise
 * arithmetic.  The conventions and the QPWC_E_* codes are those of qpwc.h.
 *
 * Common to both entry points.  All arithmetic is fp32 with separately rounded products and sums; fp16 images are
 * widened first.  Flows are fp32 only (coordinates need the precision); channel 0 is fx, channel 1 is fy.
 *   tf_warp(img, f) at pixel (Y, X) of an H x W image, exactly QPWC_WARP_TFWARP of qpwc_warp_fwd:
 *       x = (float)X + fx,  y = (float)Y + fy
 *       x0 = (int)x, y0 = (int)y (truncation toward zero), x1 = x0 + 1, y1 = y0 + 1, each then clipped to [0, W-1] /
 *       [0, H-1]; the four raw weights are taken from the CLIPPED corners and do not sum to one outside the image:
 *       wa = (x1 - x) * (y1 - y), wb = (x1 - x) * (y - y0), wc = (x - x0) * (y1 - y), wd = (x - x0) * (y - y0)
 *       out = ((wa * img[y0,x0] + wb * img[y1,x0]) + wc * img[y0,x1]) + wd * img[y1,x1]        (a, b, c, d)
 *   flow_to_image(f): exactly as qpwc_vis.h states it, by the same device code: per-image maximum of
 *       sqrtf(fmaf(fx, fx, fy * fy)) at the flow's own size, s = mag / (smax + 1e-6f), hue from atan2f, TensorFlow's
 *       HSV functor at v = 1, rgb = (1 - s) + s * d.
 *   grid: 0 = none; g > 0: after the values above, every element of rows 0, g, 2g, ... and of columns 0, g, 2g, ... of
 *       every picture is exactly 1.0f; the period counts the picture's own pixels (_show uses 32).
 *   outs[k] (B,oh,ow,3) / (B,3,oh,ow) by `out_layout`, written in that layout by the kernel:
 *       QPWC_F32: the values, unclipped;
 *       QPWC_U8 : (uint8) truncf(255.0f * min(max(x, 0), 1)), _show's export and the rule of QPWC_QUALITY_U8 -- not the
 *                 255.5 rule of qpwc_flow_to_image_fwd.  The grid is drawn before it.
 *   Non-finite values are outside the contract: the result is unspecified, no access leaves a buffer.
 *   Two launches, no atomics, no value read back and no state kept between calls (a captured graph replays them
 *   unchanged; two runs are bit-identical): flow_mag_max_kernel writes one partial maximum per (flow, image, tile of
 *   2048 flow pixels) to `ws`; review_panels_kernel folds the partials of its image and writes every picture of a tile
 *   of 256 pixels.  `ws` holds qpwc_review_workspace_floats floats and needs no initialisation.
 *   Store form, chosen from the shape alone: "review_panels_kernel<vec4>" when every picture's pixel count per image
 *   (H * W, and h * w for 5-flow) is a multiple of 4 -- a workgroup's pixels leave through LDS in the picture's own
 *   memory order, as 16-byte stores for fp32 and as packed dwords for uint8 -- else "review_panels_kernel<scalar>", one
 *   element per store.
 *   Alignment: images their element size (4 fp32 / 2 fp16), flows 4, ws 4; outputs 16 (fp32) / 4 (uint8) in the <vec4>
 *   form and 4 (fp32) / 1 (uint8) in the <scalar> form.  An output off that grid is refused with QPWC_E_ALIGN; the
 *   kernel never looks at a pointer's low bits.
 *   Errors, in this order and all before any HIP call: QPWC_E_NULL (a pointer, `outs` or one of its elements),
 *   QPWC_E_DTYPE (images not F32 / F16, outputs not F32 / U8), QPWC_E_LAYOUT, QPWC_E_SHAPE (an extent < 1; H != s * h or
 *   W != s * w for one integer s >= 1; grid < 0; 6 * B * H * W, or the workgroups of either launch, above 2^31 - 1),
 *   QPWC_E_ALIGN, QPWC_E_ALIAS (an output overlapping an input, ws or another output; ws overlapping an input).  The
 *   inputs are only read and may overlap one another. */
#ifndef QPWC_REVIEW_H_
#define QPWC_REVIEW_H_

#include "qpwc.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Floats of workspace for n_flows (2: qpwc_inference_panels_fwd, 1: qpwc_interpolation_panels_fwd) flows of h x w:
 * n_flows * B * ceil(h * w / 2048); a QPWC_E_* code (negative) for arguments it refuses. */
int64_t qpwc_review_workspace_floats(int n_flows, int B, int h, int w);

/* test_infer.py.  ims (B,H,W,6) / (B,6,H,W) by `in_layout`, F32 or F16 by ims_dtype, preprocessed (- 0.5): channels 0-2
 * are prv, 3-5 are nxt.  flo (the ground truth), flo_pred (B,H,W,2) / (B,2,H,W), fp32.  outs[0..9], each H x W:
 *   0 prv               0.5f + ims[0:3]
 *   1 nxt               0.5f + ims[3:6]
 *   2 nxt_w             0.5f + tf_warp(ims[3:6], flo_pred): the warp acts on the offset image, 0.5 is added afterwards
 *   3 overlay           0.5f * prv + 0.5f * nxt
 *   4 overlay_warped    0.5f * prv + 0.5f * nxt_w
 *   5 overlay_warped_gt 0.5f * prv + 0.5f * nxt_w_gt,   nxt_w_gt = 0.5f + tf_warp(ims[3:6], flo)
 *   6 delta_warped      fabsf(0.5f * prv - 0.5f * nxt_w)
 *   7 delta_warped_gt   fabsf(0.5f * prv - 0.5f * nxt_w_gt)
 *   8 flo_rgb           flow_to_image(flo)
 *   9 flo_pred_rgb      flow_to_image(flo_pred)
 * ws: qpwc_review_workspace_floats(2, B, H, W) floats. */
int qpwc_inference_panels_fwd(const void* ims, int ims_dtype, const void* flo, const void* flo_pred, int B, int H, int W,
                              int in_layout, void* const* outs, int out_dtype, int out_layout, int grid, void* ws,
                              void* stream);

/* pre_train_test.py.  img_pair (B,H,W,6) / (B,6,H,W), preprocessed (- 0.5); img1 (B,H,W,3) / (B,3,H,W), the ground-truth
 * middle frame in [0, 1]; pred, img1's shape, the model's output (- 0.5); all three F32 or F16 by img_dtype.  flow
 * (B,h,w,2) / (B,2,h,w), fp32, with H = s * h and W = s * w for one integer s >= 1 (the script: s = 2).  outs[0..6]:
 *   0 0-prv          0.5f + img_pair[0:3]
 *   1 1-nxt          0.5f + img_pair[3:6]
 *   2 2-ground-truth img1
 *   3 3-pred         0.5f + pred
 *   4 4-overlay      0.5f * (0-prv) + 0.5f * (1-nxt)
 *   5 5-flow         flow_to_image(flow) at the flow's own size: (B,h,w,3) / (B,3,h,w); its grid counts its own pixels
 *   6 6-warp         tf_warp(img1, upflow), upflow[Y, X] = (float)s * flow[Y / s, X / s] (einops.repeat, times s); no
 *                    offset.  The script's key for it is '6-warp(==0-prv)'.
 * All but 5-flow are H x W.  ws: qpwc_review_workspace_floats(1, B, h, w) floats. */
int qpwc_interpolation_panels_fwd(const void* img_pair, const void* img1, const void* pred, int img_dtype,
                                  const void* flow, int B, int H, int W, int h, int w, int in_layout, void* const* outs,
                                  int out_dtype, int out_layout, int grid, void* ws, void* stream);

/* The store form of the panel launch for these shapes (host only): "review_panels_kernel<vec4>" or
 * "review_panels_kernel<scalar>" as stated above; n_flows = 2 (then h = H, w = W) or 1; "" for arguments the entry
 * points refuse. */
const char* qpwc_review_panels_fwd_kernel(int n_flows, int B, int H, int W, int h, int w, int out_dtype, int out_layout);

#ifdef __cplusplus
}
#endif
#endif /* QPWC_REVIEW_H_ */

/* qpwc_vis.h -- the trainer's flow panels of libqpwc_hip.so: 1..8 flows of different sizes coloured by direction and
 * relative magnitude, nearest-resized and converted for display, in two launches for all of them together.
 * Replaces, per logging step,
 *     flow_to_image                                                                  (qpwcnet/core/vis.py:37-76)
 *     tf.image.resize(..., NEAREST_NEIGHBOR) of every picture to the label's size and tf.summary.image's
 *     convert_image_dtype(uint8, saturate=True)        (qpwcnet/app/train.py ShowImageCallback / train_custom)
 * The conventions and the QPWC_E_* codes are those of qpwc.h.
 */
#ifndef QPWC_VIS_H_
#define QPWC_VIS_H_

#include "qpwc.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Floats of workspace qpwc_flow_to_image_fwd needs for these flows: B * sum of ceil(h[l] * w[l] / 2048); a QPWC_E_*
 * code (negative) for arguments it refuses. */
int64_t qpwc_flow_to_image_workspace_floats(int n, int B, const int* h, const int* w);

/* flows[l] (B,h[l],w[l],2) / (B,2,h[l],w[l]) by `in_layout`, dense, fp32 or fp16 by flow_dtype[l] (fp16 is widened to
 * fp32 first); channel 0 is fx, channel 1 is fy.  Two flows may be one buffer.  All arithmetic is fp32.  For image n of
 * level l and the source pixel (sy, sx) of output pixel (Y, X):
 *   ang  = atan2f(fy, fx),  hue = (ang + float32(pi)) / float32(2 pi)
 *   mag  = sqrtf(fmaf(fx, fx, fy * fy))
 *   smax = max of mag over the h[l] * w[l] pixels of image n, at the flow's own size (before any resize)
 *   s    = mag / (smax + 1e-6f): an all-zero image has s = 0 and is white; nothing divides by zero
 *   HSV -> RGB with v = 1, in the form of TensorFlow's functor:
 *          dh = 6 * hue,  dr = clamp(|dh - 3| - 1, 0, 1),  dg = clamp(2 - |dh - 2|, 0, 1),  db = clamp(2 - |dh - 4|, 0, 1)
 *          rgb = (1 - s) + s * d
 *   nearest resize to (oh[l], ow[l]) by TF2's rule for tf.image.resize(..., NEAREST_NEIGHBOR):
 *          sy = min((int)floorf((Y + 0.5f) * ((float)h / oh)), h - 1), sx likewise: the identity for oh == h, ow == w.
 * outs[l] (B,oh[l],ow[l],3) / (B,3,oh[l],ow[l]) by `out_layout`, written in that layout by the kernel:
 *   QPWC_F32: the values above;
 *   QPWC_U8 : (uint8) min(max(truncf(x * 255.5f), 0), 255), the rule of tf.image.convert_image_dtype(saturate=True).
 * Non-finite flow values are outside the contract: the result is unspecified, no access leaves a buffer.
 * Two launches, no atomics and no state kept between calls (a captured graph replays them unchanged; two runs are
 * bit-identical): flow_mag_max_kernel writes one partial maximum per (level, image, tile of 2048 source pixels) to `ws`,
 * flow_to_image_kernel folds the partials of its (level, image) and colours a tile of 1024 output pixels.  `ws` holds
 * qpwc_flow_to_image_workspace_floats floats and needs no initialisation.
 * Alignment: flows 4 bytes (fp32) / 2 (fp16), fp32 outputs 4, uint8 outputs 1, ws 4.  Errors, in this order and all
 * before any HIP call: QPWC_E_NULL (an array, an element of flows / outs, or ws), QPWC_E_DTYPE (a flow that is not F32 /
 * F16, an output type that is not F32 / U8), QPWC_E_LAYOUT, QPWC_E_SHAPE (n outside 1..8; an extent < 1; 2 * B * h * w
 * or 3 * B * oh * ow of a level, or the workgroups of either launch, above 2^31 - 1), QPWC_E_ALIGN, QPWC_E_ALIAS (ws or
 * an output overlapping a flow; an output overlapping ws or another output). */
int qpwc_flow_to_image_fwd(const void* const* flows, const int* flow_dtype, const int* h, const int* w, int n, int B,
                           int in_layout, void* const* outs, const int* oh, const int* ow, int out_dtype,
                           int out_layout, void* ws, void* stream);

/* The store form of qpwc_flow_to_image_fwd for these outputs (host only): "flow_to_image_kernel<vec4>" (every level's
 * oh * ow a multiple of 4 and every output 16-byte aligned: a workgroup's pixels leave through LDS in the output's own
 * memory order, as 16-byte stores for fp32 and as packed dwords for uint8) or "flow_to_image_kernel<scalar>" (one
 * element per store); "" for arguments it refuses. */
const char* qpwc_flow_to_image_fwd_kernel(int n, int B, const int* oh, const int* ow, int out_dtype, int out_layout,
                                          const void* const* outs);

#ifdef __cplusplus
}
#endif
#endif /* QPWC_VIS_H_ */

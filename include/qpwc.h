/* qpwc.h -- C ABI of libqpwc_hip.so: the MI355X (gfx950) hot path of qpwcnet.
 *
 * The reference (yycho0108/qpwcnet) has no FFI layer of its own: its boundary
 * is the Python Keras-layer call() surface, and one level down the registered
 * TensorFlow op of tensorflow-addons.  Each entry point below names the
 * reference interface it replaces (paths relative to the reference checkout).
 *
 * Conventions
 *   - plain pointers and sizes only; every pointer is a DEVICE pointer;
 *   - the caller owns all memory; kernels never allocate, free or retain;
 *   - `out` must not overlap an input;
 *   - work is enqueued on `stream` (a hipStream_t passed as void*, NULL = the
 *     default stream) and the call returns without synchronising;
 *   - return value 0 = enqueued, negative = QPWC_E_* (nothing was enqueued);
 *     qpwc_last_error() returns a thread-local description of the last failure.
 */
#ifndef QPWC_H_
#define QPWC_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define QPWC_VERSION 200 /* 0.2.0 */

/* layout of every image-like tensor of one call */
#define QPWC_NHWC 0 /* 'channels_last'  (B,H,W,C) */
#define QPWC_NCHW 1 /* 'channels_first' (B,C,H,W) */

/* storage dtype; arithmetic is always fp32 */
#define QPWC_F32 0
#define QPWC_F16 1
#define QPWC_U8 2 /* source frames of qpwc_augment_fwd only: uint8 0..255 */

/* warp border semantics */
#define QPWC_WARP_CLAMP 0  /* WarpV2: tfa dense_image_warp, clamp-to-border */
#define QPWC_WARP_TFWARP 1 /* Warp  : qpwcnet tf_warp (truncate, clip, raw weights) */

/* flo_bcast_mask bits: set = that flow dimension has extent 1 and is broadcast */
#define QPWC_BCAST_B 1
#define QPWC_BCAST_H 2
#define QPWC_BCAST_W 4

#define QPWC_OK 0
#define QPWC_E_NULL (-1)     /* null pointer */
#define QPWC_E_LAYOUT (-2)   /* 'Unsupported data format' (layers.py:19-29) */
#define QPWC_E_DTYPE (-3)    /* unsupported dtype code */
#define QPWC_E_SHAPE (-4)    /* non-positive extent, or H/W < 2 for clamp warp (warp.py:182-184) */
#define QPWC_E_RANGE (-5)    /* search_range < 0 or too large */
#define QPWC_E_MODE (-6)     /* unknown warp mode */
#define QPWC_E_ALIAS (-7)    /* out overlaps an input */
#define QPWC_E_LAUNCH (-8)   /* hipGetLastError() after launch; see qpwc_last_error() */
#define QPWC_E_ALIGN (-9)    /* pointer not aligned to its element size */
#define QPWC_E_STRIDE (-10)  /* output stride/offset cannot hold the result */
#define QPWC_E_NODEVICE (-11)/* no HIP device / runtime error before launch */

int qpwc_version(void);
const char* qpwc_last_error(void);
const char* qpwc_strerror(int code);
/* Static description of the build.  The library selects kernels from the call's arguments only (no
 * environment variable changes what runs; the experimental build that did is removed after 784aa79, see git history). */
const char* qpwc_build_info(void);

/* Layout conversion at the boundary: out = in with the same logical (B,H,W,C) content in `to_layout`
 * (in is in the other layout).  The reference picks its layout from image_data_format()
 * (qpwcnet/core/layers.py:41,146; NCHW handled by transposing in and out, layers.py:179-183); the hot-path
 * kernels are channels-last, so a dense 'channels_first' tensor crosses the boundary through this kernel. */
int qpwc_layout_transpose_fwd(const void* in, void* out, int B, int H, int W, int C, int to_layout, int dtype,
                              void* stream);

/* dst view = src view for two channels-last (B,H,W,C) views with their own strides (elements, order batch / row /
 * pixel; channels contiguous): the skip half of the decoder's concat([UpConv(x), skip])
 * (qpwcnet/core/pwcnet.py:186-195), which the reference leaves to tf.concat.  C * element size and every stride
 * must be whole 16-byte units, both base pointers 16-byte aligned, the two extents disjoint. */
int qpwc_copy_pixels_fwd(const void* src, void* dst, int B, int H, int W, int C, const int64_t* src_strides,
                         const int64_t* dst_strides, int dtype, void* stream);

/* Measurement aid ("measure the achievable ceiling on the box with a device copy
 * kernel"): dst[0..bytes) = src[0..bytes), 16 B per lane, bytes % 16 == 0, both 16-byte aligned.
 * Not part of the reference's surface. */
int qpwc_device_copy(const void* src, void* dst, int64_t bytes, void* stream);

/* Measurement aid: ONE wave writes n_samples pairs (s_memtime = shader-clock ticks, s_memrealtime = 100 MHz ticks) into
 * out_pairs (2 * n_samples uint64), sleeping sleeps_per_sample x s_sleep 127 between stamps, then ends.  Launched on a
 * stream of its own beside the work under test, delta(s_memtime) / delta(s_memrealtime) x 100 MHz is the shader clock
 * the chip sustains under that work (bench.py: `sustained_clock_mhz`).  Not part of the reference's surface. */
int qpwc_clock_probe(void* out_pairs, int n_samples, int sleeps_per_sample, void* stream);

/* CostVolume / CostVolumeV2 forward.
 * Replaces: CostVolume.call           qpwcnet/core/layers.py:72-100
 *           CostVolumeV2.call         qpwcnet/core/layers.py:128-132, i.e. the op
 *           tfa CorrelationCost(kernel_size=1, max_displacement=r, stride_1=1,
 *           stride_2=1, pad=r, data_format) + leaky_relu   (layers.py:124-125,131)
 *           and their functor twins   qpwcnet/core/non_layers.py:72-104, 119-123.
 *   d = 2*search_range+1
 *   out[b,y,x,i*d+j] = lrelu( (1/C) * sum_c prv[b,y,x,c] * nxt[b,y+i-r,x+j-r,c] ),
 *   nxt taken as zero outside the image; lrelu(v) = v > 0 ? v : slope*v.
 * prv, nxt: (B,H,W,C) or (B,C,H,W) dense; out: (B,H,W,d*d) or (B,d*d,H,W) dense. */
int qpwc_cost_volume_fwd(const void* prv, const void* nxt, void* out,
                         int B, int H, int W, int C, int search_range,
                         int layout, int dtype, float lrelu_slope, void* stream);

/* Same computation, writing into a wider channels-last buffer: pixel p's d*d
 * results go to out + p*out_pixel_stride + out_channel_offset (in elements).
 * This is how Flow/UpFlow's concat([cost, prv, ...]) (non_layers.py:332-338,
 * 381-385) is fed without a copy.  NHWC only.
 * With out_pixel_stride == 84 and out_channel_offset == 0 the three pad channels 81..83 of every
 * pixel are written as zeros: an 84-channel cost volume whose pixels start on 16-byte boundaries (the
 * vector-load layout the fused SeparableConv2D consumes). */
int qpwc_cost_volume_fwd_strided(const void* prv, const void* nxt, void* out,
                                 int B, int H, int W, int C, int search_range,
                                 int dtype, float lrelu_slope,
                                 int64_t out_pixel_stride, int64_t out_channel_offset,
                                 void* stream);

/* Warp / WarpV2 forward.
 * Replaces: WarpV2.call  qpwcnet/core/layers.py:177-186 (non_layers.py:147-158):
 *             tfa.image.dense_image_warp(img, -flo[..., ::-1])  -> mode CLAMP
 *           Warp.call    qpwcnet/core/layers.py:166-168 -> tf_warp,
 *             qpwcnet/core/warp.py:63-153                       -> mode TFWARP
 * Samples img at (y + flo[...,1], x + flo[...,0]) bilinearly.
 * img/out: (B,H,W,C) or (B,C,H,W) of `dtype`; flo: same layout with 2 channels
 * (x, y), ALWAYS fp32 (coordinates need the precision); flow dims flagged in flo_bcast_mask have extent 1 (e.g. a (1,1,1,2) flow,
 * qpwcnet/app/optical_flow/test_warp.py:32) and flo is dense over the rest.
 * NON-FINITE AND HUGE FLOWS (a diverged model; the 1e10 "unknown" of a .flo file) are values like any other: no address
 * is formed from a flow value before it is clamped into the image.  What the kernels do, and what the CPU restatements
 * under oracle/ follow (tests/test_nonfinite_flow_cpu.py restates it pixel by pixel):
 *   mode TFWARP  the corner is int(x + fx), converted toward zero, SATURATING at INT32_MIN / INT32_MAX, NaN -> 0; the
 *                second corner is corner + 1, except that the second corner of INT32_MAX is INT32_MAX (no wrap); both
 *                are then clamped to [0, size - 1]; the weights use the clamped corners and the raw sum, so a NaN or
 *                infinite coordinate gives a NaN output at that pixel, a finite huge one a finite output;
 *   mode CLAMP   floor and alpha are clamped in floating point with fmaxf / fminf, which return their other operand
 *                for a NaN: a NaN coordinate samples corner 0 with alpha 0, +Inf the last corner pair with alpha 1,
 *                -Inf corner 0 with alpha 0; the output is finite whenever img is.
 * Only the pixel that carries such a flow is affected. */
int qpwc_warp_fwd(const void* img, const void* flo, void* out,
                  int B, int H, int W, int C, int flo_bcast_mask,
                  int layout, int dtype, int mode, void* stream);

/* ---- Backward passes (training through the layers; the reference trains with them through TF autograd,
 * qpwcnet/app/optical_flow/train.py, qpwcnet/train/loss.py).  NHWC, dense; fp32 or fp16 storage, fp32 accumulation. */

/* CostVolume / CostVolumeV2 backward: the gradient of qpwc_cost_volume_fwd (layers.py:72-100, 128-132) with
 * g' = grad_out * (out > 0 ? 1 : slope), out the saved forward output (for slope > 0 the sign of the pre-activation;
 * slope at exactly 0, as tf.nn.leaky_relu's gradient, layers.py:99, 131):
 *   grad_prv[b,y,x,c]   = (1/C) sum_ij g'[b,y,x,ij] nxt[b,y+i-r,x+j-r,c]
 *   grad_nxt[b,y',x',c] = (1/C) sum_ij g'[b,y'-i+r,x'-j+r,ij] prv[b,y'-i+r,x'-j+r,c]  (source pixels inside the image)
 * prv, nxt, grad_prv, grad_nxt: (B,H,W,C); out, grad_out: (B,H,W,d*d); all of `dtype`.  Either gradient may be NULL
 * (not both).  lrelu_slope must be >= 0 (QPWC_E_RANGE otherwise: with a negative slope out > 0 is not the sign
 * of the pre-activation).  Gathers only: the result is bitwise reproducible. */
int qpwc_cost_volume_bwd(const void* prv, const void* nxt, const void* out, const void* grad_out,
                         void* grad_prv, void* grad_nxt, int B, int H, int W, int C, int search_range,
                         int dtype, float lrelu_slope, void* stream);

/* Floats of device scratch qpwc_warp_bwd needs for grad_img: 0 for fp32, B*H*W*C for fp16 (the fp32 accumulation
 * target, cast once); negative QPWC_E_* for bad arguments. */
int64_t qpwc_warp_bwd_workspace_floats(int B, int H, int W, int C, int dtype);

/* Warp / WarpV2 backward: the gradient of qpwc_warp_fwd (NHWC, flo dense (B,H,W,2) fp32).
 *   mode CLAMP  (WarpV2, layers.py:177-186; tfa interpolate_bilinear, warp.py:157-185,207): floor = clamp(floor(q),
 *               0, size-2) carries no gradient, alpha = clamp(q - floor, 0, 1) passes it on [0, 1] -- a coordinate
 *               outside [0, size-1] gets zero flow gradient, an exact integer the one-sided (forward) difference.
 *               H, W >= 2 as in the forward (QPWC_E_SHAPE otherwise).
 *   mode TFWARP (Warp / tf_warp, warp.py:100-151): truncated, clipped corner indices carry no gradient; the raw
 *               weights wa..wd (warp.py:139-142) carry it through the float x, y; coinciding clipped corners each
 *               receive their weight.
 * grad_flo: fp32 (B,H,W,2), a per-pixel reduction over C (deterministic).  grad_img: (B,H,W,C) of `dtype`, zeroed by
 * this call on `stream`, then the weighted corner contributions are scattered with float atomics (fp16: into
 * `workspace`, qpwc_warp_bwd_workspace_floats() floats, cast once).  Either gradient may be NULL (not both). */
int qpwc_warp_bwd(const void* img, const void* flo, const void* grad_out,
                  void* grad_img, void* grad_flo, void* workspace, int B, int H, int W, int C,
                  int dtype, int mode, void* stream);

/* ---- Training losses (qpwcnet/train/loss.py; train.py:98-122 sums one per prediction level).  One full-resolution
 * ground truth y_true (B,H,W,C) / (B,C,H,W) fp32 against n_levels (1..8) predictions y_pred[l] (B,h[l],w[l],C) /
 * (B,C,h[l],w[l]) of the same layout, storage pred_dtype[l] (QPWC_F32 / QPWC_F16), all dense; fp32 arithmetic.
 * The ground truth of level l is y_true resampled to (h[l], w[l]) and, for the flow losses, multiplied by h[l] / H on
 * BOTH channels (the reference's flow scale, kept as it is even when H / h != W / w). */
#define QPWC_LOSS_FLOW_MSE_V2 0    /* FlowMseLossV2 (loss.py:134-174): area mean over sh x sw blocks (sh = H/h,
                                    * sw = W/w: H % h == W % w == 0), Keras Huber(delta = p0, the reference's 0.1) of
                                    * s*gt - s*pred with s = 2/(w+h), quadratic at |e| <= delta; mean over elements */
#define QPWC_LOSS_FLOW_MSE 1       /* FlowMseLoss (loss.py:25-82): bilinear (tf.image.resize, half-pixel centres, no
                                    * antialias), ||gt - pred||_2 over the 2 channels, mean over pixels.  Gradient at
                                    * a zero residual: 0 (TF gives NaN there; train.py:120 replaces NaN gradients by 0) */
#define QPWC_LOSS_FLOW_FINETUNE 2  /* FlowMseLossFineTune (loss.py:85-131): bilinear, (||gt - pred||_1 + eps)^q with
                                    * q = p0, eps = p1, mean over pixels; the L1 norm's gradient uses sign(0) = 0 */
#define QPWC_LOSS_AUTORESIZE_MSE 3 /* AutoResizeMseLoss (loss.py:177-197): bilinear, no flow scale, any C, squared
                                    * error, mean over elements */

/* Floats of device scratch qpwc_loss_fwd needs (the per-level partial sums); negative QPWC_E_* for bad arguments. */
int64_t qpwc_loss_workspace_floats(int kind, int B, int H, int W, int C, const int* h, const int* w, int n_levels);

/* out_losses[l] = loss of level l (n_levels fp32), in two launches for all levels: one partial-sum kernel (the area
 * loss reads y_true once for every level when the factors are nested powers of two: 32x32 tiles, H % 32 == W % 32 ==
 * 0, sh*sw >= 4, y_true 16-byte aligned; otherwise one thread per predicted pixel) and one fixed-order fold.
 * Bitwise reproducible: no atomics, fixed grids.
 * dpred: NULL, or n_levels fp32 buffers shaped like y_pred[l]: written with d out_losses[l] / d y_pred[l].
 * gt_out: NULL, or n_levels fp32 buffers (NULL entries skipped) shaped like y_pred[l] with y_true's C: written with
 * level l's resampled, flow-scaled ground truth.  y_pred[l] may be NULL where gt_out[l] is not (the prediction is
 * then taken as zero).  Outputs and workspace (qpwc_loss_workspace_floats()) must not overlap the inputs or each
 * other.  Errors: QPWC_E_MODE kind, QPWC_E_LAYOUT layout, QPWC_E_DTYPE pred_dtype, QPWC_E_SHAPE n_levels outside
 * 1..8 / extents / C != 2 for a flow loss / an area factor that does not divide / more than 2^31 - 1 pixels in an
 * image of y_true or of a level, or 32x32 tiles in y_true (both are counted in 32 bits), QPWC_E_RANGE delta < 0,
 * QPWC_E_NULL, QPWC_E_ALIGN, QPWC_E_ALIAS. */
int qpwc_loss_fwd(int kind, float p0, float p1, const void* y_true, int B, int H, int W, int C, int layout,
                  const void* const* y_pred, const int* h, const int* w, const int* pred_dtype, int n_levels,
                  void* out_losses, void* const* dpred, void* const* gt_out, void* workspace, void* stream);

/* The kernel qpwc_loss_fwd launches for these arguments ("loss_area_tile_kernel" / "loss_pixel_kernel"), "" for
 * arguments it refuses (host only). */
const char* qpwc_loss_fwd_kernel(int kind, const void* y_true, int B, int H, int W, int C, const int* h, const int* w,
                                 int n_levels);

/* Backward of qpwc_loss_fwd in one launch: grad_pred[l][i] = grad_losses[l] * dpred[l][i] (n_elems[l] elements;
 * grad_losses: n_levels fp32 on the device), stored in pred_dtype[l]. */
int qpwc_loss_bwd(const void* const* dpred, const void* grad_losses, void* const* grad_pred, const int64_t* n_elems,
                  const int* pred_dtype, int n_levels, void* stream);

/* ---- Training input pipeline (qpwcnet/data/augment.py:83-173 image_flip_ud / image_flip_lr / image_scale_and_crop /
 * image_resize / image_augment_colors; app/optical_flow/train.py:54-94 preprocess / preprocess_no_op), batched.
 * ims (B,H,W,6): two RGB frames per sample, channels-last, uint8 (QPWC_U8, taken times float32(1/255)) or fp32
 * (QPWC_F32, taken as it is); flo (B,H,W,2) fp32 (u, v).  Per sample b, in this order:
 *   flips       rows reversed and v negated (flip_ud), columns reversed and u negated (flip_lr);
 *   scale+crop  all 8 channels resized to (rh, rw) with tf.image.resize(BILINEAR) (half-pixel centres, no antialias:
 *               per axis src = (i + 0.5) * (in / float(out)) - 0.5, lo = max(floor(src), 0), hi = min(ceil(src), in - 1),
 *               t = src - floor(src), value = a + (b - a) * t, rows after columns; a NaN neighbour poisons the pixel
 *               even at weight 0), of which only the window [oy, oy + h) x [ox, ox + w) is computed;
 *   flow        (u, v) * (mu, mv);
 *   colours     (flag QPWC_AUGMENT_COLOR) on both frames with the same four scalars: x + brightness; HSV saturation *
 *               saturation, clipped to [0, 1]; HSV hue + hue mod 1 (tf.image.rgb_to_hsv / hsv_to_rgb; no clipping of
 *               RGB anywhere); (x - mean_c) * contrast + mean_c with mean_c the mean of colour channel c over the h * w
 *               pixels of BOTH frames (the reference's 'h (w k) c' rearrangement: three means per sample);
 *   offset      ims - 0.5;   scrub: NaN -> 0 in ims and flo, last (train.py:91-92).  Neither with QPWC_AUGMENT_RAW.
 * Parameters, in device memory, read by the kernels (no host synchronisation):
 *   iparams (B,6) int32 : rh, rw, oy, ox, flip_ud, flip_lr       (0 <= oy <= rh - h, 0 <= ox <= rw - w; flips 0 / 1)
 *   fparams (B,6) fp32  : mu, mv, brightness, saturation, hue, contrast
 * image_augment: rh, rw = int32(float32(H, W) * float32(scale)), mu = +-scale, mv = +-scale with the flip signs folded
 * in.  image_resize / preprocess_no_op: rh = h, rw = w, offsets 0, mu = w / W, mv = h / H, flags 0.  Source indices
 * are clamped into the image whatever the parameters hold; parameters outside the ranges above give unspecified
 * values, never an access outside the buffers.
 * out_ims (B,h,w,6) / (B,6,h,w) and out_flo (B,h,w,2) / (B,2,h,w) fp32 by `layout`, written in that layout by the
 * kernels themselves.  workspace: qpwc_augment_workspace_floats() floats (the contrast partial sums; may be NULL
 * with flags 0).  One launch with flags 0; with QPWC_AUGMENT_COLOR a second one folds the partial sums in a fixed
 * order and applies contrast, offset and scrub in place.  No atomics: bitwise reproducible.
 * Alignment: ims 2 bytes (uint8) / 8 (fp32), flo 8, everything else 4.  Errors: QPWC_E_MODE (unknown flag bits),
 * QPWC_E_NULL, QPWC_E_DTYPE (ims_dtype), QPWC_E_LAYOUT, QPWC_E_SHAPE (an extent < 1; H * W or 6 * h * w or the number
 * of 256-pixel workgroups B * ceil(h * w / 256) above 2^31 - 1 -- source offsets themselves are 64-bit), QPWC_E_ALIGN,
 * QPWC_E_ALIAS (an output or the workspace overlapping an input or another output). */
#define QPWC_AUGMENT_COLOR 1 /* flags: run the colour stage */
#define QPWC_AUGMENT_RAW 2   /* flags: leave out the offset and the scrub (image_augment / image_resize on their own) */
int64_t qpwc_augment_workspace_floats(int B, int h, int w);
int qpwc_augment_fwd(const void* ims, int ims_dtype, const void* flo, int B, int H, int W, const void* iparams,
                     const void* fparams, int h, int w, int flags, int layout, void* out_ims, void* out_flo,
                     void* workspace, void* stream);

/* The form of the first launch of qpwc_augment_fwd for these arguments (host only): "augment_pixel_kernel<vec4>" (h * w
 * a multiple of 4 and both outputs 16-byte aligned: the workgroup's pixels leave through LDS as 16-byte stores) or
 * "augment_pixel_kernel<scalar>" (4-byte stores); "" for arguments it refuses.  The second launch takes the same form. */
const char* qpwc_augment_fwd_kernel(int B, int h, int w, const void* out_ims, const void* out_flo);

/* UpFlow front end in one launch (non_layers.py:377-385):
 *   nxt_w = WarpV2(nxt, flo); cost = CostVolumeV2(prv, nxt_w)
 * without materialising nxt_w.  NHWC, mode CLAMP, flo dense (B,H,W,2) fp32,
 * search_range 4, C % 4 == 0.  Output addressing as in
 * qpwc_cost_volume_fwd_strided (pass stride d*d, offset 0 for a dense result).
 * ALIGNMENT: prv and nxt must be 16-byte aligned (every fused kernel gathers them as 16-byte vectors and there is no
 * element-wise form): QPWC_E_ALIGN otherwise, qpwc_last_error() names the operand.  flo (4 bytes) and out (its
 * element) are element-aligned like everywhere else.
 * PERFORMANCE NOTE: this entry point always computes what it is asked.  Where the matrix-core
 * kernels do not apply (qpwc_cost_volume_kernel(..., fused=1) names the choice: anything but
 * "cost_volume_mfma_lds*" means fewer than 256 regions of 8x8 pixels, C % 32 != 0, or a generic
 * shape) it runs the LDS-tiled vector kernel, which is SLOWER than calling qpwc_warp_fwd +
 * qpwc_cost_volume_fwd (B=8, 16x32x256: 94 us against 5.6 + 7.8 us).  A caller that wants the
 * faster of the two asks qpwc_cost_volume_kernel(..., fused=1) first, as qpwcnet_amd/non_layers.py does. */
int qpwc_warp_cost_volume_fwd(const void* prv, const void* nxt, const void* flo, void* out,
                              int B, int H, int W, int C, int search_range,
                              int dtype, float lrelu_slope,
                              int64_t out_pixel_stride, int64_t out_channel_offset,
                              void* stream);

/* Which kernel qpwc_cost_volume_fwd[_strided] (fused == 0) or qpwc_warp_cost_volume_fwd (fused != 0) launches for
 * this shape with 16-byte aligned operands: the launchers' own selection rules run without enqueuing anything
 * (host only, no GPU call).  out_pixel_stride <= 0 means dense.  Returns a static string -- one of
 * "cost_volume_mfma_kernel", "cost_volume_mfma_lds_kernel", "cost_volume_mfma_lds_kernel<true>",
 * "cost_volume_mfma_lds8x16_warp_kernel", "cost_volume_mfma_lds16_kernel<true>",
 * "cost_volume_mfma_lds_f16_kernel", "cost_volume_mfma_lds_f16_kernel<true>", "cost_volume_tiled_kernel",
 * "cost_volume_tiled_kernel<fused>", "cost_volume_generic_kernel" -- or "" for arguments the entry point refuses.
 * No reference counterpart: a caller's aid for the fused-or-pair decision (see the note above) and for profiles. */
const char* qpwc_cost_volume_kernel(int B, int H, int W, int C, int search_range, int layout, int dtype,
                                    int64_t out_pixel_stride, int fused);

/* End-point error (qpwcnet/app/optical_flow/train.py:247-253):
 *   *out_mean = mean over (b,y,x) of || y_true - y_pred ||_2 over the 2 flow channels.
 * fp32 flows of shape (B,H,W,2) / (B,2,H,W).  workspace: >= qpwc_epe_workspace_floats()
 * floats of device scratch owned by the caller (deterministic two-stage sum). */
int qpwc_epe_workspace_floats(void);
int qpwc_epe_fwd(const void* y_true, const void* y_pred, void* out_mean, void* workspace,
                 int B, int H, int W, int layout, void* stream);

/* Multi-scale form (FlowMseLoss.call, qpwcnet/train/loss.py:56-67): the EPE of n_levels
 * (<= 8) fp32 flow pairs y_true[i], y_pred[i] with n_pixels[i] = B*h_i*w_i each, in two
 * launches.  plane_pixels: NULL or all zero = channels-last (B,h,w,2) flows; plane_pixels[i] =
 * h_i*w_i > 0 = 'channels_first' (B,2,h,w) flows at that level.  out_means: n_levels floats;
 * workspace: >= qpwc_epe_multi_workspace_floats() floats. */
int qpwc_epe_multi_workspace_floats(void);
int qpwc_epe_multi_fwd(const void* const* y_true, const void* const* y_pred, const int64_t* n_pixels,
                       const int64_t* plane_pixels, int n_levels, void* out_means, void* workspace,
                       void* stream);
/* The same with a storage dtype per prediction (pred_dtype[i] = QPWC_F32 / QPWC_F16; y_true stays fp32): the
 * fp16-storage network's flows are converted inside the reduction instead of by a pass of their own. */
int qpwc_epe_multi_mixed_fwd(const void* const* y_true, const void* const* y_pred, const int64_t* n_pixels,
                             const int64_t* plane_pixels, const int* pred_dtype, int n_levels, void* out_means,
                             void* workspace, void* stream);

/* cost_volume_to_flow (qpwcnet/core/vis.py:9-34): flow[b,y,x] = (di, dj), the (row, column) displacement
 * of the first maximum over the D = d*d channels of a cost volume: imax = argmax_k, q = sqrt(D),
 * di = floor(imax/q) - (q-1)/2, dj = imax - floor(imax/q)*q - (q-1)/2 in fp32 like the reference.
 * cvol: (B,H,W,D) read at pixel_stride elements per pixel (>= D: the 84-channel padded volume decodes
 * in place) or (B,D,H,W) (pixel_stride == D); fp32 or fp16.  flow: fp32 (B,H,W,2) / (B,2,H,W).
 * NaN-free input assumed (tf.argmax's NaN ordering is not reproduced). */
int qpwc_cost_volume_to_flow_fwd(const void* cvol, void* flow, int B, int H, int W, int D,
                                 int64_t pixel_stride, int layout, int dtype, void* stream);

/* ---- OptFlow block, the step right after the cost volume at every level
 * (reference qpwcnet/core/non_layers.py:213-273) ---------- */

/* Depthwise half of SeparableConv2D(3x3, 'same', depth_multiplier 1, no depthwise
 * bias) (non_layers.py:223-231): out[b,y,x,c] = sum_{ky,kx} w[c,ky,kx] * in0[b,y+ky-1,x+kx-1,c],
 * in0 = (mish_on_load ? Mish(in) : in) inside the image and 0 outside.
 * `in` is the channel-wise concatenation of n_src (1..3) channels-last fp32 sources:
 * source i contributes src_channels[i] channels read at src[i] + pixel*src_pixel_stride[i]
 * (elements; all sources and `out` share the storage `dtype`, weights/params stay fp32,
 * arithmetic is fp32) -- Flow/UpFlow's concat([cost, prv, flo]) (non_layers.py:336-338,381-385) is
 * never materialised.  weight: (C,3,3) fp32, C = sum(src_channels); out: (B,H,W,C) dense. */
int qpwc_dwconv3x3_fwd(const void* const* src, const int* src_channels,
                       const int64_t* src_pixel_stride, int n_src, int mish_on_load,
                       const void* weight, void* out, int B, int H, int W, int dtype, void* stream);

/* The whole SeparableConv2D(3x3,'same') before its activation, fp32, in one launch:
 *   out[b,y,x,f] = bias[f] + sum_c pw[f,c] * (depthwise3x3(in0))[b,y,x,c]
 * with `in`/`in0` as in qpwc_dwconv3x3_fwd (1..3 sources); mish_flags: bit 0 = Mish on load (the
 * input is a pre-activation tensor), bit 1 = store Mish(out) (the SeparableConv2D's own
 * `activation='Mish'`, non_layers.py:226, applied once per element instead of at the next load); the
 * depthwise result stays on chip (LDS -> matrix cores).  dw: (C,3,3); pw: (F, Cpad) row-major,
 * Cpad = ceil(C/32)*32, zero padded; bias: (F); F in {16,32,64,128}; out: (B,H,W,F) dense. */
int qpwc_sepconv3x3_fwd(const void* const* src, const int* src_channels,
                        const int64_t* src_pixel_stride, int n_src, int mish_flags,
                        const void* dw, const void* pw, const void* bias, void* out,
                        int B, int H, int W, int F, void* stream);

/* Floats of device scratch qpwc_sepconv3x3_bwd needs for C = sum(src_channels) input channels (the recomputed
 * depthwise result and its gradient, (B*H*W, Cpad) each, gz (B*H*W, F), and the per-workgroup partials of the three
 * weight gradients); negative QPWC_E_SHAPE for a non-positive extent, F outside {16,32,64,128} or a shape whose
 * launch grids do not fit. */
int64_t qpwc_sepconv3x3_bwd_workspace_floats(int B, int H, int W, int C, int F);

/* Gradient of qpwc_sepconv3x3_fwd (fp32): what TF autograd takes through SeparableConv2D(3x3,'same')
 * (non_layers.py:223-231) under qpwcnet/app/optical_flow/train.py.  With x = concat(src), a = Mish(x) if bit 0 of
 * mish_flags else x, d = depthwise3x3(a), z = bias + pw d, out = Mish(z) if bit 1 else z, and g = grad_out =
 * dL/d(what the forward stored), dense (B,H,W,F):
 *   gz = g * Mish'(z) if bit 1 else g,   Mish'(t) = tanh(sp) + t (1 - tanh(sp)^2) sigmoid(t), sp = softplus(t)
 *   grad_bias[f] = sum_p gz[p,f]
 *   grad_pw[f,c] = sum_p gz[p,f] d[p,c]                        (F, Cpad); columns c >= C are written as 0
 *   gd[p,c]      = sum_f gz[p,f] pw[f,c]
 *   grad_dw[c,ky,kx] = sum_p gd[p,c] a[p+(ky-1,kx-1),c]         (C,3,3); pixels inside the image only
 *   ga[p,c]      = sum_{ky,kx} dw[c,ky,kx] gd[p-(ky-1,kx-1),c]  (source pixels inside the image)
 *   grad_src     = ga * Mish'(x) if bit 0 else ga, one dense (B,H,W,src_channels[i]) tensor per source
 * d and z are recomputed from the sources (Mish is not invertible; nothing but the sources and weights is needed).
 * src / src_channels / src_pixel_stride / dw / pw / bias / F as in the forward.  grad_src: n_src pointers, each may
 * be NULL, as may the array; grad_dw, grad_pw, grad_bias may be NULL; not all outputs.  Work whose only consumer is
 * a NULL output is skipped (no depthwise backward when only grad_pw / grad_bias are asked for).  All five outputs
 * are bitwise reproducible: fixed-order two-stage reductions, no atomics.  workspace:
 * qpwc_sepconv3x3_bwd_workspace_floats() floats.  Alignment: pw, grad_out, grad_pw and workspace 16 bytes (read and
 * written as float4 / 16-byte rows), everything else 4.  Errors: QPWC_E_NULL, QPWC_E_SHAPE (extents, F, n_src,
 * mish_flags, channels <= 0, pixel stride < channels), QPWC_E_ALIGN, QPWC_E_ALIAS (an output or the workspace
 * overlapping an input or another output); qpwc_last_error() names the argument. */
int qpwc_sepconv3x3_bwd(const void* const* src, const int* src_channels, const int64_t* src_pixel_stride,
                        int n_src, int mish_flags, const void* dw, const void* pw, const void* bias,
                        const void* grad_out, void* const* grad_src, void* grad_dw, void* grad_pw, void* grad_bias,
                        void* workspace, int B, int H, int W, int F, void* stream);

/* qpwc_sepconv3x3_fwd with the pointwise products on the bf16 matrix instructions ("bf16x3", csrc/split_bf16.h: both
 * operands split into three bf16 values, six partial products, fp32 accumulation; depthwise 3x3 in fp32 as before).
 * pw3: the (F, Cpad) fp32 matrix of qpwc_sepconv3x3_fwd split by qpwc_split_bf16x3_fwd = (3, F, Cpad) bf16.
 * Sources: every source but the last a multiple of 4 channels in 16-byte aligned pixels (a last source of fewer than 4
 * channels is allowed), H*W < 2^24 -- QPWC_E_ALIGN otherwise (use qpwc_sepconv3x3_fwd then). */
int qpwc_sepconv3x3_x3_fwd(const void* const* src, const int* src_channels, const int64_t* src_pixel_stride,
                           int n_src, int mish_flags, const void* dw, const void* pw3, const void* bias, void* out,
                           int B, int H, int W, int F, void* stream);

/* The same SeparableConv2D for fp16 storage (BASELINE configs[4]; the reference itself has no
 * fp16 path; layer: non_layers.py:223-231): sources and `out` fp16, dw (C,3,3) and bias (F) fp32, pw (F, Cpad)
 * fp16 with Cpad = ceil(C/32)*32, zero padded.  Depthwise in fp32 on the fp16 input, rounded to fp16
 * once, pointwise on the f16 matrix cores with fp32 accumulation; mish_flags as above.  Sources as in
 * qpwc_sepconv3x3_fwd, each a multiple of 4 channels in 8-byte aligned pixels (a last source of fewer
 * than 4 channels is read element-wise); one dense source of C % 8 == 0 channels in 16-byte aligned
 * pixels takes 16-byte loads. */
int qpwc_sepconv3x3_f16_fwd(const void* const* src, const int* src_channels,
                            const int64_t* src_pixel_stride, int n_src, int mish_flags,
                            const void* dw, const void* pw, const void* bias, void* out,
                            int B, int H, int W, int F, void* stream);

/* Tail of OptFlow.__call__ (non_layers.py:238-254, 268-273) on the 16-channel
 * pre-activation output z (B,H,W,16) of the last SeparableConv's pointwise conv:
 *   flow = scale * conv3x3_{16->2, no bias, 'same'}( BN( Mish( W1 * Mish(z) + b1 ) ) )
 * params (device fp32, qpwc_flow_head_param_floats() = 592 floats):
 *   w1[16][16] (out,in) | b1[16] | bn_scale[16] | bn_shift[16] | wf[3][3][16][2] (ky,kx,in,out)
 * with bn_scale = gamma/sqrt(var+eps), bn_shift = beta - mean*bn_scale.
 * out: (B,H,W,2) for out_layout QPWC_NHWC, (B,2,H,W) for QPWC_NCHW (a 'channels_first' model's flow
 * output, written by the kernel itself instead of by a transposition launch). */
int qpwc_flow_head_param_floats(void);
int qpwc_flow_head_fwd(const void* z, const void* params, void* out, int B, int H, int W,
                       float scale, int dtype, int out_layout, void* stream);

/* Training-mode BatchNormalization(fused=False) of the flow head (non_layers.py:242; the trainer calls
 * model(ims, training=True), app/optical_flow/train.py:270), fp32 channels-last.  With m = Mish(z), a = W1 m + b1,
 * u = Mish(a) over the M = B*H*W pixels:
 *   mean[c] = sum_p u[p,c] / M,   var[c] = sum_p (u[p,c] - mean[c])^2 / M        (biased, as Keras' non-fused layer)
 * in two stages: per-workgroup (count, mean, M2) partials of shifted sums, then a fixed-order Chan merge (accurate
 * for |mean| >> std, bitwise reproducible, no atomics).  The merging launch also writes, on the device,
 *   params (592 floats, what qpwc_flow_head_fwd takes): w1 | b1 | s | t | wf,  s = gamma / sqrt(var + eps),
 *                                                        t = beta - mean s
 *   stats (48 floats, may be NULL): mean | var | mean_lo -- what qpwc_flow_head_bwd takes; mean_lo is what the
 *                                                        rounding of the batch mean to fp32 dropped
 *   moving_mean / moving_var (16 floats each, both or neither NULL), in place:
 *                                                        moving = moving * momentum + batch * (1 - momentum)
 * so that the training forward is this call followed by qpwc_flow_head_fwd, with no host synchronisation.
 * z: (B,H,W,16); w1 (16,16) (out,in); b1, gamma, beta (16); wf (3,3,16,2) (ky,kx,in,out).  workspace:
 * qpwc_flow_head_stats_workspace_floats() floats (negative QPWC_E_SHAPE for a non-positive extent or more than
 * 2^24 pixels).  z, w1, b1, params, stats and workspace 16-byte aligned (read or written as float4), the rest 4.
 * Errors: QPWC_E_NULL, QPWC_E_SHAPE, QPWC_E_RANGE (eps <= 0, momentum outside [0,1]), QPWC_E_ALIGN, QPWC_E_ALIAS. */
int64_t qpwc_flow_head_stats_workspace_floats(int B, int H, int W);
int qpwc_flow_head_stats_fwd(const void* z, const void* w1, const void* b1, const void* gamma, const void* beta,
                             const void* wf, void* moving_mean, void* moving_var, float momentum, float eps,
                             void* params, void* stats, void* workspace, int B, int H, int W, void* stream);

/* Gradient of qpwc_flow_head_fwd (fp32, channels-last output), in both BatchNorm modes.  Notation per pixel p:
 *   m = Mish(z), a = W1 m + b1, u = Mish(a), h = s u + t, flow = scale conv3x3(h, wf) (zero 'same' padding)
 * z, params (w1 | b1 | s | t | wf) and scale as in the forward; stats = mean | var | mean_lo (48 floats) that s and t
 * were made from (those of qpwc_flow_head_stats_fwd, or the frozen moving ones with mean_lo = 0), eps the same;
 * g = grad_out = dL/dflow (B,H,W,2).  u, a and m are recomputed from z (Mish is not invertible; the forward stores
 * nothing).
 *   gh[p,c]          = scale sum_k sum_o wf[k,c,o] g[p-k+1,o]            (g = 0 outside the image)
 *   grad_wf[k,c,o]   = scale sum_p h[p+k-1,c] g[p,o]                     (3,3,16,2), h = 0 outside the image
 *   xh = (u - mean - mean_lo) rstd, rstd = 1 / sqrt(var + eps)
 *   grad_beta[c]     = sum_p gh[p,c]           grad_gamma[c] = sum_p gh[p,c] xh[p,c]
 *   gu = s gh                                                             training == 0 (frozen statistics)
 *   gu = s (gh - grad_beta / M - xh grad_gamma / M)                       training != 0 (batch statistics)
 *   ga = gu Mish'(a)     grad_b1[f] = sum_p ga[p,f]     grad_w1[f,c] = sum_p ga[p,f] m[p,c]
 *     (training != 0: sum_p gu = 0 identically, and grad_b1 is summed as sum_p gu (Mish'(a) - 1), which does not round
 *      M cancelling terms)
 *   grad_z = (W1^T ga) Mish'(z)
 * Any of the six outputs may be NULL (not all); a pass whose only consumers are NULL is not launched.  Both 16 x 16
 * products run on v_mfma_f32_16x16x4_f32.  Every output is bitwise reproducible and the same bits whatever else is
 * asked for: per-workgroup partials in tile order, then a fixed-order sum; no atomics.  With training == 0 a pixel's
 * grad_z depends on its own image only.  workspace: qpwc_flow_head_bwd_workspace_floats() floats.  z, params,
 * stats, grad_z and workspace 16-byte aligned (float4 loads and stores), grad_out 8, the rest 4.  Errors:
 * QPWC_E_NULL, QPWC_E_SHAPE, QPWC_E_RANGE (eps <= 0), QPWC_E_ALIGN, QPWC_E_ALIAS (an output or the workspace
 * overlapping an input or another output). */
int64_t qpwc_flow_head_bwd_workspace_floats(int B, int H, int W);
int qpwc_flow_head_bwd(const void* z, const void* params, const void* stats, float eps, int training, float scale,
                       const void* grad_out, void* grad_z, void* grad_w1, void* grad_b1, void* grad_gamma,
                       void* grad_beta, void* grad_wf, void* workspace, int B, int H, int W, void* stream);

/* Pointwise half of a SeparableConv2D whose depthwise half ran as qpwc_dwconv3x3_fwd (non_layers.py:223-231; the wide
 * first OptFlow layer of the coarsest levels, which stay split): out (M, F) = y (M, C) . weight^T + bias, fp32, on the
 * matrix cores, M = B*H*W pixels.  weight: (F, ceil(C/32)*32) row-major, zero padded (the layout qpwc_sepconv3x3_fwd
 * takes); F in {16,32,64,128,256}.  Measured slower than hipBLASLt at the step's shapes: the network keeps the
 * library GEMM for these two layers; this entry point serves callers that have none. */
int qpwc_pointwise_bias_fwd(const void* y, const void* weight, const void* bias, void* out, int64_t M, int C, int F,
                            void* stream);

/* qpwc_flow_head_fwd (channels-last) AND the Upsample(scale = up_scale) that follows it in pwcnet.py:55,60 in one launch:
 * out (B,H,W,2) as there, out_up (B,2H,2W,2) = up_scale * UpSampling2D(2, 'bilinear')(out) -- bit for bit what
 * qpwc_upsample2x_flow_fwd returns for `out` (the tile's one-pixel rim is computed by the same workgroup).
 * out_up_f32 (fp16 storage only, else NULL): the values of out_up once more as fp32 (B,2H,2W,2) -- the coordinates the next
 * level's WarpV2 takes, which would otherwise be a cast launch of their own. */
int qpwc_flow_head_up_fwd(const void* z, const void* params, void* out, void* out_up, void* out_up_f32, int B, int H, int W,
                          float scale, float up_scale, int dtype, void* stream);

/* The tail of OptFlow.__call__ in one launch, for small images (coarse pyramid levels), fp32 channels-last:
 *   z3   = Mish(SeparableConv2D_3(z2))    64 -> 32   (non_layers.py:223-231, third of the four)
 *   z4   = SeparableConv2D_4(z3)          32 -> 16
 *   flow = scale * conv3x3( BN( Mish( W1 * Mish(z4) + b1 ) ) )   (non_layers.py:238-254, 268-273)
 * z2: (B,H,W,64), the second SeparableConv2D's output, ALREADY Mish-activated (mish_on_load = 0) or
 * pre-activation (mish_on_load = 1).  dw3 (64,9), pw3 (32,64) row-major, b3 (32); dw4 (32,9), pw4 (16,32), b4 (16);
 * head_params as qpwc_flow_head_fwd.  out: (B,H,W,2) / (B,2,H,W) by out_layout.  Same arithmetic as
 * qpwc_sepconv3x3_fwd x 2 + qpwc_flow_head_fwd (fp32 matrix cores for the pointwise parts). */
int qpwc_optflow_tail_fwd(const void* z2, const void* dw3, const void* pw3, const void* b3, const void* dw4,
                          const void* pw4, const void* b4, const void* head_params, void* out, int B, int H, int W,
                          float scale, int mish_on_load, int out_layout, void* stream);

/* x = Mish(x + bias[c]) in place, channels-last fp32 (n_pixels, C), C % 4 == 0, bias may
 * be NULL: the `activation='Mish'` epilogue of the reference's Conv2D / Conv2DTranspose /
 * SeparableConv2D blocks (non_layers.py:196-210, 223-231, 390-449; mish.py:27-28). */
int qpwc_bias_mish_fwd(void* x, const void* bias, int64_t n_pixels, int C, int dtype, void* stream);

/* Out-of-place form that also lays down TensorFlow's 'SAME' padding for a following
 * stride-2 3x3 convolution (0 before, pad_h / pad_w after; non_layers.py:402-409):
 * dst (B, H+pad_h, W+pad_w, *): interior = Mish(src + bias[c]), border = 0.  src (B,H,W,C).
 * dst pixels are dst_pixel_stride elements apart (>= C, multiple of 4) and `dst` already points at
 * the first of the C destination channels: with pad 0 and a wider buffer this writes one
 * half of the decoder's concat([up, skip]) (pwcnet.py:186-195) in place. */
int qpwc_bias_mish_pad_fwd(const void* src, const void* bias, void* dst, int B, int H, int W, int C,
                           int pad_h, int pad_w, int64_t dst_pixel_stride, int dtype, void* stream);

/* Split(2) of the (B,H,W,6) input pair (pwcnet.py:229), the two frames stacked on the batch
 * axis (frame f of pair b at f*B + b; the encoder weights are shared, pwcnet.py:145-162) and
 * zero-padded by pad_h/pad_w at the far edges ('SAME' padding of the first stride-2 conv):
 * out (2B, H+pad_h, W+pad_w, 3). */
int qpwc_split_frames_pad_fwd(const void* in, void* out, int B, int H, int W, int pad_h, int pad_w,
                              int dtype, void* stream);

/* Upsample(scale) of a flow field (non_layers.py:183-193; pwcnet.py:55,60):
 * out (B,2h,2w,2) = scale * bilinear x2 upsampling (half-pixel centres, edge clamp) of
 * in (B,h,w,2); in_layout / out_layout QPWC_NCHW read (B,2,h,w) / write (B,2,2h,2w) instead. */
int qpwc_upsample2x_flow_fwd(const void* in, void* out, int B, int h, int w, float scale, int dtype,
                             int in_layout, int out_layout, void* stream);

/* Adjoint of qpwc_upsample2x_flow_fwd (fp32, channels-last): grad_out (B,2h,2w,2) -> grad_in (B,h,w,2), a gather.
 * Per axis in[i] receives 0.75 (g[2i] + g[2i+1]) + 0.25 (g[2i-1] + g[2i+2]); at the borders the clamped tap's 0.25
 * folds back onto the edge pixel (in[0] += 0.25 g[0], in[h-1] += 0.25 g[2h-1]).  The two axes are separable; the
 * result is multiplied by scale.  One launch, no workspace, bitwise reproducible.  Both pointers 8-byte aligned. */
int qpwc_upsample2x_flow_bwd(const void* grad_out, void* grad_in, int B, int h, int w, float scale, void* stream);

/* inv_flow = -tf_warp(flow, flow) (occlusion.py:85; app/test/test_invert_flow.py:47): the flow
 * field sampled at its own targets with the tf_warp rules (warp.py:63-153), negated.
 * flow, out: (B,H,W,2) [NHWC] or (B,2,H,W) [NCHW], storage `dtype`, arithmetic fp32.
 * Non-finite and huge flows follow mode TFWARP of qpwc_warp_fwd (saturating conversion, NaN -> 0, no wrap of the second
 * corner, clamp after the conversion): the pixel itself and the pixels whose corners it is come out NaN or finite as
 * that rule says; no other pixel changes. */
int qpwc_invert_flow_fwd(const void* flow, void* out, int B, int H, int W, int layout, int dtype,
                         void* stream);

/* estimate_occlusion_map (occlusion.py:27-118): out (B,H,W) fp32, 1 where the pixel leaves the
 * image under `flow` or is the target of no pixel under the inverse flow above
 * (idx3 = clip(int32(p + inv_flow[p])), tensor_scatter_nd_min of zeros into ones), else 0.
 * Two launches (fill, scatter); deterministic.
 * The target int32(p + inv_flow[p]) is converted like the corners of qpwc_warp_fwd's mode TFWARP (toward zero,
 * saturating, NaN -> 0) and then clamped into the image: a pixel whose inverse flow is NaN marks row / column 0, +-Inf or
 * a huge value the nearest border.  The out-of-bounds test of a NaN sum is false.  The map holds 0 and 1 only. */
int qpwc_occlusion_fwd(const void* flow, void* out, int B, int H, int W, int layout, int dtype,
                       void* stream);

/* One 3x3 stride-1 Conv2D(padding='same', activation='Mish') of the encoder's DownConv blocks
 * (conv_aa / conv_b, non_layers.py:410-449 with use_normalizer=False, pwcnet.py:146) for C_in = C_out = C
 * in {16, 32, 64, 128, 256}, channels-last fp32: out (B, H+pad_h, W+pad_w, C), interior = Mish(conv3x3(x) + bias),
 * border (the 'SAME' padding of a following stride-2 convolution, non_layers.py:402-409) = 0.
 * weight: (9, C, C) fp32 = [ky*3+kx][out][in]; x: (B,H,W,C); all pointers 16-byte aligned. */
int qpwc_conv3x3_mish_fwd(const void* x, const void* weight, const void* bias, void* out, int B, int H,
                          int W, int C, int pad_h, int pad_w, void* stream);

/* The same fp32 layer with its products on the bf16 matrix instructions ("bf16x3", csrc/split_bf16.h): both
 * operands are split (exactly) into three bf16 values, six partial products per product, fp32 accumulation -- what is
 * dropped per product is about one fp32 rounding at worst (2^-23), 2^-28 on average.  x, bias, out as qpwc_conv3x3_mish_fwd; weight3: the (9, C, C) fp32 taps split
 * by qpwc_split_bf16x3_fwd = (3, 9, C, C) bf16. */
int qpwc_conv3x3_mish_x3_fwd(const void* x, const void* weight3, const void* bias, void* out, int B, int H,
                             int W, int C, int pad_h, int pad_w, void* stream);

/* src (n) fp32 -> out (3, n) bf16: out[0] = bf16(src), out[1] = bf16(src - out[0]), out[2] = bf16(src - out[0] -
 * out[1]), round to nearest even; src[i] == out[0][i] + out[1][i] + out[2][i] exactly (parts below the smallest normal
 * fp32 flush to zero).
 * Operands must be finite and below ~3.39e38 in magnitude: bf16(a) overflows to Inf above that and the residual
 * a - bf16(a) becomes NaN (the fp32-instruction entry points have no such restriction).
 * The weight operands of the *_x3_fwd entry points. */
int qpwc_split_bf16x3_fwd(const void* src, void* out, long long n, void* stream);

/* The same layer for fp16 storage (BASELINE configs[4]; the reference itself has no fp16 path): x, weight
 * ((9, C, C) = [ky*3+kx][out][in]) and out fp16, bias fp32; fp32 accumulation on the fp16 matrix instructions,
 * bias + Mish in fp32, one rounding to fp16 at the store.  Same shapes, padding and alignment rules. */
int qpwc_conv3x3_mish_f16_fwd(const void* x, const void* weight, const void* bias, void* out, int B, int H,
                              int W, int C, int pad_h, int pad_w, void* stream);

/* First encoder layer on the raw input pair: Split(2) (pwcnet.py:229) + both frames stacked on the
 * batch axis (shared encoder weights, pwcnet.py:145-162) + enc.0.conv_a = Conv2D(3 -> 16, 3x3, stride 2,
 * padding='same' [TensorFlow: 0 before, 1 after for even H, W], activation='Mish')
 * (non_layers.py:402-409):  pairs (B,H,W,6) fp32 (layout QPWC_NHWC) or (B,6,H,W) (QPWC_NCHW, the
 * reference's inference default, app/optical_flow/test_infer.py:52), H and W even  ->  out
 * (2B, H/2, W/2, 16) channels-last, frame f of pair b at f*B + b.
 * weight: (9, 16, 4) fp32 = [ky*3+kx][out][in, slot 3 = 0]; bias (16). */
int qpwc_first_conv_mish_fwd(const void* pairs, const void* weight, const void* bias, void* out, int B,
                             int H, int W, int layout, void* stream);

/* The same layer for fp16 storage (BASELINE configs[4]): pairs and out fp16, weight and bias fp32 as above (the
 * 27-term products are exact in fp32), one rounding at the store; pairs 4-byte, out 8-byte aligned. */
int qpwc_first_conv_mish_f16_fwd(const void* pairs, const void* weight, const void* bias, void* out, int B,
                                 int H, int W, int layout, void* stream);

/* conv_a of the second encoder level: Conv2D(16 -> 32, 3x3, stride 2, padding='same', activation='Mish')
 * (non_layers.py:402-409) on the zero-bordered output of qpwc_conv3x3_mish_fwd (pad 1, 1):
 * x_padded (B, H+1, W+1, 16) fp32 with H, W even (row H and column W zero = TensorFlow's 'SAME' padding)
 * -> out (B, H/2, W/2, 32).  weight: (9, 32, 16) fp32 = [ky*3+kx][out][in]; bias (32). */
int qpwc_conv3x3s2_mish_fwd(const void* x_padded, const void* weight, const void* bias, void* out, int B,
                            int H, int W, void* stream);

/* The same layer for C_in in {16, 32, 64, 128} -> 2 C_in outputs (conv_a of encoder levels 2..5):
 * x_padded (B, H+1, W+1, C_in), weight (9, 2 C_in, C_in), bias (2 C_in), out (B, H/2, W/2, 2 C_in). */
int qpwc_conv3x3s2_mish_c_fwd(const void* x_padded, const void* weight, const void* bias, void* out, int B,
                              int H, int W, int C_in, void* stream);

/* qpwc_conv3x3s2_mish_c_fwd for C_in in {32, 64, 128} with the products on the bf16 matrix instructions ("bf16x3",
 * csrc/split_bf16.h): weight3 = the (9, 2 C_in, C_in) fp32 taps split by qpwc_split_bf16x3_fwd = (3, 9, 2 C_in, C_in) bf16. */
int qpwc_conv3x3s2_mish_x3_fwd(const void* x_padded, const void* weight3, const void* bias, void* out, int B,
                               int H, int W, int C_in, void* stream);

/* The same layers for fp16 storage (BASELINE configs[4]): x_padded, weight ((9, 2 C_in, C_in)) and out fp16, bias
 * fp32, fp32 accumulation, one rounding at the store. */
int qpwc_conv3x3s2_mish_f16_fwd(const void* x_padded, const void* weight, const void* bias, void* out, int B,
                                int H, int W, int C_in, void* stream);

/* Conv2D(C_out, 3x3, strides=stride, padding='same') (+ Mish) of the encoder (non_layers.py:390-449) for any size, on
 * the unpadded input: the training twin of the three forwards above.  fp32, channels-last, dense.
 * TensorFlow 'SAME': Ho = ceil(H / stride), total = max((Ho - 1) stride + 3 - H, 0), pt = total / 2 rows of zeros above
 * (stride 1: 1; stride 2: 0 for even H, with one row below, 1 for odd H); the same for W with pl.
 *   z[n,oy,ox,o] = bias[o] + sum_{ky,kx,i} weight[ky*3+kx][o][i] x[n, oy stride + ky - pt, ox stride + kx - pl, i]
 *   out = Mish(z) if mish else z                                  (terms outside the image are zero)
 * x (B,H,W,C_in), C_in in {3,16,32,64,128,256}; weight (9, C_out, Cp) fp32 tap-major, Cp = C_in rounded up to 4 (the
 * layouts of qpwc_conv3x3_mish_fwd and, for C_in = 3, qpwc_first_conv_mish_fwd); bias (C_out); out (B,Ho,Wo,C_out),
 * C_out in {16,32,64,128,256}; stride in {1,2}; mish in {0,1}.  Implicit GEMM on the fp32 matrix instructions, one
 * launch.  Alignment: weight, out 16 bytes, x 16 bytes (4 for the 12-byte pixels of C_in = 3), bias 4.
 * Errors as qpwc_conv3x3_same_bwd. */
int qpwc_conv3x3_same_fwd(const void* x, const void* weight, const void* bias, void* out, int B, int H, int W,
                          int C_in, int C_out, int stride, int mish, void* stream);

/* Floats of device scratch qpwc_conv3x3_same_bwd needs: gz (B*Ho*Wo, C_out) and one partial of grad_w and grad_b per
 * K-split of the pixel reduction; the number of splits comes from the shape alone.  Negative QPWC_E_SHAPE for a
 * shape qpwc_conv3x3_same_bwd refuses. */
int64_t qpwc_conv3x3_same_bwd_workspace_floats(int B, int H, int W, int C_in, int C_out, int stride);

/* Gradient of qpwc_conv3x3_same_fwd (and of qpwc_conv3x3_mish_fwd / qpwc_conv3x3s2_mish_c_fwd / the first layer, which
 * compute the same function).  With z and 'SAME' as above, g = grad_out = dL/d(out), dense (B,Ho,Wo,C_out), s = stride:
 *   gz = g * Mish'(z) if mish else g,   Mish'(t) = tanh(sp) + t (1 - tanh(sp)^2) sigmoid(t), sp = softplus(t)
 *   grad_b[o]           = sum_{n,oy,ox} gz[n,oy,ox,o]
 *   grad_w[ky,kx][o][i] = sum_{n,oy,ox} gz[n,oy,ox,o] x[n, oy s + ky - pt, ox s + kx - pl, i]
 *   grad_x[n,iy,ix,i]   = sum_{ky,kx,o} weight[ky,kx][o][i] gz[n, (iy + pt - ky) / s, (ix + pl - kx) / s, o]
 *                         over the taps where both quotients are whole and in range
 * (terms outside the image are zero).  z is recomputed from x (Mish is not invertible; only x, weight and bias are
 * needed).  grad_x (B,H,W,C_in); grad_w (9, C_out, Cp) in the layout of weight, its pad slot (C_in = 3) written as 0;
 * grad_b (C_out).  Any of the three may be NULL, not all; a stage whose only consumers are NULL is not launched.
 * Every output is bitwise reproducible and has the same bits whatever else is asked for (fixed-order sums, no
 * atomics, shape-only grids); grad_x of an image does not depend on the rest of the batch.  workspace:
 * qpwc_conv3x3_same_bwd_workspace_floats() floats.  Alignment: weight, grad_out, grad_w, workspace 16 bytes; x and
 * grad_x 16 bytes (4 for C_in = 3); bias, grad_b 4.  Errors: QPWC_E_NULL, QPWC_E_SHAPE (extents < 1, channel counts,
 * stride, mish), QPWC_E_ALIGN, QPWC_E_ALIAS (an output or the workspace overlapping an input or another output);
 * qpwc_last_error() names the argument. */
int qpwc_conv3x3_same_bwd(const void* x, const void* weight, const void* bias, const void* grad_out, void* grad_x,
                          void* grad_w, void* grad_b, void* workspace, int B, int H, int W, int C_in, int C_out,
                          int stride, int mish, void* stream);

/* UpConv of the decoder (non_layers.py:196-210): Conv2DTranspose(F, 4x4, strides 2, padding='same') + bias +
 * Mish of x (B,H,W,C), C in {64,128,256}, F % 16 == 0, written into channels [0, F) of `out`
 * (B, 2H, 2W, *) whose pixels are out_pixel_stride floats apart -- with out_pixel_stride = F + C_skip this is
 * the `up` half of the decoder's concat([up, skip]) (pwcnet.py:186-195) in place.
 * weight: (16, F, C) fp32 = [ky*4+kx][out][in] (torch ConvTranspose2d weight (C,F,4,4) permuted (2,3,1,0)). */
int qpwc_upconv4x4s2_mish_fwd(const void* x, const void* weight, const void* bias, void* out, int B, int H, int W,
                              int C, int F, int64_t out_pixel_stride, void* stream);

/* qpwc_upconv4x4s2_mish_fwd with the products on the bf16 matrix instructions ("bf16x3", csrc/split_bf16.h):
 * weight3 = the (16, F, C) fp32 taps split by qpwc_split_bf16x3_fwd = (3, 16, F, C) bf16; everything else as there. */
int qpwc_upconv4x4s2_mish_x3_fwd(const void* x, const void* weight3, const void* bias, void* out, int B, int H, int W,
                                 int C, int F, int64_t out_pixel_stride, void* stream);

/* The same layer for fp16 storage (BASELINE configs[4]): x, weight ((16, F, C)) and out fp16, bias fp32, fp32
 * accumulation, one rounding at the store; out_pixel_stride in elements (halves), out 8-byte aligned. */
int qpwc_upconv4x4s2_mish_f16_fwd(const void* x, const void* weight, const void* bias, void* out, int B, int H, int W,
                                  int C, int F, int64_t out_pixel_stride, void* stream);

/* qpwc_upconv4x4s2_mish_fwd AND the skip half of the decoder's concat([up, skip]) (pwcnet.py:186-195) in one launch:
 * channels [0, F) of `out` as there, and channels [F, 2F) = the first F channels of `skip` (B, 2H, 2W, >= F), whose batch /
 * row / pixel strides are given in elements (multiples of 4; the skip may be the interior of a zero-bordered buffer).
 * out_pixel_stride >= 2F; out must not overlap x or skip.  fp32: every pointer 16-byte aligned. */
int qpwc_upconv4x4s2_mish_cat_fwd(const void* x, const void* weight, const void* bias, const void* skip,
                                  int64_t skip_batch_stride, int64_t skip_row_stride, int64_t skip_pixel_stride, void* out,
                                  int B, int H, int W, int C, int F, int64_t out_pixel_stride, void* stream);

/* The same for fp16 storage: x, weight, skip and out fp16 (out, skip 8-byte aligned), bias fp32. */
int qpwc_upconv4x4s2_mish_cat_f16_fwd(const void* x, const void* weight, const void* bias, const void* skip,
                                      int64_t skip_batch_stride, int64_t skip_row_stride, int64_t skip_pixel_stride, void* out,
                                      int B, int H, int W, int C, int F, int64_t out_pixel_stride, void* stream);

/* Floats of device scratch qpwc_upconv4x4s2_bwd needs: gz (B*2H*2W, F) and one partial of grad_w and grad_b per
 * K-split of the pixel reduction; the number of splits comes from the shape alone.  Negative QPWC_E_SHAPE for a
 * shape qpwc_upconv4x4s2_bwd refuses. */
int64_t qpwc_upconv4x4s2_bwd_workspace_floats(int B, int H, int W, int C, int F);

/* Gradient of qpwc_upconv4x4s2_mish_fwd / _cat_fwd: the layer Mish(Conv2DTranspose(F, 4x4, strides 2, 'same')(x) + bias),
 * torch's conv_transpose2d(stride=2, padding=1) + Mish.  fp32, channels-last, dense.  x (B,H,W,C), C in {64,128,256};
 * weight (16, F, C) tap-major, weight[ky*4+kx][f][c], F in {16,32,64,128}; bias (F).  With g = grad_out = dL/d(out)
 * and terms outside the image equal to zero:
 *   z[n,oy,ox,f]        = bias[f] + sum_{ky,kx,c} weight[ky,kx][f][c] x[n,iy,ix,c]
 *                         over oy = 2 iy - 1 + ky, ox = 2 ix - 1 + kx   (an output of parity (py,px) meets 2x2 of the taps)
 *   gz                  = g * Mish'(z) if mish else g
 *   grad_b[f]           = sum_{n,oy,ox} gz[n,oy,ox,f]
 *   grad_w[ky,kx][f][c] = sum_{n,iy,ix} gz[n, 2 iy - 1 + ky, 2 ix - 1 + kx, f] x[n,iy,ix,c]
 *   grad_x[n,iy,ix,c]   = sum_{ky,kx,f} weight[ky,kx][f][c] gz[n, 2 iy - 1 + ky, 2 ix - 1 + kx, f]
 * z is recomputed from x (the forward stores Mish(z) only; x, weight and bias are all that is needed).  grad_out is
 * channels [0, F) of a (B,2H,2W,*) buffer whose pixels are grad_out_pixel_stride floats apart (>= F, a multiple of
 * 4, at most 2^24): with F + C_skip it is the `up` half of the gradient of the decoder's concat([up, skip]), read in place.
 * grad_x (B,H,W,C); grad_w (16, F, C) in the layout of weight; grad_b (F).  Any of the three may be NULL, not all; a
 * stage whose only consumers are NULL is not launched.  Every output is bitwise reproducible and has the same bits
 * whatever else is asked for (fixed-order sums, no atomics, shape-only grids); grad_x of an image does not depend on
 * the rest of the batch.  workspace: qpwc_upconv4x4s2_bwd_workspace_floats() floats.  Alignment: x, weight, grad_out,
 * grad_x, grad_w, workspace 16 bytes; bias, grad_b 4.  Errors: QPWC_E_NULL, QPWC_E_SHAPE (extents < 1, channel counts,
 * mish, grad_out_pixel_stride), QPWC_E_ALIGN, QPWC_E_ALIAS (an output or the workspace overlapping an input or another
 * output); qpwc_last_error() names the argument.  All of them are found before any HIP call. */
int qpwc_upconv4x4s2_bwd(const void* x, const void* weight, const void* bias, const void* grad_out,
                         int64_t grad_out_pixel_stride, void* grad_x, void* grad_w, void* grad_b, void* workspace,
                         int B, int H, int W, int C, int F, int mish, void* stream);

/* ---- the interpolation stack (pwcnet.py:70-131): image head, Upsample of an image, the frame pyramid ----------------
 * All fp32, channels-last, dense; one summation order per shape, no atomics, shape-only grids: every output is
 * bitwise reproducible.  Every error below is found before any HIP call and qpwc_last_error() names the argument. */

/* The image head of a FrameInterpolate block, Conv2D(3, 1x1) (non_layers.py:293, 311): out (M, 3) = z (M, 64) . w2^T
 * + b2 over the M = B*H*W pixels.  w2 (3, 64) row-major, b2 (3).  z is whatever feeds the head (the stored Mish output
 * of the block's SeparableConv2D): no activation is applied here.  z and w2 16-byte aligned (16-byte loads), b2 and
 * out 4.  Errors: QPWC_E_NULL, QPWC_E_SHAPE (M < 1), QPWC_E_ALIGN, QPWC_E_ALIAS (out over an input). */
int qpwc_image_head_fwd(const void* z, const void* w2, const void* b2, void* out, int64_t M, void* stream);

/* Floats of device scratch qpwc_image_head_bwd needs: one partial of grad_w2 (192) and grad_b2 (3) per workgroup; the
 * number of workgroups comes from M alone.  Negative QPWC_E_SHAPE for M < 1. */
int64_t qpwc_image_head_bwd_workspace_floats(int64_t M);

/* Gradient of qpwc_image_head_fwd for g = grad_out = dL/d(out), (M, 3):
 *   grad_z[p,c]  = sum_k g[p,k] w2[k,c]       (M, 64)
 *   grad_w2[k,c] = sum_p g[p,k] z[p,c]        (3, 64)
 *   grad_b2[k]   = sum_p g[p,k]               (3)
 * Any of the three may be NULL, not all; z is read only when grad_w2 or grad_b2 is asked for, and the reduce launches
 * of an output that is NULL are skipped.  The weight gradients are per-workgroup partials over a grid-stride loop in a
 * fixed order, then a sum over the workgroups in order; an output has the same bits whatever else is asked for, and
 * grad_z of a pixel depends on that pixel alone.  workspace: qpwc_image_head_bwd_workspace_floats(M) floats.
 * Alignment: z, w2, grad_z, workspace 16 bytes; grad_out, grad_w2, grad_b2 4.  Errors: QPWC_E_NULL, QPWC_E_SHAPE,
 * QPWC_E_ALIGN, QPWC_E_ALIAS (an output or the workspace overlapping an input or another output). */
int qpwc_image_head_bwd(const void* z, const void* w2, const void* grad_out, void* grad_z, void* grad_w2,
                        void* grad_b2, void* workspace, int64_t M, void* stream);

/* Upsample(scale) of an image (non_layers.py:183-193; pwcnet.py:108,124): out (B,2h,2w,C) = scale * bilinear x2
 * upsampling (half-pixel centres, edge clamp: weights 0.25 / 0.75) of in (B,h,w,C), C in 1..4.  The arithmetic of
 * qpwc_upsample2x_flow_fwd: for C = 2 the same bits.  Both pointers 4-byte aligned (16 for out with C = 4, 8 with
 * C = 2).  Errors: QPWC_E_NULL, QPWC_E_SHAPE (extents < 1, C outside 1..4, h or w above 2^29), QPWC_E_ALIGN,
 * QPWC_E_ALIAS. */
int qpwc_upsample2x_image_fwd(const void* in, void* out, int B, int h, int w, int C, float scale, void* stream);

/* Adjoint of qpwc_upsample2x_image_fwd: grad_out (B,2h,2w,C) -> grad_in (B,h,w,C), a gather over the 4 x 4 taps of
 * each input pixel with the weights of qpwc_upsample2x_flow_bwd, times scale.  One launch, no workspace.  Both pointers
 * 4-byte aligned.  Errors as the forward. */
int qpwc_upsample2x_image_bwd(const void* grad_out, void* grad_in, int B, int h, int w, int C, float scale,
                              void* stream);

/* `levels` successive AvgPool2D(2, 'same') (non_layers.py:171-180; pwcnet.py:87-90) of x (B,H,W,C), C in 1..4, in one
 * launch: out (B, H / 2^levels, W / 2^levels, C), the last level only.  Every level is the mean of its 2 x 2 window
 * of the level before, ((a + b) + c + d) / 4 in row-major order -- a mean of means, not one flat block mean.  levels in
 * 1..6; H and W multiples of 2^levels (no window is clipped): anything else is QPWC_E_SHAPE and the caller pools level
 * by level.  x is read once, in 8-byte loads: x 8-byte aligned, out 4.  No gradient: the frames carry none.
 * Errors: QPWC_E_NULL, QPWC_E_SHAPE, QPWC_E_ALIGN, QPWC_E_ALIAS. */
int qpwc_avgpool_pyramid_fwd(const void* x, void* out, int B, int H, int W, int C, int levels, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* QPWC_H_ */

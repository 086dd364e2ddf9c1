/* qpwc_triplet.h -- the frame interpolator's input pipeline of libqpwc_hip.so: three frames per sample resized,
 * colour-augmented, given additive Gaussian noise, flipped, offset and laid out for InterpolatorModel, in one launch.
 * Replaces, per batch (batch_size set),
 *     read_and_resize's convert_image_dtype + tf.image.resize, augment_triplet   (qpwcnet/data/triplet_dataset_ops.py)
 *     photometric_augmentation, rotation_matrix_from_euler                        (qpwcnet/data/augment.py:10-59)
 *     preprocess                                              (qpwcnet/app/frame_interpolation/pre_train.py:110-124)
 * The conventions and the QPWC_E_* codes are those of qpwc.h.
 */
#ifndef QPWC_TRIPLET_H_
#define QPWC_TRIPLET_H_

#include "qpwc.h"

#ifdef __cplusplus
extern "C" {
#endif

/* a, b, c (B,H,W,3): the first, middle and last frame of every sample, channels-last and dense, all uint8 (QPWC_U8,
 * taken times float32(1/255)) or all fp32 (QPWC_F32, taken as they are).  They may be one buffer.  For sample n and
 * output pixel (Y, X) of the h x w output:
 *   source    (sy, sx) = (flip_ud ? h - 1 - Y : Y, flip_lr ? w - 1 - X : X): the pixel's place before the flips, which
 *             the reference applies last (rows, then columns; the three frames together);
 *   resize    rgb_f = frame f at (sy, sx) of tf.image.resize(BILINEAR) from (H, W) to (h, w): the per-axis formula of
 *             qpwc_augment_fwd (half-pixel centres, no antialias, clamped neighbours, a + (b - a) * t, rows after
 *             columns).  With H == h and W == w it is the source pixel, bit for bit;
 *   colours   p_f = (R . rgb_f) * scale + txn in fp32, the same R, scale and txn for the three frames; no clipping;
 *   noise     nz = sigma * z(sy * w + sx): three normals per pixel (R, G, B), one field per sample shared by the three
 *             frames, added before the flips and so flipped with the image;
 *   output    out_pair[n, Y, X, 0:3] = p_a + nz - 0.5, out_pair[n, Y, X, 3:6] = p_c + nz - 0.5,
 *             out_mid[n, Y, X, :] = p_b + nz - 0.5; without the - 0.5 under QPWC_TRIPLET_RAW.  No NaN scrub (the
 *             reference has none here).
 * The noise is generated in the kernel, never stored: Philox4x32-10 (multipliers 0xD2511F53, 0xCD9E8D57; Weyl
 * constants 0x9E3779B9, 0xBB67AE85) on counter (sy * w + sx, 0, 0, 0) and key (key0, key1) gives r0..r3;
 *     u1 = ((r0 >> 8) + 1) * 2^-24 in (0, 1],  u2 = (r1 >> 8) * 2^-24 in [0, 1),  u1', u2' likewise from r2, r3
 *     z0 = sqrt(-2 ln u1) cos(2 pi u2),  z1 = sqrt(-2 ln u1) sin(2 pi u2),  z2 = sqrt(-2 ln u1') cos(2 pi u2')
 * i.e. N(0, 1) truncated at sqrt(48 ln 2) = 5.77.  The reference's tf.random.normal is another stream of the same
 * distribution; the distribution is what is matched.
 * Parameters, in device memory, read by the kernel (no host synchronisation):
 *   iparams (B,4)  int32 : flip_ud, flip_lr (0 / 1), key0, key1 (bit patterns)
 *   fparams (B,16) fp32  : R[0:9] row-major, scale[9:12], txn[12:15], sigma[15]
 * The reference draws txn, the Euler angles of R ~ U(-0.3, 0.3)^3, scale = exp(U(-0.3, 0.3))^3, sigma = 0.02, flips
 * Bernoulli(0.5); the validation path is R = I, scale 1, txn 0, sigma 0, no flips.  Source indices are clamped into
 * the image whatever the parameters hold; parameters out of range give unspecified values, never an access outside a
 * buffer.
 * out_pair (B,h,w,6) / (B,6,h,w) and out_mid (B,h,w,3) / (B,3,h,w) fp32 by `layout`, written in that layout by the
 * kernel itself.  One launch of 256-pixel workgroups, B * ceil(h * w / 256) of them; no atomics: bitwise reproducible.
 * Alignment: a, b, c 1 byte (uint8) / 4 (fp32), everything else 4.  Errors, in this order and all before any HIP
 * call: QPWC_E_MODE (unknown flag bits), QPWC_E_NULL, QPWC_E_DTYPE, QPWC_E_LAYOUT, QPWC_E_SHAPE (an extent < 1; H * W
 * or 6 * h * w or the number of workgroups above 2^31 - 1 -- source offsets themselves are 64-bit), QPWC_E_ALIGN,
 * QPWC_E_ALIAS (an output overlapping a frame, a parameter array or the other output). */
#define QPWC_TRIPLET_RAW 1 /* flags: leave out the - 0.5 (augment_triplet on its own) */
int qpwc_augment_triplet_fwd(const void* a, const void* b, const void* c, int dtype, int B, int H, int W,
                             const void* iparams, const void* fparams, int h, int w, int flags, int layout,
                             void* out_pair, void* out_mid, void* stream);

/* The launch form of qpwc_augment_triplet_fwd for these arguments (host only): "triplet_pixel_kernel<vec4>" (h * w a
 * multiple of 4 and both outputs 16-byte aligned: the workgroup's pixels leave through LDS as 16-byte stores) or
 * "triplet_pixel_kernel<scalar>" (4-byte stores); "" for arguments it refuses. */
const char* qpwc_augment_triplet_fwd_kernel(int B, int h, int w, const void* out_pair, const void* out_mid);

#ifdef __cplusplus
}
#endif
#endif /* QPWC_TRIPLET_H_ */

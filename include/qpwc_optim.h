/* qpwc_optim.h -- the trainer's update step of libqpwc_hip.so: unit-wise adaptive gradient clipping followed by
 * Keras' Adam, for every parameter tensor of a model in one launch.  Replaces
 *     agc_grads = adaptive_clip_grad(params, grads, self.clip_factor, self.eps)
 *     self.optimizer.apply_gradients(zip(agc_grads, params))
 * of qpwcnet/app/optical_flow/train.py:294-296 and app/frame_interpolation/pre_train.py:67-69 (core/agc.py:39-49;
 * tf.keras.optimizers.Adam, dense path, no amsgrad).  The conventions and the QPWC_E_* codes are those of qpwc.h.
 */
#ifndef QPWC_OPTIM_H_
#define QPWC_OPTIM_H_

#include "qpwc.h"

#ifdef __cplusplus
extern "C" {
#endif

/* One update step.  Both tables live in DEVICE memory, 8-byte aligned, and are read by the kernel:
 *
 *   tensors  n_tensors entries of 4 pointers (32 bytes): { float* p; const float* g; float* m; float* v; } -- a
 *            parameter, its gradient and Adam's two moments, all fp32, dense, with the same element count.  A null g
 *            skips every unit of that tensor: p, m and v keep their bits.
 *   units    n_units entries of 3 int64_t (24 bytes): { tensor, offset, length } -- elements [offset, offset + length)
 *            of tensors[tensor] share one AGC norm.  The units of a tensor must tile it without overlap (elements that
 *            no unit covers are not updated).  On the torch layouts every unit of the reference's Keras-layout rule
 *            (norm over axes 0, 1, 2 of a rank-4 kernel, over everything for rank <= 1) is one contiguous run:
 *              Conv2D, pointwise  (O,I,kh,kw)  one unit per [o] slice
 *              Conv2DTranspose    (I,O,kh,kw)  one unit per [i] slice (Keras stores (kh,kw,out,in))
 *              depthwise          (C,1,kh,kw)  the whole tensor (Keras stores (kh,kw,C,1))
 *              bias, gamma, beta  (n)          the whole tensor
 *            An entry with tensor outside [0, n_tensors), a negative offset or a length < 1 is skipped.
 *
 * Per unit, with pn = sqrt(sum p^2), gn = sqrt(sum g^2), mx = max(pn, agc_eps) * clip_factor:
 *     g' = g if gn < mx, else g * (mx / max(gn, 1e-6));  a NaN in pn or gn makes the unit's whole g' NaN
 * (tf.maximum propagates NaN and the NaN comparison selects the clipped branch); other units are not touched.
 * clip_factor <= 0: no clipping, g' = g (plain Keras Adam, pre_train.py:70).  Then per element
 *     m += (g' - m) * (1 - beta1);  v += (g'^2 - v) * (1 - beta2);  p -= alpha * m / (sqrt(v) + epsilon)
 * where alpha = lr * sqrt(1 - beta2^t) / (1 - beta1^t), t = iterations + 1, is the caller's: Keras folds both bias
 * corrections into the step size and adds epsilon to the uncorrected sqrt(v).
 *
 * The sums are taken in a fixed order (no atomics): two calls on the same bits give the same bits.  Units whose p, g,
 * m and v addresses share one 16-byte phase move as 16-byte accesses, any other unit as scalars.
 * Errors, all before any HIP call: QPWC_E_NULL (tensors, units), QPWC_E_SHAPE (n_tensors < 1, n_units outside
 * [1, 2^31 - 1]), QPWC_E_RANGE (a beta outside [0, 1), epsilon <= 0, agc_eps <= 0, alpha not finite; NaN fails each),
 * QPWC_E_ALIGN (a table not 8-byte aligned), QPWC_E_ALIAS (the tables overlap). */
int qpwc_agc_adam_step(const void* tensors, int n_tensors, const void* units, int64_t n_units, float alpha, float beta1,
                       float beta2, float epsilon, float clip_factor, float agc_eps, void* stream);

/* Host only: the launch form qpwc_agc_adam_step takes for n_units -- "agc_adam_kernel<one unit per wave>" while
 * ceil(n_units / 4) workgroups fit the grid cap (1024), "agc_adam_kernel<grid-stride>" above it, where a wave takes
 * more than one unit.  "" for n_units outside [1, 2^31 - 1]. */
const char* qpwc_agc_adam_step_kernel(int64_t n_units);

#ifdef __cplusplus
}
#endif
#endif /* QPWC_OPTIM_H_ */

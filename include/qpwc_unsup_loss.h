/* qpwc_unsup_loss.h -- the label-free flow training losses of libqpwc_hip.so: a photometric term (UFlow's soft ternary
 * census, or Charbonnier on RGB) between prv and nxt warped by the flow, over the pixels whose sample stays inside the
 * image and is not occluded, plus edge-aware first-order smoothness.  1..8 levels, each with its own frames: one forward
 * launch for all levels plus a fixed-order fold, one backward launch.
 * Goes beyond the reference, whose losses all take a ground truth (qpwcnet/train/loss.py) and whose occlusion estimate
 * (qpwcnet/core/occlusion.py) is wired into none of them.
 * The conventions and the QPWC_E_* codes are those of qpwc.h; "the first defect in this order" as qpwc_masked_loss.h.
 * Non-finite flows are out of scope: nothing is promised for a level that holds one.
 */
#ifndef QPWC_UNSUP_LOSS_H_
#define QPWC_UNSUP_LOSS_H_

#include "qpwc.h"

#ifdef __cplusplus
extern "C" {
#endif

#define QPWC_UNSUP_CENSUS 0
#define QPWC_UNSUP_CHARBONNIER 1

/* Floats of workspace qpwc_unsup_loss_fwd needs and qpwc_unsup_loss_bwd reads: 4 per tile of 8 x 32 pixels (the tile's
 * three partial sums and its 32-bit partial count; tiles per level = B * ceil(h / 8) * ceil(w / 32)), then 7 planes of
 * B * h * w floats per level (below).  A QPWC_E_* code (negative) for arguments it refuses (QPWC_E_NULL, QPWC_E_MODE,
 * QPWC_E_SHAPE, by the rules below). */
int64_t qpwc_unsup_loss_workspace_floats(int kind, int B, const int* h, const int* w, int n_levels);

/* prv[l], nxt[l]: fp32 (B,h[l],w[l],3), channels-last, constants.  flow[l] = (u, v): fp32 or fp16 by flow_dtype[l],
 * (B,h[l],w[l],2) / (B,2,h[l],w[l]) by `layout`, converted to fp32 on load, in level pixels.  occluded: NULL, or an array
 * whose entries are NULL or uint8 (B,h[l],w[l]), nonzero = occluded.  Per level pixel p = (x, y), all in fp32:
 *   warp      q = (x + u, y + v); floor = clamp(floor(q), 0, max(size - 2, 0)) and alpha = clamp(q - floor, 0, 1) per
 *             axis, the second tap min(floor + 1, size - 1): the CLAMP rule of qpwc_warp_fwd, every product and sum
 *             separately rounded: top = ax * (tr - tl) + tl, bot = ax * (br - bl) + bl, value = ay * (bot - top) + top
 *   inside_p  0 <= qx <= w - 1 and 0 <= qy <= h - 1
 *   m_p       inside_p and not occluded_p; census: and 3 <= x < w - 3 and 3 <= y < h - 3 (h < 7 or w < 7: count 0)
 *   census    g = 255 * (0.2989 r + 0.587 g + 0.114 b) of prv at p, and gw = the four corners' g of nxt blended as above
 *             (at every pixel, whatever m_p); over the 48 offsets d of the 7 x 7 patch t(p,d) = D / sqrt(0.81 + D^2) with
 *             D = g(p+d) - g(p), once for prv and once for gw; e = (t_prv - t_w)^2; dist_p = sum_d e / (0.1 + e);
 *             term_p = (dist_p + eps)^q
 *   charbonnier   term_p = (1/3) sum_c ((prv_c - warped_c)^2 + eps^2)^q on RGB
 *   count_l   = sum_p m_p over the batch, an exact integer
 *   photo_l   = sum_p [m_p] term_p / max(count_l, 1); count_l = 0: 0, and an all-zero photometric gradient
 *   smooth_l  = (sx + sy) / 2; sx = the mean over (B, h, w-1, 2) of wx * sqrt(D^2 + smooth_eps^2), D the flow difference
 *             along x, wx = exp(-edge * mean_c |prv(x+1,y) - prv(x,y)|); sy the same along y; an axis of extent 1 gives 0
 *   loss_l    = photo_l + smooth_weight * smooth_l
 * out_losses, out_photo, out_smooth: float[n_levels].  out_counts: int64[n_levels].
 * Saved for the backward, in `workspace` behind the partial sums, per level 7 planes of (B,h,w) floats:
 *   m_p q (dist_p + eps)^(q-1) (charbonnier: unused), g of prv, gw, d gw / d qx, d gw / d qy (charbonnier: m_p d term_p /
 *   d qx, / d qy), wx, wy.  d gw / d q is the bilinear derivative where inside_p and exactly 0 where not.
 * Kernels: unsup_loss_fwd_kernel, one workgroup per (level, image, tile of 8 x 32 pixels) through a per-level prefix
 * table in its arguments, the tile's prv grey and warped grey staged in LDS with the 3-pixel halo; then
 * unsup_loss_fold_kernel.  Grids depend on the shapes only, sums are in a fixed order, no atomics: two calls give the
 * same bits.  No form is chosen by alignment; every access is element-wise.
 * `workspace` holds qpwc_unsup_loss_workspace_floats floats and needs no initialisation.
 * Errors, all before any HIP call, the first defect in this order: QPWC_E_NULL (prv, nxt, flow, h, w, flow_dtype,
 * out_losses, out_photo, out_smooth, out_counts, workspace), QPWC_E_MODE (kind), QPWC_E_SHAPE (n_levels outside 1..8; an
 * extent < 1; more than 2^31 - 1 pixels in a level or tiles in all), QPWC_E_LAYOUT, QPWC_E_RANGE (NaN; eps <= 0;
 * smooth_eps <= 0; q <= 0; edge < 0; smooth_weight < 0), QPWC_E_DTYPE, QPWC_E_NULL (a NULL prv[l], nxt[l] or flow[l]),
 * QPWC_E_ALIGN (prv, nxt 4 bytes, a flow its element size, out_losses, out_photo, out_smooth, workspace 4, out_counts 8),
 * QPWC_E_ALIAS (an output or the workspace overlapping an input or another output). */
int qpwc_unsup_loss_fwd(int kind, float q, float eps, float smooth_weight, float edge, float smooth_eps,
                        const void* const* prv, const void* const* nxt, const void* const* flow,
                        const void* const* occluded, int B, const int* h, const int* w, const int* flow_dtype, int layout,
                        int n_levels, void* out_losses, void* out_photo, void* out_smooth, void* out_counts,
                        void* workspace, void* stream);

/* The forward kernel qpwc_unsup_loss_fwd takes for these arguments (host only): "unsup_loss_fwd_kernel<census>" or
 * "unsup_loss_fwd_kernel<charbonnier>"; "" for arguments it refuses. */
const char* qpwc_unsup_loss_fwd_kernel(int kind, int B, const int* h, const int* w, int n_levels);

/* grad_flow[l] = grad_losses[l] * d loss_l / d flow[l] in flow_dtype[l] and `layout`, every level in one launch
 * (unsup_loss_bwd_kernel, the forward's grid).  A gather, exact: per pixel r the 48 census pairs in which r is a
 * neighbour and the 48 in which it is the centre, each weighted by the saved m_p q (dist_p + eps)^(q-1) of its centre p,
 * over max(counts[l], 1) and times the saved d gw / d q of r; plus r's up to four smoothness neighbours.  A pixel whose
 * sample is outside the image gets exactly zero photometric gradient.  flow, workspace, counts: what
 * qpwc_unsup_loss_fwd read and wrote, with the same kind, shapes and layout; counts and grad_losses (float[n_levels]) are
 * read on the device.
 * Errors: QPWC_E_NULL, QPWC_E_MODE, QPWC_E_SHAPE, QPWC_E_LAYOUT, QPWC_E_RANGE (smooth_weight, smooth_eps as above),
 * QPWC_E_DTYPE, QPWC_E_NULL (a NULL flow[l] or grad_flow[l]), QPWC_E_ALIGN (a flow and a grad_flow its element size,
 * workspace and grad_losses 4, counts 8), QPWC_E_ALIAS (a grad_flow overlapping an input or another grad_flow). */
int qpwc_unsup_loss_bwd(int kind, float smooth_weight, float smooth_eps, const void* const* flow, const void* workspace,
                        const void* counts, const void* grad_losses, void* const* grad_flow, int B, const int* h,
                        const int* w, const int* flow_dtype, int layout, int n_levels, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* QPWC_UNSUP_LOSS_H_ */

// The three flow losses over the valid pixels only (include/qpwc_masked_loss.h): the MASKED variant of loss.hip's
// FlowMseLossV2, FlowMseLoss and FlowMseLossFineTune for sparse ground truth (KITTI) and unknown pixels (Sintel).
//   forward : one launch for all levels (masked_loss_tile_kernel or masked_loss_pixel_kernel) that writes, per workgroup
//             and level, the sum of the valid level pixels' terms (fp32) and their number (an integer), + one fixed-order
//             fold (masked_loss_fold_kernel) that divides by the count it has just summed; with `dpred` the forward also
//             stores d term / d y_pred (fp32, not yet divided by the count; exactly 0 at an invalid level pixel);
//   backward: one launch for all levels, grad_pred[l] = grad_losses[l] * dpred[l] / (count_l's denominator), the count
//             read from device memory.
// Validity is a selection, never a product: what an invalid pixel holds (NaN, Inf, 1e10, garbage) reaches no arithmetic.
// Deterministic as loss.hip: grids depend on the shapes only, fixed-order sums, no atomics.
// No form is chosen by alignment: the C boundary refuses a y_true off the 16-byte grid and a mask off the 4-byte grid.
namespace qpwc {
constexpr int kLossThreads = 256;
constexpr int kLossPixBlocks = 1024;    // pixel path: partial sums per level
constexpr int kLossTileBlocks = 2048;   // tile path: at most this many workgroups, each walks its tiles
constexpr int kLossTile = 32;           // tile path: 32 x 32 ground-truth pixels per tile (8 KB of fp32 flow)
constexpr int kLossBwdBlocks = 1024;
}  // namespace qpwc
#include "loss_common.h"

namespace qpwc {

// FlowMseLossV2 of every level from one read of the ground truth and the mask: the tile walk of loss_common.h with a
// count plane beside the sums.
template <int LAYOUT>
__global__ __launch_bounds__(kLossThreads) void masked_loss_tile_kernel(const float* __restrict__ gt,
                                                                      const unsigned char* __restrict__ valid,
                                                                      MaskedLevels lv, int n_levels, int B, int H,
                                                                      int W, float delta, float* __restrict__ psum,
                                                                      int* __restrict__ pcnt) {
    __shared__ float2 raw[kLossTile * kLossTile];            // (y, x) -> (sum v x, sum v y): 8 KB
    __shared__ float rawn[kLossTile * kLossTile];            // (y, x) -> sum v: 4 KB
    __shared__ float2 aux[kLossTile * kLossTile / 2];        // 4 KB
    __shared__ float auxn[kLossTile * kLossTile / 2];        // 2 KB
    __shared__ float red[kLossMaxLevels][kLossWaves];
    __shared__ int redn[kLossMaxLevels][kLossWaves];
    loss_tile_body<true, LAYOUT>(gt, valid, lv, n_levels, B, H, W, delta, psum, pcnt, raw, rawn, aux, auxn, red, redn);
}

// One thread per level pixel, blockIdx.y = level: the pixel walk of loss_common.h.
template <int KIND, int LAYOUT>
__global__ __launch_bounds__(kLossThreads) void masked_loss_pixel_kernel(const float* __restrict__ gt,
                                                                       const unsigned char* __restrict__ valid,
                                                                       MaskedLevels lv, int B, int H, int W, float p0,
                                                                       float p1, float* __restrict__ psum,
                                                                       int* __restrict__ pcnt) {
    __shared__ float red[kLossWaves];
    __shared__ int redn[kLossWaves];
    loss_pixel_body<true, KIND, LAYOUT>(gt, valid, lv, B, H, W, 2, p0, p1, psum, pcnt, red, redn);
}

// counts[l] = the nblk partial counts of level l; out[l] = (its nblk partial sums, folded in a fixed order) / denominator
__global__ __launch_bounds__(kLossThreads) void masked_loss_fold_kernel(const float* __restrict__ psum,
                                                                      const int* __restrict__ pcnt, int nblk,
                                                                      int per_element, float* __restrict__ out,
                                                                      int64_t* __restrict__ counts) {
    __shared__ float red[kLossWaves];
    __shared__ long long redn[kLossWaves];
    const int l = blockIdx.x;
    loss_fold_body<true>(psum, pcnt, nblk, red, redn);
    if (threadIdx.x == 0) {
        const int64_t count = loss_sum4(redn);
        counts[l] = count;
        out[l] = (float)((double)loss_sum4(red) / masked_denominator(count, per_element));
    }
}

// grad_pred[l] = (grad_losses[l] / denominator(counts[l])) * dpred[l] for every level in one launch (blockIdx.y = level)
__global__ __launch_bounds__(kLossThreads) void masked_loss_bwd_kernel(MaskedGrads lg, const int64_t* __restrict__ counts,
                                                                     int per_element,
                                                                     const float* __restrict__ grad_losses) {
    const int l = blockIdx.y;
    loss_scale_body(lg, (float)((double)grad_losses[l] / masked_denominator(counts[l], per_element)), lg.n[l] % 4 == 0);
}

// ---- host side ------------------------------------------------------------------------------------------------------

// floats: n_levels * kLossTileBlocks partial sums, then as many 32-bit partial counts
int64_t masked_loss_workspace_floats(int n_levels) { return (int64_t)n_levels * kLossTileBlocks * 2; }

// Which forward kernel masked_loss_fwd_launch takes for these arguments (host only).
const char* masked_loss_fwd_kernel(int kind, int H, int W, const int* h, const int* w, int n) {
    MaskedLevels lv = {};
    bool tile;
    loss_plan(kind, true, 1, H, W, h, w, n, lv, tile);
    return tile ? "masked_loss_tile_kernel" : "masked_loss_pixel_kernel";
}

int masked_loss_fwd_launch(int kind, float p0, float p1, const float* gt, const unsigned char* valid, int B, int H, int W,
                           int layout, const void* const* pred, const int* h, const int* w, const int* pred_dtype, int n,
                           float* out, int64_t* counts, void* const* dpred, void* const* gt_out, void* const* valid_out,
                           float* ws, hipStream_t s) {
    MaskedLevels lv = {};
    loss_fill_levels(lv, kind, B, H, W, 2, pred, h, w, pred_dtype, n, dpred, gt_out);
    for (int i = 0; i < n; ++i) lv.valid_out[i] = valid_out ? (unsigned char*)valid_out[i] : nullptr;
    bool tile;
    const int nblk = loss_plan(kind, true, B, H, W, h, w, n, lv, tile);
    float* psum = ws;
    int* pcnt = reinterpret_cast<int*>(ws + (int64_t)n * nblk);
    if (tile) {
        loss_launch(masked_loss_tile_kernel<QPWC_NHWC>, masked_loss_tile_kernel<QPWC_NCHW>, layout, dim3(nblk), s, gt,
                    valid, lv, n, B, H, W, p0, psum, pcnt);
    } else {
#define PIXEL_ARGS layout, dim3(nblk, n), s, gt, valid, lv, B, H, W, p0, p1, psum, pcnt
        switch (kind) {
            QPWC_LOSS_KIND(masked_loss_pixel_kernel, QPWC_LOSS_FLOW_MSE_V2, PIXEL_ARGS);
            QPWC_LOSS_KIND(masked_loss_pixel_kernel, QPWC_LOSS_FLOW_MSE, PIXEL_ARGS);
            default:   // validated at the boundary
                QPWC_LOSS_KIND(masked_loss_pixel_kernel, QPWC_LOSS_FLOW_FINETUNE, PIXEL_ARGS);
        }
#undef PIXEL_ARGS
    }
    const int rc = check_launch(tile ? "masked_loss_tile_kernel" : "masked_loss_pixel_kernel");
    if (rc != QPWC_OK) return rc;
    hipLaunchKernelGGL(masked_loss_fold_kernel, dim3(n), dim3(kLossThreads), 0, s, psum, pcnt, nblk,
                       kind == QPWC_LOSS_FLOW_MSE_V2 ? 1 : 0, out, counts);
    return check_launch("masked_loss_fold_kernel");
}

int masked_loss_bwd_launch(int kind, const void* const* dpred, const int64_t* counts, const float* grad_losses,
                           void* const* grad_pred, const int64_t* n_elems, const int* pred_dtype, int n, hipStream_t s) {
    MaskedGrads lg = {};
    loss_fill_grads(lg, dpred, grad_pred, n_elems, pred_dtype, n);
    hipLaunchKernelGGL(masked_loss_bwd_kernel, dim3(kLossBwdBlocks, n), dim3(kLossThreads), 0, s, lg, counts,
                       kind == QPWC_LOSS_FLOW_MSE_V2 ? 1 : 0, grad_losses);
    return check_launch("masked_loss_bwd_kernel");
}

}  // namespace qpwc

// Multi-scale training losses (qpwcnet/train/loss.py): FlowMseLossV2, FlowMseLoss, FlowMseLossFineTune and
// AutoResizeMseLoss of up to 8 prediction levels against ONE full-resolution ground truth.
//   forward : one partial-sum launch for all levels (loss_area_tile_kernel or loss_pixel_kernel) + one fixed-order
//             fold (loss_final_kernel); with `dpred` the forward also stores d loss_l / d y_pred_l (fp32);
//   backward: one launch for all levels, grad_pred[l] = grad_losses[l] * dpred[l] in the prediction's dtype.
// Deterministic by construction: grids depend on the shapes only, every thread sums in a fixed order, the partial sums
// are folded by shuffles and a fixed-order LDS step; no atomics.
namespace qpwc {
constexpr int kLossThreads = 256;
constexpr int kLossPixBlocks = 1024;    // pixel path: partial sums per level
constexpr int kLossTileBlocks = 2048;   // tile path: at most this many workgroups, each walks its tiles
constexpr int kLossTile = 32;           // tile path: 32 x 32 ground-truth pixels per tile (8 KB of fp32 flow)
constexpr int kLossBwdBlocks = 1024;
}  // namespace qpwc
#include "loss_common.h"

namespace qpwc {

// FlowMseLossV2 of every level from one read of the ground truth: the tile walk of loss_common.h.
template <int LAYOUT>
__global__ __launch_bounds__(kLossThreads) void loss_area_tile_kernel(const float* __restrict__ gt, LossLevels lv,
                                                                      int n_levels, int B, int H, int W, float delta,
                                                                      float* __restrict__ partial) {
    __shared__ loss_f32x4 raw4[kLossTile * kLossTile / 2];   // (y, x) -> (flow x, flow y) cells: 8 KB
    __shared__ float2 aux[kLossTile * kLossTile / 2];         // 4 KB
    __shared__ float red[kLossMaxLevels][kLossWaves];
    loss_tile_body<false, LAYOUT>(gt, nullptr, lv, n_levels, B, H, W, delta, partial, nullptr,
                                  reinterpret_cast<float2*>(raw4), nullptr, aux, nullptr, red, nullptr);
}

// One thread per prediction pixel, blockIdx.y = level: the pixel walk of loss_common.h.
template <int KIND, int LAYOUT>
__global__ __launch_bounds__(kLossThreads) void loss_pixel_kernel(const float* __restrict__ gt, LossLevels lv, int B,
                                                                  int H, int W, int C, float p0, float p1,
                                                                  float* __restrict__ partial) {
    __shared__ float red[kLossWaves];
    loss_pixel_body<false, KIND, LAYOUT>(gt, nullptr, lv, B, H, W, C, p0, p1, partial, nullptr, red, nullptr);
}

// out[l] = inv_n[l] * (the nblk partial sums of level l, folded in a fixed order)
__global__ __launch_bounds__(kLossThreads) void loss_final_kernel(const float* __restrict__ partial, int nblk,
                                                                  LossLevels lv, float* __restrict__ out) {
    __shared__ float red[kLossWaves];
    const int l = blockIdx.x;
    loss_fold_body<false>(partial, nullptr, nblk, red, nullptr);
    if (threadIdx.x == 0) out[l] = loss_sum4(red) * lv.inv_n[l];
}

// grad_pred[l] = grad_losses[l] * dpred[l] for every level in one launch (blockIdx.y = level)
__global__ __launch_bounds__(kLossThreads) void loss_bwd_kernel(LossGrads lg, const float* __restrict__ grad_losses) {
    const int l = blockIdx.y;
    loss_scale_body(lg, grad_losses[l], lg.vec[l]);
}

// ---- host side ------------------------------------------------------------------------------------------------------

int64_t loss_workspace_floats(int n_levels) { return (int64_t)n_levels * kLossTileBlocks; }

// Which forward kernel loss_fwd_launch takes for these arguments (host only).
const char* loss_fwd_kernel(int kind, int H, int W, const int* h, const int* w, int n, const void* gt) {
    LossLevels lv = {};
    bool tile;
    loss_plan(kind, (uintptr_t)gt % 16 == 0, 1, H, W, h, w, n, lv, tile);
    return tile ? "loss_area_tile_kernel" : "loss_pixel_kernel";
}

int loss_fwd_launch(int kind, float p0, float p1, const float* gt, int B, int H, int W, int C, int layout,
                    const void* const* pred, const int* h, const int* w, const int* pred_dtype, int n, float* out,
                    void* const* dpred, void* const* gt_out, float* ws, hipStream_t s) {
    LossLevels lv = {};
    loss_fill_levels(lv, kind, B, H, W, C, pred, h, w, pred_dtype, n, dpred, gt_out);
    bool tile;
    const int nblk = loss_plan(kind, (uintptr_t)gt % 16 == 0, B, H, W, h, w, n, lv, tile);
    if (tile) {
        loss_launch(loss_area_tile_kernel<QPWC_NHWC>, loss_area_tile_kernel<QPWC_NCHW>, layout, dim3(nblk), s, gt, lv, n,
                    B, H, W, p0, ws);
    } else {
#define PIXEL_ARGS layout, dim3(nblk, n), s, gt, lv, B, H, W, C, p0, p1, ws
        switch (kind) {
            QPWC_LOSS_KIND(loss_pixel_kernel, QPWC_LOSS_FLOW_MSE_V2, PIXEL_ARGS);
            QPWC_LOSS_KIND(loss_pixel_kernel, QPWC_LOSS_FLOW_MSE, PIXEL_ARGS);
            QPWC_LOSS_KIND(loss_pixel_kernel, QPWC_LOSS_FLOW_FINETUNE, PIXEL_ARGS);
            default:   // validated at the boundary
                QPWC_LOSS_KIND(loss_pixel_kernel, QPWC_LOSS_AUTORESIZE_MSE, PIXEL_ARGS);
        }
#undef PIXEL_ARGS
    }
    const int rc = check_launch(tile ? "loss_area_tile_kernel" : "loss_pixel_kernel");
    if (rc != QPWC_OK) return rc;
    hipLaunchKernelGGL(loss_final_kernel, dim3(n), dim3(kLossThreads), 0, s, ws, nblk, lv, out);
    return check_launch("loss_final_kernel");
}

int loss_bwd_launch(const void* const* dpred, const float* grad_losses, void* const* grad_pred, const int64_t* n_elems,
                    const int* pred_dtype, int n, hipStream_t s) {
    LossGrads lg = {};
    loss_fill_grads(lg, dpred, grad_pred, n_elems, pred_dtype, n);
    for (int i = 0; i < n; ++i)
        lg.vec[i] = n_elems[i] % 4 == 0 && (uintptr_t)dpred[i] % 16 == 0 &&
                    (uintptr_t)grad_pred[i] % (lg.f16[i] ? 8 : 16) == 0;
    hipLaunchKernelGGL(loss_bwd_kernel, dim3(kLossBwdBlocks, n), dim3(kLossThreads), 0, s, lg, grad_losses);
    return check_launch("loss_bwd_kernel");
}

}  // namespace qpwc

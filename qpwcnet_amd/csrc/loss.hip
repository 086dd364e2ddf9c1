// Multi-scale training losses (qpwcnet/train/loss.py): FlowMseLossV2, FlowMseLoss, FlowMseLossFineTune and
// AutoResizeMseLoss of up to 8 prediction levels against ONE full-resolution ground truth.
//   forward : one partial-sum launch for all levels (loss_area_tile_kernel or loss_pixel_kernel) + one fixed-order
//             fold (loss_final_kernel); with `dpred` the forward also stores d loss_l / d y_pred_l (fp32);
//   backward: one launch for all levels, grad_pred[l] = grad_losses[l] * dpred[l] in the prediction's dtype.
// Deterministic by construction: grids depend on the shapes only, every thread sums in a fixed order, the partial sums
// are folded by shuffles and a fixed-order LDS step; no atomics.
#include "common.h"
#include "launch.h"
#include "loss_common.h"

namespace qpwc {

constexpr int kLossThreads = 256;
constexpr int kLossPixBlocks = 1024;    // pixel path: partial sums per level
constexpr int kLossTileBlocks = 2048;   // tile path: at most this many workgroups, each walks its tiles
constexpr int kLossTile = 32;           // tile path: 32 x 32 ground-truth pixels per tile (8 KB of fp32 flow)
constexpr int kLossBwdBlocks = 1024;

struct LossLevels {
    const void* pred[kLossMaxLevels];   // NULL: taken as zero (gt_out only)
    float* dpred[kLossMaxLevels];       // NULL: not written
    float* gt_out[kLossMaxLevels];      // NULL: not written
    int h[kLossMaxLevels], w[kLossMaxLevels];
    int sh[kLossMaxLevels], sw[kLossMaxLevels];   // area factors H / h, W / w
    int f16[kLossMaxLevels];
    float fscale[kLossMaxLevels];       // flow scale h / H on both channels (1 for AutoResizeMseLoss)
    float inv_area[kLossMaxLevels];     // 1 / (sh * sw)
    float inv_n[kLossMaxLevels];        // 1 / number of averaged terms
    float lscale[kLossMaxLevels];       // FlowMseLossV2: 2 / (w + h)
    float ry_scale[kLossMaxLevels], rx_scale[kLossMaxLevels];   // bilinear: (float)H / h, (float)W / w
    // tile path: the sum pyramid of one tile; step s sums step_ry x step_rx cells (1 or 2 each) of the previous step
    // and evaluates level step_level[s] on the result (-1: an intermediate step)
    int nsteps;
    int step_ry[kLossMaxSteps], step_rx[kLossMaxSteps], step_level[kLossMaxSteps];
};

namespace {

// the two channels of prediction pixel (b, y, x) of level l as fp32
template <int LAYOUT>
__device__ __forceinline__ float2 ld_pred_pixel(const LossLevels& lv, int l, int64_t b, int y, int x) {
    const int64_t o = pix_offset<LAYOUT>(b, y, x, lv.h[l], lv.w[l], 2), cs = chan_stride<LAYOUT>(lv.h[l], lv.w[l]);
    return make_float2(ld_pred(lv.pred[l], o, lv.f16[l]), ld_pred(lv.pred[l], o + cs, lv.f16[l]));
}

// One flow pixel of level l (ground truth resampled and scaled, prediction pv): its term; stores its derivative and
// ground truth where asked.
template <int KIND, int LAYOUT>
__device__ __forceinline__ float flow_pixel(const LossLevels& lv, int l, int64_t b, int y, int x, float gx, float gy,
                                            float p0, float p1, float2 pv) {
    const int h = lv.h[l], w = lv.w[l];
    const int64_t o = pix_offset<LAYOUT>(b, y, x, h, w, 2), cs = chan_stride<LAYOUT>(h, w);
    const float px = pv.x, py = pv.y;
    float dx, dy;
    const float t = flow_term<KIND>(gx, gy, px, py, lv.lscale[l], p0, p1, dx, dy);
    if (float* d = lv.dpred[l]) {
        d[o] = dx * lv.inv_n[l];
        d[o + cs] = dy * lv.inv_n[l];
    }
    if (float* g = lv.gt_out[l]) {
        g[o] = gx;
        g[o + cs] = gy;
    }
    return t;
}

}  // namespace

// FlowMseLossV2 of every level from one read of the ground truth: a workgroup owns 32x32 GT pixels at a time (two
// 16-byte loads per thread; the next tile's loads are in flight while this one is reduced), sums them in LDS by 2x2
// steps up to every level's area factor (nested powers of two with sh * sw >= 4: at most one output per thread) and
// evaluates that level's pixels of the tile on the way.
template <int LAYOUT>
__global__ __launch_bounds__(kLossThreads) void loss_area_tile_kernel(const float* __restrict__ gt, LossLevels lv,
                                                                      int n_levels, int B, int H, int W, float delta,
                                                                      float* __restrict__ partial) {
    __shared__ loss_f32x4 raw4[kLossTile * kLossTile / 2];   // (y, x) -> (flow x, flow y) cells: 8 KB
    __shared__ float2 aux[kLossTile * kLossTile / 2];         // 4 KB
    __shared__ float red[kLossMaxLevels][kLossThreads / 64];
    float2* raw = reinterpret_cast<float2*>(raw4);
    const int tid = threadIdx.x;
    const int tiles_x = W / kLossTile, tiles_y = H / kLossTile;
    const int ntiles = B * tiles_y * tiles_x;
    float acc[kLossMaxLevels];
#pragma unroll
    for (int k = 0; k < kLossMaxLevels; ++k) acc[k] = 0.0f;

    // 512 float4 per tile, two per thread.  NHWC: row i / 16 holds 16 float4 (2 pixels each);
    // NCHW: plane i / 256, row (i / 8) % 32 holds 8 float4 (4 pixels of one channel each)
    const loss_f32x4* g4 = reinterpret_cast<const loss_f32x4*>(gt);
    auto gt_index = [&](int tile, int i) -> int64_t {
        const int tx = tile % tiles_x, ty = (tile / tiles_x) % tiles_y, b = tile / (tiles_x * tiles_y);
        if (LAYOUT == QPWC_NHWC) {
            const int row = i >> 4, c4 = i & 15;
            return ((((int64_t)b * H + ty * kLossTile + row) * W + tx * kLossTile) * 2) / 4 + c4;
        }
        const int c = i >> 8, row = (i >> 3) & 31, c4 = i & 7;
        return ((((int64_t)b * 2 + c) * H + ty * kLossTile + row) * W + tx * kLossTile) / 4 + c4;
    };
    loss_f32x4 v[2];
    if ((int)blockIdx.x < ntiles) {
#pragma unroll
        for (int k = 0; k < 2; ++k) v[k] = __builtin_nontemporal_load(g4 + gt_index(blockIdx.x, tid + k * kLossThreads));
    }
    for (int tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const int tx = tile % tiles_x, ty = (tile / tiles_x) % tiles_y, b = tile / (tiles_x * tiles_y);
        // this thread's prediction pixel of every level of the tile, all loads issued up front: waiting for each
        // level's load inside its step serialised five memory latencies per tile
        float2 pv[kLossMaxSteps];
        {
            int fy = 1, fx = 1;
#pragma unroll
            for (int s = 0; s < kLossMaxSteps; ++s) {
                pv[s] = make_float2(0.0f, 0.0f);
                if (s < lv.nsteps) {
                    fy *= lv.step_ry[s];
                    fx *= lv.step_rx[s];
                    const int l = lv.step_level[s], nx = kLossTile / fx;
                    if (l >= 0 && tid < (kLossTile / fy) * nx)
                        pv[s] = ld_pred_pixel<LAYOUT>(lv, l, b, ty * (kLossTile / fy) + tid / nx,
                                                      tx * nx + tid % nx);
                }
            }
        }
        __syncthreads();                                   // the previous tile's steps are done with raw / aux
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            const int i = tid + k * kLossThreads;
            if (LAYOUT == QPWC_NHWC) {
                raw4[i] = v[k];                            // 2 pixels = 2 cells
            } else {
                const int c = i >> 8, row = (i >> 3) & 31, c4 = i & 7;
                float* cell = reinterpret_cast<float*>(raw + row * kLossTile + c4 * 4) + c;
                cell[0] = v[k].x;
                cell[2] = v[k].y;
                cell[4] = v[k].z;
                cell[6] = v[k].w;
            }
        }
        const int next = tile + gridDim.x;
        if (next < ntiles) {
#pragma unroll
            for (int k = 0; k < 2; ++k) v[k] = __builtin_nontemporal_load(g4 + gt_index(next, tid + k * kLossThreads));
        }
        __syncthreads();
        int fy = 1, fx = 1;
#pragma unroll
        for (int s = 0; s < kLossMaxSteps; ++s) {
            if (s >= lv.nsteps) continue;
            const int ry = lv.step_ry[s], rx = lv.step_rx[s], l = lv.step_level[s];
            const float2* src = (s & 1) ? aux : raw;
            float2* dst = (s & 1) ? raw : aux;
            const int pnx = kLossTile / fx;
            fy *= ry;
            fx *= rx;
            const int ny = kLossTile / fy, nx = kLossTile / fx;
            for (int o = tid; o < ny * nx; o += kLossThreads) {
                const int oy = o / nx, ox = o - oy * nx;
                const float2* p = src + (oy * ry) * pnx + ox * rx;
                float2 sum = p[0];
                if (rx == 2) sum = f2add(sum, p[1]);
                if (ry == 2) {
                    float2 q = p[pnx];
                    if (rx == 2) q = f2add(q, p[pnx + 1]);
                    sum = f2add(sum, q);
                }
                dst[o] = sum;
                if (l >= 0) {
                    // power-of-two area: the mean is exact; then the flow scale h / H on both channels
                    const float t = flow_pixel<QPWC_LOSS_FLOW_MSE_V2, LAYOUT>(
                        lv, l, b, ty * ny + oy, tx * nx + ox, (sum.x * lv.inv_area[l]) * lv.fscale[l],
                        (sum.y * lv.inv_area[l]) * lv.fscale[l], delta, 0.0f, pv[s]);
#pragma unroll
                    for (int k = 0; k < kLossMaxLevels; ++k) acc[k] += k == l ? t : 0.0f;   // no dynamic register index
                }
            }
            __syncthreads();
        }
    }
    const int lane = tid & 63, wid = tid >> 6;
#pragma unroll
    for (int k = 0; k < kLossMaxLevels; ++k) {
        const float s = loss_wave_sum(acc[k]);
        if (lane == 0) red[k][wid] = s;
    }
    __syncthreads();
    if (tid < n_levels) partial[tid * gridDim.x + blockIdx.x] = (red[tid][0] + red[tid][1]) + (red[tid][2] + red[tid][3]);
}

// One thread per prediction pixel, blockIdx.y = level: FlowMseLossV2 with area factors the tile path does not take (a
// loop over the sh x sw block), and the bilinear losses (the 4 ground-truth corners of the half-pixel sample point:
// tf.image.resize = F.interpolate(align_corners=False), no antialias).
template <int KIND, int LAYOUT>
__global__ __launch_bounds__(kLossThreads) void loss_pixel_kernel(const float* __restrict__ gt, LossLevels lv, int B,
                                                                  int H, int W, int C, float p0, float p1,
                                                                  float* __restrict__ partial) {
    __shared__ float red[kLossThreads / 64];
    const int l = blockIdx.y;
    const int h = lv.h[l], w = lv.w[l];
    const int64_t plane = (int64_t)h * w, n = (int64_t)B * plane;
    const int64_t gcs = chan_stride<LAYOUT>(H, W);
    float acc = 0.0f;
    for (int64_t i = (int64_t)blockIdx.x * kLossThreads + threadIdx.x; i < n; i += (int64_t)gridDim.x * kLossThreads) {
        const int64_t b = i / plane;
        const int r = (int)(i - b * plane);
        const int y = r / w, x = r - y * w;
        if (KIND == QPWC_LOSS_FLOW_MSE_V2) {
            const int sh = lv.sh[l], sw = lv.sw[l];
            // each row's sum first, then the rows: one running sum over all sh * sw terms put a 32 x 32 mean ~1e-6 of
            // the level's largest value off (the tile path's 2 x 2 steps: ~1e-7)
            float sx = 0.0f, sy = 0.0f;
            for (int yy = 0; yy < sh; ++yy) {
                const int64_t o = pix_offset<LAYOUT>(b, y * sh + yy, x * sw, H, W, 2);
                float rx = 0.0f, ry = 0.0f;
                for (int xx = 0; xx < sw; ++xx) {
                    const int64_t oo = o + (LAYOUT == QPWC_NHWC ? 2 * xx : xx);
                    rx += gt[oo];
                    ry += gt[oo + gcs];
                }
                sx += rx;
                sy += ry;
            }
            acc += flow_pixel<KIND, LAYOUT>(lv, l, b, y, x, (sx * lv.inv_area[l]) * lv.fscale[l],
                                            (sy * lv.inv_area[l]) * lv.fscale[l], p0, p1,
                                            ld_pred_pixel<LAYOUT>(lv, l, b, y, x));
        } else {
            // area_pixel_compute_source_index (align_corners = false): src = scale * (dst + 0.5) - 0.5, 0 below 0
            const float fy = fmaxf(lv.ry_scale[l] * ((float)y + 0.5f) - 0.5f, 0.0f);
            const float fx = fmaxf(lv.rx_scale[l] * ((float)x + 0.5f) - 0.5f, 0.0f);
            const int y0 = (int)fy, x0 = (int)fx;
            const int y1 = y0 + (y0 < H - 1 ? 1 : 0), x1 = x0 + (x0 < W - 1 ? 1 : 0);
            const float ly1 = fy - (float)y0, lx1 = fx - (float)x0;
            const float ly0 = 1.0f - ly1, lx0 = 1.0f - lx1;
            const int cc = KIND == QPWC_LOSS_AUTORESIZE_MSE ? C : 2;
            const int64_t o00 = pix_offset<LAYOUT>(b, y0, x0, H, W, cc), o01 = pix_offset<LAYOUT>(b, y0, x1, H, W, cc);
            const int64_t o10 = pix_offset<LAYOUT>(b, y1, x0, H, W, cc), o11 = pix_offset<LAYOUT>(b, y1, x1, H, W, cc);
            auto sample = [&](int c) -> float {
                const int64_t k = c * gcs;
                return ly0 * (lx0 * gt[o00 + k] + lx1 * gt[o01 + k]) + ly1 * (lx0 * gt[o10 + k] + lx1 * gt[o11 + k]);
            };
            if (KIND == QPWC_LOSS_AUTORESIZE_MSE) {
                const int64_t o = pix_offset<LAYOUT>(b, y, x, h, w, C), cs = chan_stride<LAYOUT>(h, w);
                for (int c = 0; c < C; ++c) {
                    const float g = sample(c);
                    const float e = ld_pred(lv.pred[l], o + c * cs, lv.f16[l]) - g;
                    acc += e * e;
                    if (float* d = lv.dpred[l]) d[o + c * cs] = (2.0f * e) * lv.inv_n[l];
                    if (float* go = lv.gt_out[l]) go[o + c * cs] = g;
                }
            } else {
                acc += flow_pixel<KIND, LAYOUT>(lv, l, b, y, x, sample(0) * lv.fscale[l], sample(1) * lv.fscale[l], p0,
                                                p1, ld_pred_pixel<LAYOUT>(lv, l, b, y, x));
            }
        }
    }
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    acc = loss_wave_sum(acc);
    if (lane == 0) red[wid] = acc;
    __syncthreads();
    if (threadIdx.x == 0) partial[l * gridDim.x + blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
}

// out[l] = inv_n[l] * (the nblk partial sums of level l, folded in a fixed order)
__global__ __launch_bounds__(kLossThreads) void loss_final_kernel(const float* __restrict__ partial, int nblk,
                                                                  LossLevels lv, float* __restrict__ out) {
    __shared__ float red[kLossThreads / 64];
    const int l = blockIdx.x;
    float s = 0.0f;
    for (int i = threadIdx.x; i < nblk; i += kLossThreads) s += partial[l * nblk + i];
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    s = loss_wave_sum(s);
    if (lane == 0) red[wid] = s;
    __syncthreads();
    if (threadIdx.x == 0) out[l] = ((red[0] + red[1]) + (red[2] + red[3])) * lv.inv_n[l];
}

struct LossGrads {
    const float* d[kLossMaxLevels];
    void* g[kLossMaxLevels];
    int64_t n[kLossMaxLevels];
    int f16[kLossMaxLevels];
    int vec[kLossMaxLevels];   // n % 4 == 0, d 16-byte and g 16-byte (fp32) / 8-byte (fp16) aligned
};

// grad_pred[l] = grad_losses[l] * dpred[l] for every level in one launch (blockIdx.y = level)
__global__ __launch_bounds__(kLossThreads) void loss_bwd_kernel(LossGrads lg, const float* __restrict__ grad_losses) {
    const int l = blockIdx.y;
    const float s = grad_losses[l];
    const float* d = lg.d[l];
    const int64_t n = lg.n[l];
    const int64_t tid = (int64_t)blockIdx.x * kLossThreads + threadIdx.x, nthr = (int64_t)gridDim.x * kLossThreads;
    if (lg.vec[l]) {
        const loss_f32x4* d4 = reinterpret_cast<const loss_f32x4*>(d);
        for (int64_t i = tid; i < n / 4; i += nthr) {
            const loss_f32x4 v = __builtin_nontemporal_load(d4 + i);
            const float4 r = make_float4(s * v.x, s * v.y, s * v.z, s * v.w);
            if (lg.f16[l]) st4(reinterpret_cast<__half*>(lg.g[l]) + 4 * i, r);
            else st4(reinterpret_cast<float*>(lg.g[l]) + 4 * i, r);
        }
        return;
    }
    for (int64_t i = tid; i < n; i += nthr) {
        if (lg.f16[l]) st(reinterpret_cast<__half*>(lg.g[l]) + i, s * d[i]);
        else st(reinterpret_cast<float*>(lg.g[l]) + i, s * d[i]);
    }
}

// ---- host side ------------------------------------------------------------------------------------------------------

int64_t loss_workspace_floats(int n_levels) { return (int64_t)n_levels * kLossTileBlocks; }

// Which forward kernel loss_fwd_launch takes for these arguments (host only).
const char* loss_fwd_kernel(int kind, int H, int W, const int* h, const int* w, int n, const void* gt) {
    LossLevels lv = {};
    if (kind == QPWC_LOSS_FLOW_MSE_V2 && (uintptr_t)gt % 16 == 0 && loss_tile_plan<kLossTile>(H, W, h, w, n, lv))
        return "loss_area_tile_kernel";
    return "loss_pixel_kernel";
}

int loss_fwd_launch(int kind, float p0, float p1, const float* gt, int B, int H, int W, int C, int layout,
                    const void* const* pred, const int* h, const int* w, const int* pred_dtype, int n, float* out,
                    void* const* dpred, void* const* gt_out, float* ws, hipStream_t s) {
    LossLevels lv = {};
    // Huber and MSE: the mean over the last axis, then SUM_OVER_BATCH_SIZE -- for dense tensors the mean over every
    // element in both layouts; the two norm losses: the mean over pixels
    const bool per_element = kind == QPWC_LOSS_FLOW_MSE_V2 || kind == QPWC_LOSS_AUTORESIZE_MSE;
    for (int i = 0; i < n; ++i) {
        lv.pred[i] = pred[i];
        lv.dpred[i] = dpred ? (float*)dpred[i] : nullptr;
        lv.gt_out[i] = gt_out ? (float*)gt_out[i] : nullptr;
        lv.h[i] = h[i];
        lv.w[i] = w[i];
        lv.sh[i] = H / h[i];
        lv.sw[i] = W / w[i];
        lv.f16[i] = pred_dtype[i] == QPWC_F16;
        // h / H in fp32, as the reference's tf.cast(h) / tf.cast(H); AutoResizeMseLoss has no flow scale
        lv.fscale[i] = kind == QPWC_LOSS_AUTORESIZE_MSE ? 1.0f : (float)h[i] / (float)H;
        lv.inv_area[i] = lv.sh[i] > 0 && lv.sw[i] > 0 ? 1.0f / (float)(lv.sh[i] * lv.sw[i]) : 0.0f;
        const double pix = (double)B * h[i] * w[i];
        lv.inv_n[i] = (float)(1.0 / (per_element ? pix * C : pix));
        lv.lscale[i] = (float)(2.0 / ((double)w[i] + (double)h[i]));
        lv.ry_scale[i] = (float)H / (float)h[i];
        lv.rx_scale[i] = (float)W / (float)w[i];
    }
    int nblk;
    if (kind == QPWC_LOSS_FLOW_MSE_V2 && (uintptr_t)gt % 16 == 0 && loss_tile_plan<kLossTile>(H, W, h, w, n, lv)) {
        const int64_t ntiles = (int64_t)B * (H / kLossTile) * (W / kLossTile);
        nblk = (int)(ntiles < kLossTileBlocks ? ntiles : kLossTileBlocks);
        if (layout == QPWC_NHWC)
            hipLaunchKernelGGL((loss_area_tile_kernel<QPWC_NHWC>), dim3(nblk), dim3(kLossThreads), 0, s, gt, lv, n, B, H,
                               W, p0, ws);
        else
            hipLaunchKernelGGL((loss_area_tile_kernel<QPWC_NCHW>), dim3(nblk), dim3(kLossThreads), 0, s, gt, lv, n, B, H,
                               W, p0, ws);
        const int rc = check_launch("loss_area_tile_kernel");
        if (rc != QPWC_OK) return rc;
    } else {
        nblk = kLossPixBlocks;
        const dim3 grid(kLossPixBlocks, n);
#define QPWC_LOSS_PIX(K)                                                                                              \
    do {                                                                                                              \
        if (layout == QPWC_NHWC)                                                                                      \
            hipLaunchKernelGGL((loss_pixel_kernel<K, QPWC_NHWC>), grid, dim3(kLossThreads), 0, s, gt, lv, B, H, W, C, \
                               p0, p1, ws);                                                                           \
        else                                                                                                          \
            hipLaunchKernelGGL((loss_pixel_kernel<K, QPWC_NCHW>), grid, dim3(kLossThreads), 0, s, gt, lv, B, H, W, C, \
                               p0, p1, ws);                                                                           \
    } while (0)
        switch (kind) {
            case QPWC_LOSS_FLOW_MSE_V2: QPWC_LOSS_PIX(QPWC_LOSS_FLOW_MSE_V2); break;
            case QPWC_LOSS_FLOW_MSE: QPWC_LOSS_PIX(QPWC_LOSS_FLOW_MSE); break;
            case QPWC_LOSS_FLOW_FINETUNE: QPWC_LOSS_PIX(QPWC_LOSS_FLOW_FINETUNE); break;
            default: QPWC_LOSS_PIX(QPWC_LOSS_AUTORESIZE_MSE); break;
        }
#undef QPWC_LOSS_PIX
        const int rc = check_launch("loss_pixel_kernel");
        if (rc != QPWC_OK) return rc;
    }
    hipLaunchKernelGGL(loss_final_kernel, dim3(n), dim3(kLossThreads), 0, s, ws, nblk, lv, out);
    return check_launch("loss_final_kernel");
}

int loss_bwd_launch(const void* const* dpred, const float* grad_losses, void* const* grad_pred, const int64_t* n_elems,
                    const int* pred_dtype, int n, hipStream_t s) {
    LossGrads lg = {};
    for (int i = 0; i < n; ++i) {
        lg.d[i] = (const float*)dpred[i];
        lg.g[i] = grad_pred[i];
        lg.n[i] = n_elems[i];
        lg.f16[i] = pred_dtype[i] == QPWC_F16;
        lg.vec[i] = n_elems[i] % 4 == 0 && (uintptr_t)dpred[i] % 16 == 0 &&
                    (uintptr_t)grad_pred[i] % (lg.f16[i] ? 8 : 16) == 0;
    }
    hipLaunchKernelGGL(loss_bwd_kernel, dim3(kLossBwdBlocks, n), dim3(kLossThreads), 0, s, lg, grad_losses);
    return check_launch("loss_bwd_kernel");
}

}  // namespace qpwc

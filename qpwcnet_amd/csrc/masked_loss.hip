// The three flow losses over the valid pixels only (include/qpwc_masked_loss.h): the masked twins of loss.hip's
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
#include "common.h"
#include "launch.h"
#include "loss_common.h"

namespace qpwc {

constexpr int kMaskedThreads = 256;
constexpr int kMaskedTile = 32;           // tile path: 32 x 32 ground-truth pixels per tile, as loss.hip
constexpr int kMaskedPixBlocks = 1024;    // pixel path: workgroups per level
constexpr int kMaskedTileBlocks = 2048;   // tile path: at most this many workgroups, each walks its tiles
constexpr int kMaskedBwdBlocks = 1024;
constexpr float kFlowUnknown = 1e9f;      // |component| above it: unknown (the .flo convention); NaN and Inf fail it too

struct MaskedLevels {
    const void* pred[kLossMaxLevels];          // NULL: taken as zero (gt_out / valid_out only)
    float* dpred[kLossMaxLevels];              // NULL: not written
    float* gt_out[kLossMaxLevels];             // NULL: not written
    unsigned char* valid_out[kLossMaxLevels];  // NULL: not written
    int h[kLossMaxLevels], w[kLossMaxLevels];
    int sh[kLossMaxLevels], sw[kLossMaxLevels];   // area factors H / h, W / w
    int f16[kLossMaxLevels];
    float fscale[kLossMaxLevels];              // flow scale h / H on both channels
    float lscale[kLossMaxLevels];              // FlowMseLossV2: 2 / (w + h)
    float ry_scale[kLossMaxLevels], rx_scale[kLossMaxLevels];   // bilinear: (float)H / h, (float)W / w
    int nsteps;                                // tile path: as LossLevels
    int step_ry[kLossMaxSteps], step_rx[kLossMaxSteps], step_level[kLossMaxSteps];
};

namespace {

__device__ __forceinline__ int masked_wave_sum(int v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
    return v;
}

// false for NaN and +-Inf as well
__device__ __forceinline__ bool flow_known(float x, float y) { return fabsf(x) <= kFlowUnknown && fabsf(y) <= kFlowUnknown; }

// area_pixel_compute_source_index (align_corners = false): src = scale * (dst + 0.5) - 0.5, 0 below 0.  The product and
// the difference are rounded one by one (no fused multiply-add), so that the point is the one loss.py's fp32 chain forms:
// where only corners of small weight are valid, the renormalisation by S magnifies an ulp of the point a hundredfold.
__device__ __forceinline__ float masked_sample_point(float scale, int o) {
#pragma clang fp contract(off)
    const float p = scale * ((float)o + 0.5f);
    return fmaxf(p - 0.5f, 0.0f);
}

template <int LAYOUT>
__device__ __forceinline__ float2 masked_ld_pred_pixel(const MaskedLevels& lv, int l, int64_t b, int y, int x) {
    const int64_t o = pix_offset<LAYOUT>(b, y, x, lv.h[l], lv.w[l], 2), cs = chan_stride<LAYOUT>(lv.h[l], lv.w[l]);
    return make_float2(ld_pred(lv.pred[l], o, lv.f16[l]), ld_pred(lv.pred[l], o + cs, lv.f16[l]));
}

// One level pixel: m its validity, (gx, gy) its ground truth (used only where m), pv the prediction (may hold anything
// where !m).  Returns the term, 0 where !m; stores the derivative, the ground truth and the validity where asked.
template <int KIND, int LAYOUT>
__device__ __forceinline__ float masked_flow_pixel(const MaskedLevels& lv, int l, int64_t b, int y, int x, bool m,
                                                   float gx, float gy, float p0, float p1, float2 pv) {
    const int h = lv.h[l], w = lv.w[l];
    const int64_t o = pix_offset<LAYOUT>(b, y, x, h, w, 2), cs = chan_stride<LAYOUT>(h, w);
    gx = m ? gx : 0.0f;
    gy = m ? gy : 0.0f;
    float dx, dy;
    float t = flow_term<KIND>(gx, gy, m ? pv.x : 0.0f, m ? pv.y : 0.0f, lv.lscale[l], p0, p1, dx, dy);
    t = m ? t : 0.0f;
    if (float* d = lv.dpred[l]) {
        d[o] = m ? dx : 0.0f;
        d[o + cs] = m ? dy : 0.0f;
    }
    if (float* g = lv.gt_out[l]) {
        g[o] = gx;
        g[o + cs] = gy;
    }
    if (unsigned char* v = lv.valid_out[l]) v[(b * h + y) * (int64_t)w + x] = m ? 1 : 0;
    return t;
}

}  // namespace

// FlowMseLossV2 of every level from one read of the ground truth and the mask: as loss_area_tile_kernel, a workgroup owns
// 32x32 GT pixels at a time (two 16-byte loads of the flow and 4 mask bytes per thread; the next tile's loads are in
// flight while this one is reduced) and carries a sum pyramid of (sum v x, sum v y) and sum v per cell through the 2x2
// steps.  sum v <= 1024 is exact in fp32; a level pixel is valid iff it is >= 1.
template <int LAYOUT>
__global__ __launch_bounds__(kMaskedThreads) void masked_loss_tile_kernel(const float* __restrict__ gt,
                                                                        const unsigned char* __restrict__ valid,
                                                                        MaskedLevels lv, int n_levels, int B, int H,
                                                                        int W, float delta, float* __restrict__ psum,
                                                                        int* __restrict__ pcnt) {
    __shared__ float2 raw[kMaskedTile * kMaskedTile];            // (y, x) -> (sum v x, sum v y): 8 KB
    __shared__ float rawn[kMaskedTile * kMaskedTile];            // (y, x) -> sum v: 4 KB
    __shared__ float2 aux[kMaskedTile * kMaskedTile / 2];        // 4 KB
    __shared__ float auxn[kMaskedTile * kMaskedTile / 2];        // 2 KB
    __shared__ float red[kLossMaxLevels][kMaskedThreads / 64];
    __shared__ int redn[kLossMaxLevels][kMaskedThreads / 64];
    const int tid = threadIdx.x;
    const int tiles_x = W / kMaskedTile, tiles_y = H / kMaskedTile;
    const int ntiles = B * tiles_y * tiles_x;
    float acc[kLossMaxLevels];
    int cnt[kLossMaxLevels];
#pragma unroll
    for (int k = 0; k < kLossMaxLevels; ++k) {
        acc[k] = 0.0f;
        cnt[k] = 0;
    }

    // 512 float4 per tile, two per thread.  NHWC: float4 i = tid + 256 k is row i / 16, pixels 2 (i % 16) and the next;
    // NCHW: k is the channel, row tid / 8, pixels 4 (tid % 8) .. + 3 -- both channels of 4 pixels in one thread
    const loss_f32x4* g4 = reinterpret_cast<const loss_f32x4*>(gt);
    auto gt_index = [&](int tile, int i) -> int64_t {
        const int tx = tile % tiles_x, ty = (tile / tiles_x) % tiles_y, b = tile / (tiles_x * tiles_y);
        if (LAYOUT == QPWC_NHWC) {
            const int row = i >> 4, c4 = i & 15;
            return ((((int64_t)b * H + ty * kMaskedTile + row) * W + tx * kMaskedTile) * 2) / 4 + c4;
        }
        const int c = i >> 8, row = (i >> 3) & 31, c4 = i & 7;
        return ((((int64_t)b * 2 + c) * H + ty * kMaskedTile + row) * W + tx * kMaskedTile) / 4 + c4;
    };
    // the mask bytes of the pixels this thread holds: NHWC 2 bytes per k (a 2-byte load), NCHW 4 bytes (a 4-byte load)
    auto ld_mask = [&](int tile, unsigned* mk) {
        mk[0] = mk[1] = 0x01010101u;
        if (!valid) return;
        const int tx = tile % tiles_x, ty = (tile / tiles_x) % tiles_y, b = tile / (tiles_x * tiles_y);
        if (LAYOUT == QPWC_NHWC) {
#pragma unroll
            for (int k = 0; k < 2; ++k) {
                const int i = tid + k * kMaskedThreads, row = i >> 4, c4 = i & 15;
                const int64_t o = ((int64_t)b * H + ty * kMaskedTile + row) * W + tx * kMaskedTile + 2 * c4;
                mk[k] = __builtin_nontemporal_load(reinterpret_cast<const unsigned short*>(valid + o));
            }
        } else {
            const int row = tid >> 3, c4 = tid & 7;
            const int64_t o = ((int64_t)b * H + ty * kMaskedTile + row) * W + tx * kMaskedTile + 4 * c4;
            mk[0] = __builtin_nontemporal_load(reinterpret_cast<const unsigned*>(valid + o));
        }
    };
    loss_f32x4 v[2];
    unsigned mk[2];
    if ((int)blockIdx.x < ntiles) {
#pragma unroll
        for (int k = 0; k < 2; ++k) v[k] = __builtin_nontemporal_load(g4 + gt_index(blockIdx.x, tid + k * kMaskedThreads));
        ld_mask(blockIdx.x, mk);
    }
    for (int tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const int tx = tile % tiles_x, ty = (tile / tiles_x) % tiles_y, b = tile / (tiles_x * tiles_y);
        // this thread's prediction pixel of every level of the tile, all loads issued up front (as the dense kernel)
        float2 pv[kLossMaxSteps];
        {
            int fy = 1, fx = 1;
#pragma unroll
            for (int s = 0; s < kLossMaxSteps; ++s) {
                pv[s] = make_float2(0.0f, 0.0f);
                if (s < lv.nsteps) {
                    fy *= lv.step_ry[s];
                    fx *= lv.step_rx[s];
                    const int l = lv.step_level[s], nx = kMaskedTile / fx;
                    if (l >= 0 && tid < (kMaskedTile / fy) * nx)
                        pv[s] = masked_ld_pred_pixel<LAYOUT>(lv, l, b, ty * (kMaskedTile / fy) + tid / nx,
                                                             tx * nx + tid % nx);
                }
            }
        }
        __syncthreads();                                   // the previous tile's steps are done with raw / aux
        auto put = [&](int cell, float x, float y, unsigned mbyte) {
            const bool ok = mbyte != 0 && flow_known(x, y);
            raw[cell] = make_float2(ok ? x : 0.0f, ok ? y : 0.0f);
            rawn[cell] = ok ? 1.0f : 0.0f;
        };
        if (LAYOUT == QPWC_NHWC) {
#pragma unroll
            for (int k = 0; k < 2; ++k) {
                const int cell = 2 * (tid + k * kMaskedThreads);
                put(cell, v[k].x, v[k].y, mk[k] & 0xffu);
                put(cell + 1, v[k].z, v[k].w, (mk[k] >> 8) & 0xffu);
            }
        } else {
            const int cell = (tid >> 3) * kMaskedTile + (tid & 7) * 4;
            put(cell, v[0].x, v[1].x, mk[0] & 0xffu);
            put(cell + 1, v[0].y, v[1].y, (mk[0] >> 8) & 0xffu);
            put(cell + 2, v[0].z, v[1].z, (mk[0] >> 16) & 0xffu);
            put(cell + 3, v[0].w, v[1].w, mk[0] >> 24);
        }
        const int next = tile + gridDim.x;
        if (next < ntiles) {
#pragma unroll
            for (int k = 0; k < 2; ++k) v[k] = __builtin_nontemporal_load(g4 + gt_index(next, tid + k * kMaskedThreads));
            ld_mask(next, mk);
        }
        __syncthreads();
        int fy = 1, fx = 1;
#pragma unroll
        for (int s = 0; s < kLossMaxSteps; ++s) {
            if (s >= lv.nsteps) continue;
            const int ry = lv.step_ry[s], rx = lv.step_rx[s], l = lv.step_level[s];
            const float2* src = (s & 1) ? aux : raw;
            const float* srcn = (s & 1) ? auxn : rawn;
            float2* dst = (s & 1) ? raw : aux;
            float* dstn = (s & 1) ? rawn : auxn;
            const int pnx = kMaskedTile / fx;
            fy *= ry;
            fx *= rx;
            const int ny = kMaskedTile / fy, nx = kMaskedTile / fx;
            for (int o = tid; o < ny * nx; o += kMaskedThreads) {
                const int oy = o / nx, ox = o - oy * nx;
                const int pi = (oy * ry) * pnx + ox * rx;
                float2 sum = src[pi];
                float n = srcn[pi];
                if (rx == 2) {
                    sum = f2add(sum, src[pi + 1]);
                    n += srcn[pi + 1];
                }
                if (ry == 2) {
                    float2 q = src[pi + pnx];
                    float qn = srcn[pi + pnx];
                    if (rx == 2) {
                        q = f2add(q, src[pi + pnx + 1]);
                        qn += srcn[pi + pnx + 1];
                    }
                    sum = f2add(sum, q);
                    n += qn;
                }
                dst[o] = sum;
                dstn[o] = n;
                if (l >= 0) {
                    const bool m = n >= 1.0f;
                    // the mean over the block's valid pixels times h / H with one division: for a full block (n a power
                    // of two) h / H / n is exact and the product is the dense kernel's (sum * inv_area) * fscale, bit for bit
                    const float r = lv.fscale[l] / (m ? n : 1.0f);
                    const float t = masked_flow_pixel<QPWC_LOSS_FLOW_MSE_V2, LAYOUT>(
                        lv, l, b, ty * ny + oy, tx * nx + ox, m, sum.x * r, sum.y * r, delta, 0.0f, pv[s]);
#pragma unroll
                    for (int k = 0; k < kLossMaxLevels; ++k) {   // no dynamic register index
                        acc[k] += k == l ? t : 0.0f;
                        cnt[k] += (k == l && m) ? 1 : 0;
                    }
                }
            }
            __syncthreads();
        }
    }
    const int lane = tid & 63, wid = tid >> 6;
#pragma unroll
    for (int k = 0; k < kLossMaxLevels; ++k) {
        const float s = loss_wave_sum(acc[k]);
        const int c = masked_wave_sum(cnt[k]);
        if (lane == 0) {
            red[k][wid] = s;
            redn[k][wid] = c;
        }
    }
    __syncthreads();
    if (tid < n_levels) {
        psum[tid * gridDim.x + blockIdx.x] = (red[tid][0] + red[tid][1]) + (red[tid][2] + red[tid][3]);
        pcnt[tid * gridDim.x + blockIdx.x] = (redn[tid][0] + redn[tid][1]) + (redn[tid][2] + redn[tid][3]);
    }
}

// One thread per level pixel, blockIdx.y = level: FlowMseLossV2 with area factors the tile path does not take (a loop
// over the sh x sw block) and the bilinear losses (the 4 ground-truth corners of the half-pixel sample point, their
// weights renormalised over the valid ones).
template <int KIND, int LAYOUT>
__global__ __launch_bounds__(kMaskedThreads) void masked_loss_pixel_kernel(const float* __restrict__ gt,
                                                                         const unsigned char* __restrict__ valid,
                                                                         MaskedLevels lv, int B, int H, int W, float p0,
                                                                         float p1, float* __restrict__ psum,
                                                                         int* __restrict__ pcnt) {
    __shared__ float red[kMaskedThreads / 64];
    __shared__ int redn[kMaskedThreads / 64];
    const int l = blockIdx.y;
    const int h = lv.h[l], w = lv.w[l];
    const int64_t plane = (int64_t)h * w, n = (int64_t)B * plane;
    const int64_t gcs = chan_stride<LAYOUT>(H, W);
    float acc = 0.0f;
    int cnt = 0;   // a workgroup sees n / kMaskedPixBlocks pixels: below 2^31 for every tensor that fits a device
    // the ground truth of pixel (b, y, x) where it is valid: ok, and (gx, gy) only then
    auto known = [&](int64_t b, int y, int x, float& gx, float& gy) -> bool {
        if (valid && valid[(b * H + y) * (int64_t)W + x] == 0) return false;
        const int64_t o = pix_offset<LAYOUT>(b, y, x, H, W, 2);
        gx = gt[o];
        gy = gt[o + gcs];
        return flow_known(gx, gy);
    };
    for (int64_t i = (int64_t)blockIdx.x * kMaskedThreads + threadIdx.x; i < n; i += (int64_t)gridDim.x * kMaskedThreads) {
        const int64_t b = i / plane;
        const int r = (int)(i - b * plane);
        const int y = r / w, x = r - y * w;
        float sx = 0.0f, sy = 0.0f, sn = 0.0f;
        if (KIND == QPWC_LOSS_FLOW_MSE_V2) {
            const int sh = lv.sh[l], sw = lv.sw[l];
            // each row's sum first, then the rows, as the dense kernel; the valid pixels are counted as an integer
            int nv = 0;
            for (int yy = 0; yy < sh; ++yy) {
                float rx = 0.0f, ry = 0.0f;
                for (int xx = 0; xx < sw; ++xx) {
                    float gx, gy;
                    const bool ok = known(b, y * sh + yy, x * sw + xx, gx, gy);
                    rx += ok ? gx : 0.0f;
                    ry += ok ? gy : 0.0f;
                    nv += ok ? 1 : 0;
                }
                sx += rx;
                sy += ry;
            }
            sn = (float)nv;
        } else {
            // the four corners of the half-pixel sample point and their weights, as the dense kernel's
            const float fy = masked_sample_point(lv.ry_scale[l], y), fx = masked_sample_point(lv.rx_scale[l], x);
            const int y0 = min((int)fy, H - 1), x0 = min((int)fx, W - 1);   // fy < H, fx < W: the min never binds
            const int y1 = y0 + (y0 < H - 1 ? 1 : 0), x1 = x0 + (x0 < W - 1 ? 1 : 0);
            const float ly1 = fy - (float)y0, lx1 = fx - (float)x0;
            const float ly0 = 1.0f - ly1, lx0 = 1.0f - lx1;
            const int cy[4] = {y0, y0, y1, y1}, cx[4] = {x0, x1, x0, x1};
            const float cw[4] = {ly0 * lx0, ly0 * lx1, ly1 * lx0, ly1 * lx1};
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                float gx, gy;
                const bool ok = known(b, cy[k], cx[k], gx, gy);
                sx += ok ? cw[k] * gx : 0.0f;
                sy += ok ? cw[k] * gy : 0.0f;
                sn += ok ? cw[k] : 0.0f;
            }
        }
        const bool m = KIND == QPWC_LOSS_FLOW_MSE_V2 ? sn >= 1.0f : sn > 0.0f;
        const float dn = m ? sn : 1.0f;
        acc += masked_flow_pixel<KIND, LAYOUT>(lv, l, b, y, x, m, (sx / dn) * lv.fscale[l], (sy / dn) * lv.fscale[l], p0,
                                               p1, masked_ld_pred_pixel<LAYOUT>(lv, l, b, y, x));
        cnt += m ? 1 : 0;
    }
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    acc = loss_wave_sum(acc);
    cnt = masked_wave_sum(cnt);
    if (lane == 0) {
        red[wid] = acc;
        redn[wid] = cnt;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        psum[l * gridDim.x + blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
        pcnt[l * gridDim.x + blockIdx.x] = (redn[0] + redn[1]) + (redn[2] + redn[3]);
    }
}

// the number of averaged terms of a level with `count` valid pixels: max(count, 1), per element for the Huber kind
__device__ __forceinline__ double masked_denominator(int64_t count, int per_element) {
    return (double)(count > 0 ? count : 1) * (per_element ? 2.0 : 1.0);
}

// counts[l] = the nblk partial counts of level l; out[l] = (its nblk partial sums, folded in a fixed order) / denominator
__global__ __launch_bounds__(kMaskedThreads) void masked_loss_fold_kernel(const float* __restrict__ psum,
                                                                        const int* __restrict__ pcnt, int nblk,
                                                                        int per_element, float* __restrict__ out,
                                                                        int64_t* __restrict__ counts) {
    __shared__ float red[kMaskedThreads / 64];
    __shared__ long long redn[kMaskedThreads / 64];
    const int l = blockIdx.x;
    float s = 0.0f;
    long long c = 0;
    for (int i = threadIdx.x; i < nblk; i += kMaskedThreads) {
        s += psum[l * nblk + i];
        c += pcnt[l * nblk + i];
    }
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    s = loss_wave_sum(s);
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) c += __shfl_down(c, off, 64);
    if (lane == 0) {
        red[wid] = s;
        redn[wid] = c;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        const int64_t count = (redn[0] + redn[1]) + (redn[2] + redn[3]);
        const float sum = (red[0] + red[1]) + (red[2] + red[3]);
        counts[l] = count;
        out[l] = (float)((double)sum / masked_denominator(count, per_element));
    }
}

struct MaskedGrads {
    const float* d[kLossMaxLevels];
    void* g[kLossMaxLevels];
    int64_t n[kLossMaxLevels];
    int f16[kLossMaxLevels];
};

// grad_pred[l] = (grad_losses[l] / denominator(counts[l])) * dpred[l] for every level in one launch (blockIdx.y = level);
// 16 bytes of dpred per thread where the level's element count is a multiple of 4 (the boundary holds both on the grid)
__global__ __launch_bounds__(kMaskedThreads) void masked_loss_bwd_kernel(MaskedGrads lg, const int64_t* __restrict__ counts,
                                                                       int per_element,
                                                                       const float* __restrict__ grad_losses) {
    const int l = blockIdx.y;
    const float s = (float)((double)grad_losses[l] / masked_denominator(counts[l], per_element));
    const float* d = lg.d[l];
    const int64_t n = lg.n[l];
    const int64_t tid = (int64_t)blockIdx.x * kMaskedThreads + threadIdx.x, nthr = (int64_t)gridDim.x * kMaskedThreads;
    if (n % 4 == 0) {
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

// floats: n_levels * kMaskedTileBlocks partial sums, then as many 32-bit partial counts
int64_t masked_loss_workspace_floats(int n_levels) { return (int64_t)n_levels * kMaskedTileBlocks * 2; }

// Which forward kernel masked_loss_fwd_launch takes for these arguments (host only).
const char* masked_loss_fwd_kernel(int kind, int H, int W, const int* h, const int* w, int n) {
    MaskedLevels lv = {};
    if (kind == QPWC_LOSS_FLOW_MSE_V2 && loss_tile_plan<kMaskedTile>(H, W, h, w, n, lv)) return "masked_loss_tile_kernel";
    return "masked_loss_pixel_kernel";
}

int masked_loss_fwd_launch(int kind, float p0, float p1, const float* gt, const unsigned char* valid, int B, int H, int W,
                           int layout, const void* const* pred, const int* h, const int* w, const int* pred_dtype, int n,
                           float* out, int64_t* counts, void* const* dpred, void* const* gt_out, void* const* valid_out,
                           float* ws, hipStream_t s) {
    MaskedLevels lv = {};
    for (int i = 0; i < n; ++i) {
        lv.pred[i] = pred[i];
        lv.dpred[i] = dpred ? (float*)dpred[i] : nullptr;
        lv.gt_out[i] = gt_out ? (float*)gt_out[i] : nullptr;
        lv.valid_out[i] = valid_out ? (unsigned char*)valid_out[i] : nullptr;
        lv.h[i] = h[i];
        lv.w[i] = w[i];
        lv.sh[i] = H / h[i];
        lv.sw[i] = W / w[i];
        lv.f16[i] = pred_dtype[i] == QPWC_F16;
        lv.fscale[i] = (float)h[i] / (float)H;              // as loss_fwd_launch
        lv.lscale[i] = (float)(2.0 / ((double)w[i] + (double)h[i]));
        lv.ry_scale[i] = (float)H / (float)h[i];
        lv.rx_scale[i] = (float)W / (float)w[i];
    }
    const bool tile = kind == QPWC_LOSS_FLOW_MSE_V2 && loss_tile_plan<kMaskedTile>(H, W, h, w, n, lv);
    int nblk;
    if (tile) {
        const int64_t ntiles = (int64_t)B * (H / kMaskedTile) * (W / kMaskedTile);
        nblk = (int)(ntiles < kMaskedTileBlocks ? ntiles : kMaskedTileBlocks);
    } else {
        nblk = kMaskedPixBlocks;
    }
    float* psum = ws;
    int* pcnt = reinterpret_cast<int*>(ws + (int64_t)n * nblk);
    if (tile) {
        if (layout == QPWC_NHWC)
            hipLaunchKernelGGL((masked_loss_tile_kernel<QPWC_NHWC>), dim3(nblk), dim3(kMaskedThreads), 0, s, gt, valid, lv,
                               n, B, H, W, p0, psum, pcnt);
        else
            hipLaunchKernelGGL((masked_loss_tile_kernel<QPWC_NCHW>), dim3(nblk), dim3(kMaskedThreads), 0, s, gt, valid, lv,
                               n, B, H, W, p0, psum, pcnt);
        const int rc = check_launch("masked_loss_tile_kernel");
        if (rc != QPWC_OK) return rc;
    } else {
        const dim3 grid(kMaskedPixBlocks, n);
#define QPWC_MASKED_PIX(K)                                                                                         \
    do {                                                                                                           \
        if (layout == QPWC_NHWC)                                                                                   \
            hipLaunchKernelGGL((masked_loss_pixel_kernel<K, QPWC_NHWC>), grid, dim3(kMaskedThreads), 0, s, gt, valid, \
                               lv, B, H, W, p0, p1, psum, pcnt);                                                   \
        else                                                                                                       \
            hipLaunchKernelGGL((masked_loss_pixel_kernel<K, QPWC_NCHW>), grid, dim3(kMaskedThreads), 0, s, gt, valid, \
                               lv, B, H, W, p0, p1, psum, pcnt);                                                   \
    } while (0)
        switch (kind) {
            case QPWC_LOSS_FLOW_MSE_V2: QPWC_MASKED_PIX(QPWC_LOSS_FLOW_MSE_V2); break;
            case QPWC_LOSS_FLOW_MSE: QPWC_MASKED_PIX(QPWC_LOSS_FLOW_MSE); break;
            default: QPWC_MASKED_PIX(QPWC_LOSS_FLOW_FINETUNE); break;
        }
#undef QPWC_MASKED_PIX
        const int rc = check_launch("masked_loss_pixel_kernel");
        if (rc != QPWC_OK) return rc;
    }
    hipLaunchKernelGGL(masked_loss_fold_kernel, dim3(n), dim3(kMaskedThreads), 0, s, psum, pcnt, nblk,
                       kind == QPWC_LOSS_FLOW_MSE_V2 ? 1 : 0, out, counts);
    return check_launch("masked_loss_fold_kernel");
}

int masked_loss_bwd_launch(int kind, const void* const* dpred, const int64_t* counts, const float* grad_losses,
                           void* const* grad_pred, const int64_t* n_elems, const int* pred_dtype, int n, hipStream_t s) {
    MaskedGrads lg = {};
    for (int i = 0; i < n; ++i) {
        lg.d[i] = (const float*)dpred[i];
        lg.g[i] = grad_pred[i];
        lg.n[i] = n_elems[i];
        lg.f16[i] = pred_dtype[i] == QPWC_F16;
    }
    hipLaunchKernelGGL(masked_loss_bwd_kernel, dim3(kMaskedBwdBlocks, n), dim3(kMaskedThreads), 0, s, lg, counts,
                       kind == QPWC_LOSS_FLOW_MSE_V2 ? 1 : 0, grad_losses);
    return check_launch("masked_loss_bwd_kernel");
}

}  // namespace qpwc

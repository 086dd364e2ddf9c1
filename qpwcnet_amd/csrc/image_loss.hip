// The frame interpolator's structural loss (include/qpwc_image_loss.h): per level ssim_weight * (1 - SSIM) / 2 plus
// (1 - ssim_weight) * Charbonnier between a prediction and its target, SSIM with tf.image.ssim's default 11 x 11 window.
//   forward : one launch for all levels (image_loss_fwd_kernel), a workgroup per (level, image, tile of 16 x 32 pixels)
//             found through the per-level prefix table in the kernel arguments.  Per channel the 26 x 42 patch of vt and
//             vp whose origin is the tile's goes through LDS (zeros beyond the image); the Charbonnier terms of the tile's
//             own pixels are summed as they are staged; then the row pass of vt, vp, vt^2 + vp^2 and vt * vp into LDS, the
//             column pass from it, s and its three partial derivatives Pa, Pb, Pc, which go to the workspace for the
//             backward.  The workgroup writes its two partial sums; + one fixed-order fold (image_loss_fold_kernel).
//             LDS: 2 * 26 * 42 + 4 * 26 * 32 floats + the reduction = 21.6 KB, static.
//   backward: one launch on the same grid (image_loss_bwd_kernel): a gather.  The transposed window pass over a plane P is
//             the same pair of 11-tap passes over P's patch whose origin is the tile's origin - 10, zero outside the
//             positions, with the taps reversed; the three results combine with vp, vt and the Charbonnier derivative.
//             LDS: 3 * 26 * 42 + 3 * 26 * 32 floats = 23.1 KB, static.
// Deterministic: grids depend on the shapes only, fixed-order sums, no atomics.  Every global access is element-wise: no
// form depends on an address.  quality.hip keeps its own window pass: sharing it is a later change.
#include <math.h>

#include "../../include/qpwc_image_loss.h"
#include "common.h"
#include "launch.h"

// s and its derivatives are separately rounded products and sums, as include/qpwc_image_loss.h states them; the
// convolutions name their fmaf
#pragma clang fp contract(off)

namespace qpwc {

constexpr int kImgThreads = 256;
constexpr int kImgTileH = 16, kImgTileW = 32;      // pixels per workgroup (_hip.IMAGE_LOSS_TILE)
constexpr int kImgTaps = 11, kImgRim = kImgTaps - 1;
constexpr int kImgWH = kImgTileH + kImgRim, kImgWW = kImgTileW + kImgRim;   // the patch: 26 x 42
constexpr int kImgMaps = 4;                        // vt, vp, vt^2 + vp^2, vt * vp
constexpr int kImgPlanes = 3;                      // saved per position: Pa, Pb, Pc
constexpr int kImgMaxLevels = 8;
constexpr int kImgWaves = kImgThreads / 64;

static_assert(kImgThreads == kImgTileW * (kImgTileH / 2), "the column pass gives every lane two rows of one column");

struct ImgLevels {
    const float* truth[kImgMaxLevels];
    const void* pred[kImgMaxLevels];
    void* grad[kImgMaxLevels];                   // backward: d loss / d pred
    float* planes[kImgMaxLevels];                // the level's 3 saved planes of B * C * (h - 10) * (w - 10) floats
    int h[kImgMaxLevels], w[kImgMaxLevels], f16[kImgMaxLevels];
    int tiles_x[kImgMaxLevels], tiles_y[kImgMaxLevels];
    int tile_start[kImgMaxLevels + 1];           // prefix sums of B * tiles_y * tiles_x
};

struct ImgParams {
    float g[kImgTaps];
    float c1, c2, offset, q, eps, ssim_weight;
};

namespace {

template <class T>
__device__ __forceinline__ T img_wave_sum(T v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
    return v;
}

// the workgroup's (level, image, tile origin)
struct ImgTile {
    int l, b, y0, x0;
};
__device__ __forceinline__ ImgTile img_tile(const ImgLevels& lv, int n_levels) {
    const int bid = blockIdx.x;
    ImgTile t;
    t.l = 0;
    for (int k = 1; k < n_levels; ++k)
        if (bid >= lv.tile_start[k]) t.l = k;
    int i = bid - lv.tile_start[t.l];
    const int tx = i % lv.tiles_x[t.l];
    i /= lv.tiles_x[t.l];
    t.y0 = (i % lv.tiles_y[t.l]) * kImgTileH;
    t.b = i / lv.tiles_y[t.l];
    t.x0 = tx * kImgTileW;
    return t;
}

// element (b, y, x, c) of a dense (B,h,w,C) / (B,C,h,w) tensor
template <int LAYOUT>
__device__ __forceinline__ int64_t img_offset(int64_t b, int c, int y, int x, int h, int w, int C) {
    return LAYOUT == QPWC_NHWC ? ((b * h + y) * w + x) * C + c : ((b * C + c) * h + y) * (int64_t)w + x;
}

__device__ __forceinline__ float img_ld_pred(const void* p, int f16, int64_t o) {
    if (f16) return __half2float(reinterpret_cast<const __half*>(p)[o]);
    return reinterpret_cast<const float*>(p)[o];
}

}  // namespace

// part[blockIdx.x * 2]: the tile's sum of s over its positions and channels, [.. + 1]: its sum of Charbonnier terms.
template <int LAYOUT>
__global__ __launch_bounds__(kImgThreads) void image_loss_fwd_kernel(ImgLevels lv, int n_levels, int B, int C, ImgParams pm,
                                                                   float* __restrict__ part) {
    __shared__ float st[kImgWH][kImgWW];
    __shared__ float sp[kImgWH][kImgWW];
    __shared__ float rp[kImgMaps][kImgWH][kImgTileW];
    __shared__ float red[2][kImgWaves];
    const ImgTile t = img_tile(lv, n_levels);
    const int l = t.l, h = lv.h[l], w = lv.w[l], f16 = lv.f16[l];
    const int64_t b = t.b;
    const int y0 = t.y0, x0 = t.x0;
    const int tid = threadIdx.x;
    const int OH = h - kImgRim, OW = w - kImgRim;
    const bool has_pos = y0 < OH && x0 < OW;           // workgroup-uniform: some position lies in this tile
    const int cx = tid % kImgTileW, cy = (tid / kImgTileW) * 2;   // this lane's column and first row of the column pass
    const float* const truth = lv.truth[l];
    const void* const pred = lv.pred[l];
    float* const planes = lv.planes[l];
    const int64_t np = has_pos ? (int64_t)B * C * OH * OW : 0;
    const float eps2 = pm.eps * pm.eps;

    float ssum = 0.0f, csum = 0.0f;
    for (int c = 0; c < C; ++c) {
        // the patch of both images, zeros beyond the image; a tile without positions needs its own pixels only
        for (int e = tid; e < kImgWH * kImgWW; e += kImgThreads) {
            const int r = e / kImgWW, x = e - r * kImgWW;
            const bool own = r < kImgTileH && x < kImgTileW;
            float vt = 0.0f, vp = 0.0f;
            if (r < h - y0 && x < w - x0 && (own || has_pos)) {     // y0 + r formed only where it is inside the image
                const int64_t o = img_offset<LAYOUT>(b, c, y0 + r, x0 + x, h, w, C);
                const float tv = truth[o], pv = img_ld_pred(pred, f16, o);
                vt = tv + pm.offset;
                vp = pv + pm.offset;
                if (own) {
                    const float d = pv - tv;
                    csum += powf(d * d + eps2, pm.q);
                }
            }
            st[r][x] = vt;
            sp[r][x] = vp;
        }
        if (!has_pos) continue;                         // uniform: nobody reads st, sp or rp
        __syncthreads();
        // row pass: 26 rows x 32 columns of the four maps
        for (int i = tid; i < kImgWH * kImgTileW; i += kImgThreads) {
            const int r = i / kImgTileW, x = i - r * kImgTileW;
            float a0 = 0.0f, a1 = 0.0f, a2 = 0.0f, a3 = 0.0f;
#pragma unroll
            for (int k = 0; k < kImgTaps; ++k) {
                const float a = st[r][x + k], bb = sp[r][x + k];
                a0 = __fmaf_rn(pm.g[k], a, a0);
                a1 = __fmaf_rn(pm.g[k], bb, a1);
                a2 = __fmaf_rn(pm.g[k], a * a + bb * bb, a2);
                a3 = __fmaf_rn(pm.g[k], a * bb, a3);
            }
            rp[0][r][x] = a0;
            rp[1][r][x] = a1;
            rp[2][r][x] = a2;
            rp[3][r][x] = a3;
        }
        __syncthreads();
        // column pass: positions (cy, cx) and (cy + 1, cx) of the tile share 10 of their 11 rows, read once
        float m[2][kImgMaps] = {};
#pragma unroll
        for (int k = 0; k <= kImgTaps; ++k) {
#pragma unroll
            for (int i = 0; i < kImgMaps; ++i) {
                const float v = rp[i][cy + k][cx];
                if (k < kImgTaps) m[0][i] = __fmaf_rn(pm.g[k], v, m[0][i]);
                if (k > 0) m[1][i] = __fmaf_rn(pm.g[k - 1], v, m[1][i]);
            }
        }
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            if (cy + j < OH - y0 && cx < OW - x0) {
                const int py = y0 + cy + j, px = x0 + cx;
                const float mt = m[j][0], mp = m[j][1], den1 = m[j][2], tp = m[j][3];
                const float num0 = 2.0f * mt * mp, den0 = mt * mt + mp * mp, num1 = 2.0f * tp;
                const float Bd = den0 + pm.c1, D = den1 - den0 + pm.c2;
                const float lum = (num0 + pm.c1) / Bd, cs = (num1 - num0 + pm.c2) / D;
                ssum += lum * cs;
                const int64_t o = ((b * C + c) * OH + py) * (int64_t)OW + px;
                planes[o] = 2.0f * (mt - lum * mp) / Bd * cs + lum * (2.0f * (cs * mp - mt)) / D;
                planes[np + o] = -(lum * cs) / D;
                planes[2 * np + o] = 2.0f * lum / D;
            }
        }
        __syncthreads();    // the next channel's staging overwrites st, sp and its row pass rp
    }

    const int lane = tid & 63, wid = tid >> 6;
    ssum = img_wave_sum(ssum);
    csum = img_wave_sum(csum);
    if (lane == 0) {
        red[0][wid] = ssum;
        red[1][wid] = csum;
    }
    __syncthreads();
    if (tid < 2) part[(int64_t)blockIdx.x * 2 + tid] = (red[tid][0] + red[tid][1]) + (red[tid][2] + red[tid][3]);
}

// One workgroup, level after level: the level's tiles' partial sums in a fixed order, in double; then the two means and
// the weighted total.
__global__ __launch_bounds__(kImgThreads) void image_loss_fold_kernel(ImgLevels lv, int n_levels, int B, int C,
                                                                    float ssim_weight, const float* __restrict__ part,
                                                                    float* __restrict__ out_losses,
                                                                    float* __restrict__ out_dssim,
                                                                    float* __restrict__ out_charb) {
    __shared__ double red[2][kImgWaves];
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    for (int l = 0; l < n_levels; ++l) {
        double s[2] = {0.0, 0.0};
        for (int i = lv.tile_start[l] + threadIdx.x; i < lv.tile_start[l + 1]; i += kImgThreads) {
            s[0] += (double)part[(int64_t)i * 2];
            s[1] += (double)part[(int64_t)i * 2 + 1];
        }
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            s[k] = img_wave_sum(s[k]);
            if (lane == 0) red[k][wid] = s[k];
        }
        __syncthreads();
        if (threadIdx.x == 0) {
            const int h = lv.h[l], w = lv.w[l];
            const double tot_s = (red[0][0] + red[0][1]) + (red[0][2] + red[0][3]);
            const double tot_c = (red[1][0] + red[1][1]) + (red[1][2] + red[1][3]);
            const bool has = h > kImgRim && w > kImgRim;
            const double N = has ? (double)B * C * (double)(h - kImgRim) * (double)(w - kImgRim) : 0.0;
            const double M = (double)B * C * (double)h * (double)w;
            const double dssim = has ? (1.0 - tot_s / N) / 2.0 : 0.0;
            const double charb = tot_c / M;
            out_dssim[l] = (float)dssim;
            out_charb[l] = (float)charb;
            out_losses[l] = (float)((double)ssim_weight * dssim + (1.0 - (double)ssim_weight) * charb);
        }
        __syncthreads();    // the next level overwrites red
    }
}

template <int LAYOUT>
__global__ __launch_bounds__(kImgThreads) void image_loss_bwd_kernel(ImgLevels lv, int n_levels, int B, int C, ImgParams pm,
                                                                   const float* __restrict__ grad_losses) {
    __shared__ float sP[kImgPlanes][kImgWH][kImgWW];
    __shared__ float rp[kImgPlanes][kImgWH][kImgTileW];
    const ImgTile t = img_tile(lv, n_levels);
    const int l = t.l, h = lv.h[l], w = lv.w[l], f16 = lv.f16[l];
    const int64_t b = t.b;
    const int y0 = t.y0, x0 = t.x0;
    const int tid = threadIdx.x;
    const int OH = h - kImgRim, OW = w - kImgRim;
    const bool ssim = OH > 0 && OW > 0 && pm.ssim_weight > 0.0f;   // workgroup-uniform
    const int cx = tid % kImgTileW, cy = (tid / kImgTileW) * 2;
    const float* const truth = lv.truth[l];
    const void* const pred = lv.pred[l];
    const float* const planes = lv.planes[l];
    const int64_t np = ssim ? (int64_t)B * C * OH * OW : 0;
    const float gl = grad_losses[l];
    const double M = (double)B * C * (double)h * (double)w;
    const float ks = ssim ? (float)(-(double)pm.ssim_weight / (2.0 * (double)np)) : 0.0f;
    const float kc = (float)((1.0 - (double)pm.ssim_weight) * 2.0 * (double)pm.q / M);
    const float eps2 = pm.eps * pm.eps;

    for (int c = 0; c < C; ++c) {
        float T[2][kImgPlanes] = {};
        if (ssim) {
            // the patch of the three planes whose origin is the tile's origin - 10, zeros outside the positions
            for (int e = tid; e < kImgWH * kImgWW; e += kImgThreads) {
                const int r = e / kImgWW, x = e - r * kImgWW;
                const int ry = r - kImgRim, rx = x - kImgRim;       // the position relative to the tile's origin
                float pa = 0.0f, pb = 0.0f, pc = 0.0f;
                if (ry >= -y0 && ry < OH - y0 && rx >= -x0 && rx < OW - x0) {
                    const int jy = y0 + ry, jx = x0 + rx;
                    const int64_t o = ((b * C + c) * OH + jy) * (int64_t)OW + jx;
                    pa = planes[o];
                    pb = planes[np + o];
                    pc = planes[2 * np + o];
                }
                sP[0][r][x] = pa;
                sP[1][r][x] = pb;
                sP[2][r][x] = pc;
            }
            __syncthreads();
            // row pass: pixel column x of the tile takes the positions x - 10 + k, k = 0..10, with the tap 10 - k
            for (int i = tid; i < kImgWH * kImgTileW; i += kImgThreads) {
                const int r = i / kImgTileW, x = i - r * kImgTileW;
                float a0 = 0.0f, a1 = 0.0f, a2 = 0.0f;
#pragma unroll
                for (int k = 0; k < kImgTaps; ++k) {
                    const float gk = pm.g[kImgRim - k];
                    a0 = __fmaf_rn(gk, sP[0][r][x + k], a0);
                    a1 = __fmaf_rn(gk, sP[1][r][x + k], a1);
                    a2 = __fmaf_rn(gk, sP[2][r][x + k], a2);
                }
                rp[0][r][x] = a0;
                rp[1][r][x] = a1;
                rp[2][r][x] = a2;
            }
            __syncthreads();
            // column pass: pixels (cy, cx) and (cy + 1, cx) of the tile share 10 of their 11 rows
#pragma unroll
            for (int k = 0; k <= kImgTaps; ++k) {
#pragma unroll
                for (int i = 0; i < kImgPlanes; ++i) {
                    const float v = rp[i][cy + k][cx];
                    if (k < kImgTaps) T[0][i] = __fmaf_rn(pm.g[kImgRim - k], v, T[0][i]);
                    if (k > 0) T[1][i] = __fmaf_rn(pm.g[kImgRim - (k - 1)], v, T[1][i]);
                }
            }
        }
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            if (cy + j < h - y0 && cx < w - x0) {
                const int64_t o = img_offset<LAYOUT>(b, c, y0 + cy + j, x0 + cx, h, w, C);
                const float tv = truth[o], pv = img_ld_pred(pred, f16, o);
                const float d = pv - tv;
                float g = 0.0f;                                     // ssim_weight = 1: no Charbonnier term at all
                if (kc != 0.0f) g = kc * (d * powf(d * d + eps2, pm.q - 1.0f));
                if (ssim) {
                    const float vt = tv + pm.offset, vp = pv + pm.offset;
                    g = ks * (T[j][0] + 2.0f * vp * T[j][1] + vt * T[j][2]) + g;
                }
                g = gl * g;
                if (f16)
                    reinterpret_cast<__half*>(lv.grad[l])[o] = __float2half_rn(g);
                else
                    reinterpret_cast<float*>(lv.grad[l])[o] = g;
            }
        }
        if (ssim) __syncthreads();    // the next channel's staging overwrites sP and its row pass rp
    }
}

// ---- host side ------------------------------------------------------------------------------------------------------

// tiles of level (h, w) over the batch
static int64_t img_level_tiles(int B, int h, int w) {
    return (int64_t)B * ((h - 1) / kImgTileH + 1) * ((w - 1) / kImgTileW + 1);   // h, w >= 1: no sum near INT_MAX
}

// SSIM positions of level (h, w) over the batch and the channels
static int64_t img_level_positions(int B, int C, int h, int w) {
    return h > kImgRim && w > kImgRim ? (int64_t)B * C * (h - kImgRim) * (w - kImgRim) : 0;
}

int64_t image_loss_total_tiles(int B, const int* h, const int* w, int n) {
    int64_t tiles = 0;
    for (int i = 0; i < n; ++i) tiles += img_level_tiles(B, h[i], w[i]);
    return tiles;
}

// floats: 2 per tile, then 3 planes per level
int64_t image_loss_workspace_floats(int B, int C, const int* h, const int* w, int n) {
    int64_t positions = 0;
    for (int i = 0; i < n; ++i) positions += img_level_positions(B, C, h[i], w[i]);
    return 2 * image_loss_total_tiles(B, h, w, n) + kImgPlanes * positions;
}

const char* image_loss_fwd_kernel() { return "image_loss_fwd_kernel"; }

static void img_fill(ImgLevels& lv, int B, int C, const int* h, const int* w, const int* pred_dtype, int n,
                     const void* const* truth, const void* const* pred, float* ws) {
    float* planes = ws + 2 * image_loss_total_tiles(B, h, w, n);
    lv.tile_start[0] = 0;
    for (int i = 0; i < n; ++i) {
        lv.truth[i] = (const float*)truth[i];
        lv.pred[i] = pred[i];
        lv.h[i] = h[i];
        lv.w[i] = w[i];
        lv.f16[i] = pred_dtype[i] == QPWC_F16;
        lv.tiles_y[i] = (h[i] - 1) / kImgTileH + 1;
        lv.tiles_x[i] = (w[i] - 1) / kImgTileW + 1;
        lv.tile_start[i + 1] = lv.tile_start[i] + (int)img_level_tiles(B, h[i], w[i]);
        lv.planes[i] = planes;
        planes += kImgPlanes * img_level_positions(B, C, h[i], w[i]);
    }
}

static ImgParams img_params(float ssim_weight, float q, float eps, float max_val, float offset) {
    ImgParams pm;
    double e[kImgTaps], sum = 0.0;
    for (int k = 0; k < kImgTaps; ++k) sum += e[k] = exp(-(double)((k - 5) * (k - 5)) / 4.5);
    for (int k = 0; k < kImgTaps; ++k) pm.g[k] = (float)(e[k] / sum);
    pm.c1 = (float)((0.01 * (double)max_val) * (0.01 * (double)max_val));
    pm.c2 = (float)((0.03 * (double)max_val) * (0.03 * (double)max_val));
    pm.offset = offset;
    pm.q = q;
    pm.eps = eps;
    pm.ssim_weight = ssim_weight;
    return pm;
}

int image_loss_fwd_launch(float ssim_weight, float q, float eps, float max_val, float offset, const void* const* truth,
                          const void* const* pred, int B, int C, const int* h, const int* w, const int* pred_dtype,
                          int layout, int n, float* out_losses, float* out_dssim, float* out_charb, float* ws,
                          hipStream_t s) {
    ImgLevels lv = {};
    img_fill(lv, B, C, h, w, pred_dtype, n, truth, pred, ws);
    const ImgParams pm = img_params(ssim_weight, q, eps, max_val, offset);
    const dim3 grid((unsigned)lv.tile_start[n]), block(kImgThreads);
    if (layout == QPWC_NHWC)
        hipLaunchKernelGGL(image_loss_fwd_kernel<QPWC_NHWC>, grid, block, 0, s, lv, n, B, C, pm, ws);
    else
        hipLaunchKernelGGL(image_loss_fwd_kernel<QPWC_NCHW>, grid, block, 0, s, lv, n, B, C, pm, ws);
    const int rc = check_launch(image_loss_fwd_kernel());
    if (rc != QPWC_OK) return rc;
    hipLaunchKernelGGL(image_loss_fold_kernel, dim3(1), block, 0, s, lv, n, B, C, ssim_weight, (const float*)ws,
                       out_losses, out_dssim, out_charb);
    return check_launch("image_loss_fold_kernel");
}

int image_loss_bwd_launch(float ssim_weight, float q, float eps, float offset, const void* const* truth,
                          const void* const* pred, const float* ws, const float* grad_losses, void* const* grad_pred,
                          int B, int C, const int* h, const int* w, const int* pred_dtype, int layout, int n,
                          hipStream_t s) {
    ImgLevels lv = {};
    img_fill(lv, B, C, h, w, pred_dtype, n, truth, pred, const_cast<float*>(ws));
    for (int i = 0; i < n; ++i) lv.grad[i] = grad_pred[i];
    const ImgParams pm = img_params(ssim_weight, q, eps, 1.0f, offset);   // c1, c2 live in the saved planes already
    const dim3 grid((unsigned)lv.tile_start[n]), block(kImgThreads);
    if (layout == QPWC_NHWC)
        hipLaunchKernelGGL(image_loss_bwd_kernel<QPWC_NHWC>, grid, block, 0, s, lv, n, B, C, pm, grad_losses);
    else
        hipLaunchKernelGGL(image_loss_bwd_kernel<QPWC_NCHW>, grid, block, 0, s, lv, n, B, C, pm, grad_losses);
    return check_launch("image_loss_bwd_kernel");
}

}  // namespace qpwc

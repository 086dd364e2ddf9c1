// The interpolation stack's own pieces (qpwcnet/core/pwcnet.py:70-131, non_layers.py:171-193, 276-312) for gfx950
// (MI355X, CDNA4, wave64): the image head Conv2D(3, 1x1) on the 64 features of a FrameInterpolate block, forward and
// backward; Upsample(scale) of an image of 1..4 channels, forward and adjoint; and the chain of AvgPool2D(2, 'same')
// that takes the input frames down to the coarsest level.  fp32, channels-last, dense.  Formulas: include/qpwc.h.
//
// Kernels:
//   image_head_fwd_kernel        16 lanes per pixel, lane q holds channels 4q .. 4q+3 (one 16-byte load) and the 12
//                                weights of those channels; the 16 partial dots are folded by xor shuffles
//   image_head_bwd_kernel        the same roles: grad_z = g W2 as 12 fused multiply-adds per lane and one 16-byte
//                                store; per-workgroup partials of grad_w2 = g^T z and grad_b2 = sum g
//   conv_bwd_reduce_kernel       (conv_bwd.hip, through conv_bwd_reduce_launch) the workgroups' partials per output
//   upsample2x_image_kernel<C>   one thread per output pixel, the arithmetic of upsample2x_flow_kernel (optflow.hip)
//   upsample2x_image_bwd_kernel<C>  one thread per input pixel: 4 x 4 taps of grad_out, separable weights
//   avgpool_pyramid_kernel<C>    one workgroup per tile of 2^levels rows: the first 2 x 2 mean on load (8-byte loads
//                                along W C, every byte of a row read once), the further levels in LDS
//
// Determinism: grids depend on the shape only; a workgroup walks its pixels in grid-stride order; a lane adds its own
// pixels in that order, the 16 lane groups of a workgroup are added in order, the workgroups in the order of
// conv_bwd_reduce_kernel.  No atomics.  What is asked for is a kernel ARGUMENT, not a template parameter: an output's
// bits do not depend on its neighbours.  Contraction is off in the kernels (every fused multiply-add is written out).
// cg_tile_sum of conv_bwd_common.h adds matrix-instruction tiles and has nothing to add here: the 3 x 64 product is
// 12 multiply-adds per lane.
#include "conv_bwd_common.h"
#include "launch.h"

namespace qpwc {

constexpr int kIhC = 64;         // features the image head reads
constexpr int kIhK = 3;          // image channels it writes
constexpr int kIhPx = 64;        // pixels per workgroup and trip: 4 waves x 4 pixels x 4 in flight
constexpr int kIhBlocks = 1000;  // workgroups of the image head kernels (each walks its pixels in grid-stride order)
constexpr int kIhNW = kIhK * kIhC;  // floats of a workgroup's grad_w2 partial
constexpr int kUiBlocks = 1024;     // workgroups of upsample2x_image_kernel, 256 output pixels per trip each
constexpr int kUiBwdBlocks = 256;   // workgroups of upsample2x_image_bwd_kernel, 256 input pixels per trip each
constexpr int kApTilePx = 4096;     // input pixels of a pyramid tile: 2^levels rows x kApTilePx / 2^levels columns
constexpr int kApMaxLevels = 6;     // ... which holds a whole 2^levels square up to here

// sum over the 16 lanes of a pixel: every lane ends with the same bits
__device__ __forceinline__ float ih_fold16(float v) {
    v += __shfl_xor(v, 1);
    v += __shfl_xor(v, 2);
    v += __shfl_xor(v, 4);
    v += __shfl_xor(v, 8);
    return v;
}

// ---- image head ---------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void image_head_fwd_kernel(const float* __restrict__ z, const float* __restrict__ w2,
                                                             const float* __restrict__ b2, float* __restrict__ out,
                                                             int64_t M) {
#pragma clang fp contract(off)
    const int tid = threadIdx.x, q = tid & 15, sub = tid >> 4;  // sub = wave * 4 + pixel of the wave
    float4 wv[kIhK];
#pragma unroll
    for (int k = 0; k < kIhK; ++k) wv[k] = *reinterpret_cast<const float4*>(w2 + k * kIhC + 4 * q);
    const float bias = q < kIhK ? b2[q] : 0.0f;
    for (int64_t p0 = (int64_t)blockIdx.x * kIhPx; p0 < M; p0 += (int64_t)gridDim.x * kIhPx) {
        float4 zv[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int64_t p = p0 + u * 16 + sub;
            zv[u] = p < M ? ldg_f4(z + p * kIhC + 4 * q) : make_float4(0.f, 0.f, 0.f, 0.f);
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int64_t p = p0 + u * 16 + sub;
            float mine = 0.0f;
#pragma unroll
            for (int k = 0; k < kIhK; ++k) {
                const float s = ih_fold16(fmaf(zv[u].w, wv[k].w, fmaf(zv[u].z, wv[k].z, fmaf(zv[u].y, wv[k].y, zv[u].x * wv[k].x))));
                if (q == k) mine = s;
            }
            if (p < M && q < kIhK) out[p * kIhK + q] = mine + bias;
        }
    }
}

// part_w: kIhNW floats per workgroup, part_b: kIhK; grad_z may be null, need_w != 0 asks for the two partials
__global__ __launch_bounds__(256) void image_head_bwd_kernel(const float* __restrict__ z, const float* __restrict__ w2,
                                                             const float* __restrict__ g, float* __restrict__ grad_z,
                                                             float* __restrict__ part_w, float* __restrict__ part_b,
                                                             int64_t M, int need_w) {
#pragma clang fp contract(off)
    __shared__ float red[16 * kIhNW];
    __shared__ float red_b[16 * kIhK];
    const int tid = threadIdx.x, q = tid & 15, sub = tid >> 4;
    float4 wv[kIhK];
#pragma unroll
    for (int k = 0; k < kIhK; ++k) wv[k] = *reinterpret_cast<const float4*>(w2 + k * kIhC + 4 * q);
    float4 aw[kIhK];
    float ab[kIhK];
#pragma unroll
    for (int k = 0; k < kIhK; ++k) aw[k] = make_float4(0.f, 0.f, 0.f, 0.f), ab[k] = 0.0f;
    for (int64_t p0 = (int64_t)blockIdx.x * kIhPx; p0 < M; p0 += (int64_t)gridDim.x * kIhPx) {
        float4 zv[4];
        float gv[4][kIhK];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int64_t p = p0 + u * 16 + sub;
            const bool ok = p < M;
            zv[u] = ok && need_w ? ldg_f4(z + p * kIhC + 4 * q) : make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
            for (int k = 0; k < kIhK; ++k) gv[u][k] = ok ? ldg_f1(g + p * kIhK + k) : 0.0f;
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int64_t p = p0 + u * 16 + sub;
            if (grad_z && p < M) {
                float4 r;
                r.x = fmaf(gv[u][2], wv[2].x, fmaf(gv[u][1], wv[1].x, gv[u][0] * wv[0].x));
                r.y = fmaf(gv[u][2], wv[2].y, fmaf(gv[u][1], wv[1].y, gv[u][0] * wv[0].y));
                r.z = fmaf(gv[u][2], wv[2].z, fmaf(gv[u][1], wv[1].z, gv[u][0] * wv[0].z));
                r.w = fmaf(gv[u][2], wv[2].w, fmaf(gv[u][1], wv[1].w, gv[u][0] * wv[0].w));
                *reinterpret_cast<float4*>(grad_z + p * kIhC + 4 * q) = r;
            }
            if (need_w) {
#pragma unroll
                for (int k = 0; k < kIhK; ++k) {
                    aw[k].x = fmaf(gv[u][k], zv[u].x, aw[k].x);
                    aw[k].y = fmaf(gv[u][k], zv[u].y, aw[k].y);
                    aw[k].z = fmaf(gv[u][k], zv[u].z, aw[k].z);
                    aw[k].w = fmaf(gv[u][k], zv[u].w, aw[k].w);
                    ab[k] += gv[u][k];
                }
            }
        }
    }
    if (!need_w) return;
    // the 16 lane groups of the workgroup, added in order
#pragma unroll
    for (int k = 0; k < kIhK; ++k) {
        *reinterpret_cast<float4*>(&red[sub * kIhNW + k * kIhC + 4 * q]) = aw[k];
        if (q == 0) red_b[sub * kIhK + k] = ab[k];
    }
    __syncthreads();
    if (tid < kIhNW) {
        float s = red[tid];
        for (int j = 1; j < 16; ++j) s += red[j * kIhNW + tid];
        part_w[(int64_t)blockIdx.x * kIhNW + tid] = s;
    } else if (tid < kIhNW + kIhK) {
        const int k = tid - kIhNW;
        float s = red_b[k];
        for (int j = 1; j < 16; ++j) s += red_b[j * kIhK + k];
        part_b[(int64_t)blockIdx.x * kIhK + k] = s;
    }
}

// ---- x2 bilinear upsampling of an image -----------------------------------------------------------------------------------
// scale * (w00 v00 + w01 v01 + w10 v10 + w11 v11): the chain of bilerp_flow (optflow.hip), so that two channels come out
// with the bits of qpwc_upsample2x_flow_fwd
__device__ __forceinline__ float ui_bilerp(float w00, float w01, float w10, float w11, float v00, float v01, float v10,
                                           float v11, float scale) {
    return scale * fmaf(w11, v11, fmaf(w10, v10, fmaf(w01, v01, w00 * v00)));
}

template <int C>
__global__ __launch_bounds__(256) void upsample2x_image_kernel(const float* __restrict__ in, float* __restrict__ out,
                                                               int64_t n_out, int h, int w, float scale) {
#pragma clang fp contract(off)
    const int H = 2 * h, W = 2 * w;
    for (int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x; idx < n_out; idx += (int64_t)gridDim.x * 256) {
        const int x = (int)(idx % W);
        const int y = (int)((idx / W) % H);
        const int64_t b = idx / ((int64_t)W * H);
        const float sy = fmaxf(0.0f, (y + 0.5f) * 0.5f - 0.5f), sx = fmaxf(0.0f, (x + 0.5f) * 0.5f - 0.5f);
        const int y0 = (int)sy, x0 = (int)sx;
        const int y1 = y0 + 1 < h ? y0 + 1 : h - 1, x1 = x0 + 1 < w ? x0 + 1 : w - 1;
        const float ly = sy - y0, lx = sx - x0;
        const float w00 = (1.f - ly) * (1.f - lx), w01 = (1.f - ly) * lx, w10 = ly * (1.f - lx), w11 = ly * lx;
        const float* p = in + b * h * w * C;
        const float *p00 = p + ((int64_t)y0 * w + x0) * C, *p01 = p + ((int64_t)y0 * w + x1) * C,
                    *p10 = p + ((int64_t)y1 * w + x0) * C, *p11 = p + ((int64_t)y1 * w + x1) * C;
        float r[C];
#pragma unroll
        for (int c = 0; c < C; ++c)
            r[c] = ui_bilerp(w00, w01, w10, w11, ldg_f1(p00 + c), ldg_f1(p01 + c), ldg_f1(p10 + c), ldg_f1(p11 + c), scale);
        float* o = out + idx * C;
        if constexpr (C == 4) {
            *reinterpret_cast<float4*>(o) = make_float4(r[0], r[1], r[2], r[3]);
        } else if constexpr (C == 2) {
            *reinterpret_cast<float2*>(o) = make_float2(r[0], r[1]);
        } else {
#pragma unroll
            for (int c = 0; c < C; ++c) o[c] = r[c];
        }
    }
}

// the adjoint: upsample2x_flow_bwd_kernel (flow_head_bwd.hip) for C channels
template <int C>
__global__ __launch_bounds__(256) void upsample2x_image_bwd_kernel(const float* __restrict__ g, float* __restrict__ out,
                                                                   int64_t n_pix, int h, int w, float scale) {
#pragma clang fp contract(off)
    const int H2 = 2 * h, W2 = 2 * w;
    for (int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x; idx < n_pix; idx += (int64_t)gridDim.x * 256) {
        const int j = (int)(idx % w);
        const int i = (int)((idx / w) % h);
        const int64_t b = idx / ((int64_t)w * h);
        // taps 2i-1, 2i, 2i+1, 2i+2 with weights 1/4, 3/4, 3/4, 1/4; a tap past the border is the border's own
        const int ys[4] = {2 * i - 1 < 0 ? 0 : 2 * i - 1, 2 * i, 2 * i + 1, 2 * i + 2 > H2 - 1 ? H2 - 1 : 2 * i + 2};
        const int xs[4] = {2 * j - 1 < 0 ? 0 : 2 * j - 1, 2 * j, 2 * j + 1, 2 * j + 2 > W2 - 1 ? W2 - 1 : 2 * j + 2};
        const float wt[4] = {0.25f, 0.75f, 0.75f, 0.25f};
        const float* gb = g + b * H2 * W2 * C;
        float a[C];
#pragma unroll
        for (int c = 0; c < C; ++c) a[c] = 0.0f;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            float row[C];
#pragma unroll
            for (int c = 0; c < C; ++c) row[c] = 0.0f;
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                const float* p = gb + ((int64_t)ys[r] * W2 + xs[t]) * C;
#pragma unroll
                for (int c = 0; c < C; ++c) row[c] = fmaf(wt[t], ldg_f1(p + c), row[c]);
            }
#pragma unroll
            for (int c = 0; c < C; ++c) a[c] = fmaf(wt[r], row[c], a[c]);
        }
#pragma unroll
        for (int c = 0; c < C; ++c) out[idx * C + c] = scale * a[c];
    }
}

// ---- the pyramid of 2 x 2 means ----------------------------------------------------------------------------------------------
// mean of a 2 x 2 window in row-major order, as a chain of AvgPool2D sums it
__device__ __forceinline__ float ap_mean(float a, float b, float c, float d) { return (((a + b) + c) + d) * 0.25f; }

// One workgroup per tile of S = 2^levels rows and tw columns (a multiple of S, at most TW).  Level 1 is taken on load:
// a thread owns one level-1 pixel and reads the 2 C floats of its pixel pair from both rows as C 8-byte loads, so a
// wave's loads cover its stretch of a row without gaps.  Levels 2 .. levels halve the tile in LDS, one thread per
// element, between two buffers; the last one goes to `out`.
template <int C>
__global__ __launch_bounds__(256) void avgpool_pyramid_kernel(const float* __restrict__ x, float* __restrict__ out,
                                                              int H, int W, int levels, int TW, int tiles_x) {
#pragma clang fp contract(off)
    __shared__ float buf[kApTilePx + kApTilePx / 4];  // level 1: at most S TW C / 4 <= kApTilePx floats (C <= 4)
    const int tid = threadIdx.x, S = 1 << levels, tiles_y = H / S;
    const int tx = blockIdx.x % tiles_x, ty = (blockIdx.x / tiles_x) % tiles_y;
    const int64_t b = blockIdx.x / (tiles_x * tiles_y);
    const int x0 = tx * TW, tw = W - x0 < TW ? W - x0 : TW;
    const int Ho = H >> levels, Wo = W >> levels;
    int rows = S / 2, cols = tw / 2;
    float* dst = levels == 1 ? out + ((b * Ho + ty * rows) * Wo + x0 / 2) * C : buf;
    const int64_t dst_row = levels == 1 ? (int64_t)Wo * C : (int64_t)cols * C;
    const float* src = x + ((b * H + (int64_t)ty * S) * W + x0) * C;
    for (int i = tid; i < rows * cols; i += 256) {
        const int r = i / cols, px = i - r * cols;
        const float* p = src + ((int64_t)(2 * r) * W + 2 * px) * C;
        float top[2 * C], bot[2 * C];
#pragma unroll
        for (int k = 0; k < C; ++k) {
            const float2 t = *reinterpret_cast<const float2*>(p + 2 * k);
            const float2 u = *reinterpret_cast<const float2*>(p + (int64_t)W * C + 2 * k);
            top[2 * k] = t.x, top[2 * k + 1] = t.y, bot[2 * k] = u.x, bot[2 * k + 1] = u.y;
        }
#pragma unroll
        for (int c = 0; c < C; ++c) dst[r * dst_row + px * C + c] = ap_mean(top[c], top[C + c], bot[c], bot[C + c]);
    }
    float* cur = buf;
    float* nxt = buf + kApTilePx;
    for (int l = 2; l <= levels; ++l) {
        __syncthreads();
        const int ld = cols * C;  // floats of a row of the level that is read
        rows >>= 1, cols >>= 1;
        const bool last = l == levels;
        float* d = last ? out + ((b * Ho + ty * rows) * Wo + (x0 >> levels)) * C : nxt;
        const int64_t d_row = last ? (int64_t)Wo * C : (int64_t)cols * C;
        for (int i = tid; i < rows * cols * C; i += 256) {
            const int r = i / (cols * C), j = i - r * cols * C, px = j / C, c = j - px * C;
            const float* p = cur + (2 * r) * ld + 2 * px * C + c;
            d[r * d_row + j] = ap_mean(p[0], p[C], p[ld], p[ld + C]);
        }
        float* t = cur;
        cur = nxt, nxt = t;
    }
}

// ---- host side --------------------------------------------------------------------------------------------------------------
struct IhPlan {
    int blocks;
    int64_t off_pw, off_pb, total;  // workspace offsets in floats, each 16-byte aligned
};

static IhPlan ih_plan(int64_t M) {
    IhPlan p;
    const int64_t want = (M + kIhPx - 1) / kIhPx;
    p.blocks = (int)(want < kIhBlocks ? want : kIhBlocks);
    p.off_pw = 0;
    p.off_pb = p.off_pw + (int64_t)p.blocks * kIhNW;
    p.total = p.off_pb + ((int64_t)p.blocks * kIhK + 3) / 4 * 4;
    return p;
}

int64_t image_head_bwd_workspace_floats(int64_t M) { return ih_plan(M).total; }

int image_head_fwd_launch(const void* z, const void* w2, const void* b2, void* out, int64_t M, hipStream_t s) {
    const IhPlan p = ih_plan(M);
    hipLaunchKernelGGL(image_head_fwd_kernel, dim3((unsigned)p.blocks), dim3(256), 0, s, (const float*)z,
                       (const float*)w2, (const float*)b2, (float*)out, M);
    return check_launch("image_head_fwd_kernel");
}

int image_head_bwd_launch(const void* z, const void* w2, const void* gout, void* gz, void* gw2, void* gb2, void* ws,
                          int64_t M, hipStream_t s) {
    const IhPlan p = ih_plan(M);
    float *part_w = (float*)ws + p.off_pw, *part_b = (float*)ws + p.off_pb;
    const int need_w = gw2 || gb2 ? 1 : 0;
    hipLaunchKernelGGL(image_head_bwd_kernel, dim3((unsigned)p.blocks), dim3(256), 0, s, (const float*)z,
                       (const float*)w2, (const float*)gout, (float*)gz, part_w, part_b, M, need_w);
    int rc = check_launch("image_head_bwd_kernel");
    if (rc) return rc;
    if (gw2 && (rc = conv_bwd_reduce_launch(part_w, (float*)gw2, kIhNW, p.blocks, s))) return rc;
    if (gb2 && (rc = conv_bwd_reduce_launch(part_b, (float*)gb2, kIhK, p.blocks, s))) return rc;
    return QPWC_OK;
}

// f(std::integral_constant<int, C>) for C = 1 .. 4
template <class F>
static void ui_channels(int C, F&& f) {
    if (C == 1) f(std::integral_constant<int, 1>{});
    else if (C == 2) f(std::integral_constant<int, 2>{});
    else if (C == 3) f(std::integral_constant<int, 3>{});
    else f(std::integral_constant<int, 4>{});
}

int upsample2x_image_launch(const void* in, void* out, int B, int h, int w, int C, float scale, hipStream_t s) {
    const int64_t n = (int64_t)B * 4 * h * w, want = (n + 255) / 256;
    const dim3 grid((unsigned)(want < kUiBlocks ? want : kUiBlocks));
    ui_channels(C, [&](auto CC) {
        hipLaunchKernelGGL((upsample2x_image_kernel<decltype(CC)::value>), grid, dim3(256), 0, s, (const float*)in,
                           (float*)out, n, h, w, scale);
    });
    return check_launch("upsample2x_image_kernel");
}

int upsample2x_image_bwd_launch(const void* gout, void* gin, int B, int h, int w, int C, float scale, hipStream_t s) {
    const int64_t n = (int64_t)B * h * w, want = (n + 255) / 256;
    const dim3 grid((unsigned)(want < kUiBwdBlocks ? want : kUiBwdBlocks));
    ui_channels(C, [&](auto CC) {
        hipLaunchKernelGGL((upsample2x_image_bwd_kernel<decltype(CC)::value>), grid, dim3(256), 0, s, (const float*)gout,
                           (float*)gin, n, h, w, scale);
    });
    return check_launch("upsample2x_image_bwd_kernel");
}

int avgpool_pyramid_max_levels() { return kApMaxLevels; }

// tiles of the launch; the caller has checked levels in 1 .. kApMaxLevels and H, W multiples of 2^levels
int64_t avgpool_pyramid_tiles(int B, int H, int W, int levels, int* tw_out) {
    const int S = 1 << levels;
    int TW = kApTilePx / S > S ? kApTilePx / S : S;
    if (TW > W) TW = W;
    if (tw_out) *tw_out = TW;
    return (int64_t)B * (H / S) * ((W + TW - 1) / TW);
}

int avgpool_pyramid_launch(const void* x, void* out, int B, int H, int W, int C, int levels, hipStream_t s) {
    int TW;
    const int64_t tiles = avgpool_pyramid_tiles(B, H, W, levels, &TW);
    const int tiles_x = (W + TW - 1) / TW;
    ui_channels(C, [&](auto CC) {
        hipLaunchKernelGGL((avgpool_pyramid_kernel<decltype(CC)::value>), dim3((unsigned)tiles), dim3(256), 0, s,
                           (const float*)x, (float*)out, H, W, levels, TW, tiles_x);
    });
    return check_launch("avgpool_pyramid_kernel");
}

}  // namespace qpwc

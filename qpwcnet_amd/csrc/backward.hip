// Backward passes of the cost volume and the two warps for gfx950 (MI355X, CDNA4, wave64): what training through
// CostVolume / CostVolumeV2 / Warp / WarpV2 needs (reference: the layers' TF op graphs, qpwcnet/core/layers.py:72-100,
// 128-132, 166-168, 177-186, differentiated by the trainer, qpwcnet/app/optical_flow/train.py).
//
// Lane mapping shared by all kernels here: a group of G = min(64, next_pow2(C)) consecutive lanes owns one pixel, lane
// l of the group channels l, l + G, ... (NC of them per pass).  Every global access of a wave instruction is then one
// contiguous run of G channels per pixel (128 / 256 bytes at C = 32 / 64 fp32), the per-pixel values (cost-volume
// entries, flow) are same-address loads within the group, and a reduction over C stays inside the group.
//
// Determinism: the cost-volume gradients and grad_flo are gathers with a fixed summation order per output element
// (grad_flo: per-lane partial sums in channel order, then a fixed xor butterfly).  Only grad_img is a scatter
// (no-return float atomics), so its bits may vary with the order the atomics land in.
//
// Compiled with -ffp-contract=off semantics inside the helpers, like the forward (`#pragma clang fp contract(off)`).
#include "common.h"
#include "launch.h"

namespace qpwc {

// g' = grad_out * lrelu'(pre-activation), taken from the saved forward output: for slope > 0, out > 0 exactly when the
// pre-activation is > 0, and the tie at 0 takes `slope` like TF's / torch's leaky_relu gradient.
template <typename T>
__device__ __forceinline__ float lrelu_grad(const T* out, const T* gout, int64_t i, float slope) {
    const float o = ld(out + i), g = ld(gout + i);
    return o > 0.0f ? g : g * slope;
}

// ---- cost volume ----------------------------------------------------------------------------------------------------
// out[b,y,x,i*d+j] = lrelu((1/C) sum_c prv[b,y,x,c] nxt[b,y+i-r,x+j-r,c])   (zero outside the image), so
//   grad_prv[b,y,x,c]   = (1/C) sum_ij g'[b,y,x,ij] nxt[b,y+i-r,x+j-r,c]
//   grad_nxt[b,y',x',c] = (1/C) sum_ij g'[b,y'-i+r,x'-j+r,ij] prv[b,y'-i+r,x'-j+r,c]   (source pixels inside the image)
// One group of G lanes per pixel computes both (either may be skipped); NC channels per lane and pass.
template <typename T, int NC>
__global__ __launch_bounds__(256) void cost_volume_bwd_kernel(const T* __restrict__ prv, const T* __restrict__ nxt,
                                                              const T* __restrict__ out, const T* __restrict__ gout,
                                                              T* __restrict__ gprv, T* __restrict__ gnxt, int B, int H,
                                                              int W, int C, int r, int G, int lg2G, float slope,
                                                              float inv_c) {
#pragma clang fp contract(off)
    const int d = 2 * r + 1, D = d * d;
    const int64_t npix = (int64_t)B * H * W;
    const int lane = threadIdx.x & (G - 1);
    const int64_t groups_per_grid = ((int64_t)gridDim.x * blockDim.x) >> lg2G;
    for (int64_t p = (((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> lg2G); p < npix; p += groups_per_grid) {
        const int x = (int)(p % W);
        const int y = (int)((p / W) % H);
        const int64_t bbase = p - ((int64_t)y * W + x);  // first pixel of this image
        for (int c0 = 0; c0 < C; c0 += G * NC) {
            float ap[NC], an[NC];
#pragma unroll
            for (int k = 0; k < NC; ++k) ap[k] = an[k] = 0.0f;
            for (int i = 0; i < d; ++i) {
                const int yn = y + i - r;   // nxt row read by this pixel's grad_prv
                const int ys = y - i + r;   // source row whose output reads nxt at this pixel
                for (int j = 0; j < d; ++j) {
                    const int ij = i * d + j;
                    if (gprv) {
                        const int xn = x + j - r;
                        if (yn >= 0 && yn < H && xn >= 0 && xn < W) {
                            const float g = lrelu_grad(out, gout, p * D + ij, slope);
                            const T* q = nxt + (bbase + (int64_t)yn * W + xn) * C + c0 + lane;
#pragma unroll
                            for (int k = 0; k < NC; ++k)
                                if (c0 + lane + k * G < C) ap[k] += g * ld(q + k * G);
                        }
                    }
                    if (gnxt) {
                        const int xs = x - j + r;
                        if (ys >= 0 && ys < H && xs >= 0 && xs < W) {
                            const int64_t ps = bbase + (int64_t)ys * W + xs;
                            const float g = lrelu_grad(out, gout, ps * D + ij, slope);
                            const T* q = prv + ps * C + c0 + lane;
#pragma unroll
                            for (int k = 0; k < NC; ++k)
                                if (c0 + lane + k * G < C) an[k] += g * ld(q + k * G);
                        }
                    }
                }
            }
#pragma unroll
            for (int k = 0; k < NC; ++k) {
                const int c = c0 + lane + k * G;
                if (c < C) {
                    if (gprv) st(gprv + p * C + c, ap[k] * inv_c);
                    if (gnxt) st(gnxt + p * C + c, an[k] * inv_c);
                }
            }
        }
    }
}

// ---- warp -----------------------------------------------------------------------------------------------------------
// Sum of v over the G lanes of this lane's group (G a power of two <= 64): fixed butterfly, same bits in every lane.
__device__ __forceinline__ float group_sum(float v, int G) {
    for (int m = G >> 1; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
    return v;
}

// Per-pixel set-up of the warp backward: corner indices, the four corner weights of grad_img, and the derivative
// factors of grad_flo.  The sample point is (y + fy, x + fx), as in qpwc_warp_fwd.
struct BwdTaps {
    int y0, y1, x0, x1;
    float w00, w01, w10, w11;  // d out / d corner: (y0,x0) (y0,x1) (y1,x0) (y1,x1)
    // d out / d fx = sum over corners of corner * dx.., d out / d fy likewise
    float dx00, dx01, dx10, dx11, dy00, dy01, dy10, dy11;
};

// WarpV2 (tfa interpolate_bilinear, warp.py:157-185,207): floor = clamp(floor(q), 0, size-2) carries no gradient,
// alpha = clamp(q - floor, 0, 1) passes it on the closed interval [0, 1]; out = ay*(bot - top) + top,
// top = ax*(tr - tl) + tl, bot = ax*(br - bl) + bl.
__device__ __forceinline__ BwdTaps bwd_taps_clamp(int y, int x, float fx, float fy, int H, int W) {
#pragma clang fp contract(off)
    const Taps t = taps_clamp(y, x, fx, fy, H, W);
    BwdTaps b;
    b.y0 = t.y0; b.y1 = t.y1; b.x0 = t.x0; b.x1 = t.x1;
    const float qy = (float)y - (-fy), qx = (float)x - (-fx);
    const float ry = qy - (float)t.y0, rx = qx - (float)t.x0;  // alpha before its clamp
    const float my = (ry >= 0.0f && ry <= 1.0f) ? 1.0f : 0.0f;
    const float mx = (rx >= 0.0f && rx <= 1.0f) ? 1.0f : 0.0f;
    const float ax = t.ax, ay = t.ay;
    b.w00 = (1.0f - ax) * (1.0f - ay);
    b.w01 = ax * (1.0f - ay);
    b.w10 = (1.0f - ax) * ay;
    b.w11 = ax * ay;
    // d/d ax = (1-ay)(tr - tl) + ay (br - bl);  d/d ay = bot - top = (1-ax)(bl - tl) + ax (br - tr)
    b.dx00 = -(1.0f - ay) * mx; b.dx01 = (1.0f - ay) * mx; b.dx10 = -ay * mx; b.dx11 = ay * mx;
    b.dy00 = -(1.0f - ax) * my; b.dy01 = -ax * my; b.dy10 = (1.0f - ax) * my; b.dy11 = ax * my;
    return b;
}

// Warp (tf_warp, warp.py:100-151): truncated, clipped corners carry no gradient; the raw weights
// wa = (x1-x)(y1-y) (x0,y0), wb = (x1-x)(y-y0) (x0,y1), wc = (x-x0)(y1-y) (x1,y0), wd = (x-x0)(y-y0) (x1,y1)
// carry it through the float x, y.  Coinciding clipped corners each receive their own weight.
__device__ __forceinline__ BwdTaps bwd_taps_tfwarp(int y, int x, float fx, float fy, int H, int W) {
#pragma clang fp contract(off)
    const Taps t = taps_tfwarp(y, x, fx, fy, H, W);
    BwdTaps b;
    b.y0 = t.y0; b.y1 = t.y1; b.x0 = t.x0; b.x1 = t.x1;
    b.w00 = t.w00; b.w01 = t.w01; b.w10 = t.w10; b.w11 = t.w11;
    const float xf = (float)x + fx, yf = (float)y + fy;
    const float ey1 = (float)t.y1 - yf, ey0 = yf - (float)t.y0;
    const float ex1 = (float)t.x1 - xf, ex0 = xf - (float)t.x0;
    b.dx00 = -ey1; b.dx10 = -ey0; b.dx01 = ey1; b.dx11 = ey0;
    b.dy00 = -ex1; b.dy10 = ex1; b.dy01 = -ex0; b.dy11 = ex0;
    return b;
}

template <int MODE>
__device__ __forceinline__ BwdTaps make_bwd_taps(int y, int x, float fx, float fy, int H, int W) {
    if (MODE == QPWC_WARP_CLAMP) return bwd_taps_clamp(y, x, fx, fy, H, W);
    return bwd_taps_tfwarp(y, x, fx, fy, H, W);
}

// grad_img (fp32 accumulation target, zeroed before): += weight * grad_out, one no-return float atomic per
// corner and channel.  grad_flo (B,H,W,2) fp32: the group's channel sum, written by lane 0 of the group.
template <typename T, int MODE, int NC>
__global__ __launch_bounds__(256) void warp_bwd_kernel(const T* __restrict__ img, const float* __restrict__ flo,
                                                       const T* __restrict__ gout, float* __restrict__ gimg,
                                                       float* __restrict__ gflo, int B, int H, int W, int C, int G,
                                                       int lg2G) {
#pragma clang fp contract(off)
    const int64_t npix = (int64_t)B * H * W;
    const int lane = threadIdx.x & (G - 1);
    const int64_t groups_per_grid = ((int64_t)gridDim.x * blockDim.x) >> lg2G;
    // every lane of the wave runs the same trip count (the butterfly needs all 64 lanes)
    const int64_t p_first = ((int64_t)blockIdx.x * blockDim.x + (threadIdx.x & ~63)) >> lg2G;
    for (int64_t pw = p_first; pw < npix; pw += groups_per_grid) {
        const int64_t p = pw + ((threadIdx.x & 63) >> lg2G);
        const bool live = p < npix;
        const int64_t pc = live ? p : npix - 1;
        const int x = (int)(pc % W);
        const int y = (int)((pc / W) % H);
        const int64_t ibase = (pc - ((int64_t)y * W + x)) * C;
        const float fx = flo[2 * pc], fy = flo[2 * pc + 1];
        const BwdTaps t = make_bwd_taps<MODE>(y, x, fx, fy, H, W);
        const int64_t o00 = ibase + ((int64_t)t.y0 * W + t.x0) * C, o01 = ibase + ((int64_t)t.y0 * W + t.x1) * C;
        const int64_t o10 = ibase + ((int64_t)t.y1 * W + t.x0) * C, o11 = ibase + ((int64_t)t.y1 * W + t.x1) * C;
        float sx = 0.0f, sy = 0.0f;
        for (int c0 = 0; c0 < C; c0 += G * NC) {
#pragma unroll
            for (int k = 0; k < NC; ++k) {
                const int c = c0 + lane + k * G;
                if (!live || c >= C) continue;
                const float g = ld(gout + pc * C + c);
                if (gflo) {
                    const float v00 = ld(img + o00 + c), v01 = ld(img + o01 + c);
                    const float v10 = ld(img + o10 + c), v11 = ld(img + o11 + c);
                    sx += g * (((t.dx00 * v00 + t.dx10 * v10) + t.dx01 * v01) + t.dx11 * v11);
                    sy += g * (((t.dy00 * v00 + t.dy10 * v10) + t.dy01 * v01) + t.dy11 * v11);
                }
                if (gimg) {
                    unsafeAtomicAdd(gimg + o00 + c, t.w00 * g);
                    unsafeAtomicAdd(gimg + o01 + c, t.w01 * g);
                    unsafeAtomicAdd(gimg + o10 + c, t.w10 * g);
                    unsafeAtomicAdd(gimg + o11 + c, t.w11 * g);
                }
            }
        }
        if (gflo) {
            sx = group_sum(sx, G);
            sy = group_sum(sy, G);
            if (live && lane == 0) {
                gflo[2 * p] = sx;
                gflo[2 * p + 1] = sy;
            }
        }
    }
}

__global__ __launch_bounds__(256) void fill_zero_kernel(float* __restrict__ p, int64_t n) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
        p[i] = 0.0f;
}

__global__ __launch_bounds__(256) void f32_to_f16_kernel(const float* __restrict__ src, __half* __restrict__ dst,
                                                         int64_t n) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
        dst[i] = __float2half_rn(src[i]);
}

// ---- host side ------------------------------------------------------------------------------------------------------
static void group_of(int C, int* G, int* lg2G) {
    int g = 1, l = 0;
    while (g < C && g < 64) { g <<= 1; ++l; }
    *G = g;
    *lg2G = l;
}

static unsigned grid_for(int64_t threads) {
    const int64_t want = (threads + 255) / 256;
    return (unsigned)(want < (1 << 20) ? want : (1 << 20));
}

template <typename T>
static int cost_volume_bwd_impl(const void* prv, const void* nxt, const void* out, const void* gout, void* gprv,
                                void* gnxt, int B, int H, int W, int C, int r, float slope, hipStream_t s) {
    int G, l;
    group_of(C, &G, &l);
    const unsigned grid = grid_for((int64_t)B * H * W * G);
    const float inv_c = 1.0f / (float)C;
#define QPWC_CVB(NC)                                                                                                   \
    hipLaunchKernelGGL((cost_volume_bwd_kernel<T, NC>), dim3(grid), dim3(256), 0, s, (const T*)prv, (const T*)nxt,  \
                       (const T*)out, (const T*)gout, (T*)gprv, (T*)gnxt, B, H, W, C, r, G, l, slope, inv_c)
    if (C <= 64) QPWC_CVB(1);
    else if (C <= 128) QPWC_CVB(2);
    else QPWC_CVB(4);
#undef QPWC_CVB
    return check_launch("cost_volume_bwd_kernel");
}

int cost_volume_bwd_launch(const void* prv, const void* nxt, const void* out, const void* gout, void* gprv,
                           void* gnxt, int B, int H, int W, int C, int r, int dtype, float slope, hipStream_t s) {
    if (dtype == QPWC_F32) return cost_volume_bwd_impl<float>(prv, nxt, out, gout, gprv, gnxt, B, H, W, C, r, slope, s);
    return cost_volume_bwd_impl<__half>(prv, nxt, out, gout, gprv, gnxt, B, H, W, C, r, slope, s);
}

template <typename T, int MODE>
static int warp_bwd_impl(const void* img, const float* flo, const void* gout, float* gacc, float* gflo, int B, int H,
                         int W, int C, hipStream_t s) {
    int G, l;
    group_of(C, &G, &l);
    // whole waves per group set: threads = pixels * G rounded up to 64
    const int64_t threads = ((int64_t)B * H * W * G + 63) / 64 * 64;
    const unsigned grid = grid_for(threads);
#define QPWC_WB(NC)                                                                                                    \
    hipLaunchKernelGGL((warp_bwd_kernel<T, MODE, NC>), dim3(grid), dim3(256), 0, s, (const T*)img, flo,            \
                       (const T*)gout, gacc, gflo, B, H, W, C, G, l)
    if (C <= 64) QPWC_WB(1);
    else if (C <= 128) QPWC_WB(2);
    else QPWC_WB(4);
#undef QPWC_WB
    return check_launch("warp_bwd_kernel");
}

int warp_bwd_launch(const void* img, const void* flo, const void* gout, void* gimg, void* gflo, void* ws, int B,
                    int H, int W, int C, int dtype, int mode, hipStream_t s) {
    const int64_t n = (int64_t)B * H * W * C;
    // fp32: accumulate in grad_img itself; fp16: in the fp32 workspace, cast once at the end
    float* acc = gimg ? (dtype == QPWC_F32 ? (float*)gimg : (float*)ws) : nullptr;
    if (acc) {
        hipLaunchKernelGGL(fill_zero_kernel, dim3(grid_for(n)), dim3(256), 0, s, acc, n);
        const int rc = check_launch("fill_zero_kernel");
        if (rc) return rc;
    }
    const float* f = (const float*)flo;
    int rc;
    if (dtype == QPWC_F32)
        rc = mode == QPWC_WARP_CLAMP ? warp_bwd_impl<float, QPWC_WARP_CLAMP>(img, f, gout, acc, (float*)gflo, B, H, W, C, s)
                                     : warp_bwd_impl<float, QPWC_WARP_TFWARP>(img, f, gout, acc, (float*)gflo, B, H, W, C, s);
    else
        rc = mode == QPWC_WARP_CLAMP ? warp_bwd_impl<__half, QPWC_WARP_CLAMP>(img, f, gout, acc, (float*)gflo, B, H, W, C, s)
                                     : warp_bwd_impl<__half, QPWC_WARP_TFWARP>(img, f, gout, acc, (float*)gflo, B, H, W, C, s);
    if (rc || !gimg || dtype == QPWC_F32) return rc;
    hipLaunchKernelGGL(f32_to_f16_kernel, dim3(grid_for(n)), dim3(256), 0, s, (const float*)ws, (__half*)gimg, n);
    return check_launch("f32_to_f16_kernel");
}

}  // namespace qpwc

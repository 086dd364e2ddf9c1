// Backward pass of the fused SeparableConv2D(3x3,'same') (+ Mish on load / on store) for gfx950 (MI355X, CDNA4,
// wave64): what training through the OptFlow / FrameInterpolate layers needs (reference: the TF op graph of
// qpwcnet/core/non_layers.py:223-231, differentiated by the trainer, qpwcnet/app/optical_flow/train.py).  fp32,
// channels-last, the sources read through their pixel strides as the forward reads them.
//
//   x = concat(src_0..src_{n-1}) (C channels), a = Mish(x) if bit 0 else x
//   d[p,c] = sum_{ky,kx} dw[c,ky,kx] a[p+(ky-1,kx-1),c]     (zero outside the image)
//   z[p,f] = bias[f] + sum_c pw[f,c] d[p,c],  out = Mish(z) if bit 1 else z
// given g = dL/dout:
//   gz = g Mish'(z) if bit 1 else g
//   grad_bias[f] = sum_p gz[p,f]          grad_pw[f,c] = sum_p gz[p,f] d[p,c]        gd[p,c] = sum_f gz[p,f] pw[f,c]
//   grad_dw[c,ky,kx] = sum_p gd[p,c] a[p+(ky-1,kx-1),c]     ga[p,c] = sum_{ky,kx} dw[c,ky,kx] gd[p-(ky-1,kx-1),c]
//   grad_x = ga Mish'(x) if bit 0 else ga, split into one dense (B,H,W,c_i) tensor per source
//
// Mish is not invertible, so z is not recovered from the stored output: d is recomputed (it is needed for grad_pw
// anyway) and z taken from it.  Stages, each skipped when nothing that is asked for consumes it:
//   A  sepconv_bwd_d_kernel    d into the (M, Cpad) workspace, M = B H W, Cpad = ceil(C / 32) 32, pad columns 0
//   B1 sepconv_bwd_gz_kernel   z = d pw^T + bias on v_mfma_f32_16x16x4_f32, gz = g Mish'(z) -> (M, F) workspace (bit 1 only)
//   B2 sepconv_bwd_pw_kernel   per (pixel-block group, 32-channel chunk): gd = gz pw -> workspace, partial grad_pw = gz^T d
//                              (both on the fp32 matrix instructions, >= 2 independent accumulators per wave), partial grad_bias
//   C  sepconv_bwd_dw_kernel   ga as a gather of gd through the transposed taps, times Mish'(x), stored per source;
//                              partial grad_dw
//   D  sepconv_bwd_reduce_kernel  the partials of grad_pw / grad_bias / grad_dw summed in workgroup order
//
// Determinism: every output element is a gather with a fixed summation order; the weight gradients are a two-stage
// reduction (per workgroup: pixel blocks in grid-stride order, waves 0..3 / slots 0..7 in order; then stage D over the
// workgroups in order).  No atomics.  A pixel's gz, gd and grad_x depend on its own image only.
#include "conv_bwd_common.h"
#include "launch.h"

namespace qpwc {

constexpr int kScbPx = 64;          // pixels per block of the pointwise backward: 16 per wave, 4 waves
constexpr int kScbPwBlocks = 512;   // workgroups of sepconv_bwd_pw_kernel, shared between the pixel groups and the chunks
constexpr int kScbStrip = 4;        // consecutive pixels of one row per thread in stages A and C
constexpr int kScbDwSlots = 8;      // strips per workgroup trip of sepconv_bwd_dw_kernel (256 threads = 8 x 32 channels)
constexpr int kScbDwBlocks = 1024;  // workgroups of sepconv_bwd_dw_kernel, shared likewise
constexpr int kScbLd = kScKC + 4;   // LDS row of a 32-channel tile: 16-byte rows, 4 banks apart

struct ScbGrad {
    float* ptr[3];  // dense (B,H,W,c_i) gradient of each source; NULL = not asked for
};

// 3 rows x 6 columns around the strip (y, x0 .. x0+3) of one channel, zero outside the image
__device__ __forceinline__ void scb_window(const float* p, int64_t ps, int y, int x0, int H, int W, float (&w)[3][6]) {
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        const int yy = y - 1 + r;
        const bool row_ok = yy >= 0 && yy < H;
#pragma unroll
        for (int j = 0; j < 6; ++j) {
            const int xx = x0 - 1 + j;
            w[r][j] = (row_ok && xx >= 0 && xx < W) ? ldg_f1(p + ((int64_t)yy * W + xx) * ps) : 0.0f;
        }
    }
}

// ---- stage A: d = depthwise3x3(a) ---------------------------------------------------------------------------------
// thread = (strip of 4 pixels, channel of Cpad): consecutive lanes read consecutive channels of a source.
template <bool ACT>
__global__ __launch_bounds__(256) void sepconv_bwd_d_kernel(DwSrc src, const float* __restrict__ dw,
                                                            float* __restrict__ d, int H, int W, int C, int cpad,
                                                            int wq, int64_t n_threads) {
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= n_threads) return;
    const int c = (int)(idx % cpad);
    const int64_t strip = idx / cpad;
    const int x0 = (int)(strip % wq) * kScbStrip;
    const int64_t row = strip / wq;  // b * H + y
    const int y = (int)(row % H);
    const int64_t b = row / H;
    float o[kScbStrip] = {0.0f, 0.0f, 0.0f, 0.0f};
    if (c < C) {
        const DwPick k = dwsrc_pick(src, c, C);
        const float* p = (const float*)k.p + b * H * W * k.ps + k.cc;
        float a[3][6];
        scb_window(p, k.ps, y, x0, H, W, a);
        if (ACT) {
#pragma unroll
            for (int r = 0; r < 3; ++r)
#pragma unroll
                for (int j = 0; j < 6; ++j) a[r][j] = mishf(a[r][j]);  // mishf(0) = 0: the zero padding stays
        }
        float w[9];
#pragma unroll
        for (int t = 0; t < 9; ++t) w[t] = dw[c * 9 + t];
#pragma unroll
        for (int i = 0; i < kScbStrip; ++i) {
            float s = 0.0f;
#pragma unroll
            for (int ky = 0; ky < 3; ++ky)
#pragma unroll
                for (int kx = 0; kx < 3; ++kx) s = fmaf(w[ky * 3 + kx], a[ky][i + kx], s);
            o[i] = s;
        }
    }
    float* q = d + (row * W + x0) * cpad + c;
#pragma unroll
    for (int i = 0; i < kScbStrip; ++i)
        if (x0 + i < W) q[(int64_t)i * cpad] = o[i];
}

// ---- stage B1: gz = g * Mish'(d pw^T + bias) ----------------------------------------------------------------------
// One workgroup per 64 pixels; wave w owns pixels 16 w .. 16 w + 15 and all F columns: F / 16 accumulators.
// v_mfma_f32_16x16x4_f32: lane l holds A[i = l & 15][k = l >> 4] and B[k = l >> 4][j = l & 15]; D register r of lane l
// is row (l >> 4) * 4 + r, column l & 15.
template <int F>
__global__ __launch_bounds__(256) void sepconv_bwd_gz_kernel(const float* __restrict__ d, const float* __restrict__ pw,
                                                             const float* __restrict__ bias,
                                                             const float* __restrict__ gout, float* __restrict__ gz,
                                                             int64_t M, int cpad) {
    __shared__ __attribute__((aligned(16))) float d_s[kScbPx * kScbLd];
    __shared__ __attribute__((aligned(16))) float pw_s[F * kScbLd];
    constexpr int NT = F / 16;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int li = lane & 15, lk = lane >> 4;
    const int64_t p0 = (int64_t)blockIdx.x * kScbPx;
    f32x4v acc[NT];
#pragma unroll
    for (int n = 0; n < NT; ++n) acc[n] = f32x4v{0.0f, 0.0f, 0.0f, 0.0f};
    for (int k0 = 0; k0 < cpad; k0 += kScKC) {
        __syncthreads();  // the previous chunk's fragments are read
        for (int i = tid; i < kScbPx * 8; i += 256) {
            const int r = i >> 3, q = i & 7;
            const int64_t p = p0 + r;
            const float4 v = p < M ? ldg_f4(d + p * cpad + k0 + q * 4) : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            *reinterpret_cast<float4*>(&d_s[r * kScbLd + q * 4]) = v;
        }
        for (int i = tid; i < F * 8; i += 256) {
            const int r = i >> 3, q = i & 7;
            *reinterpret_cast<float4*>(&pw_s[r * kScbLd + q * 4]) = ldg_f4(pw + (int64_t)r * cpad + k0 + q * 4);
        }
        __syncthreads();
#pragma unroll
        for (int kk = 0; kk < kScKC; kk += 4) {
            const float a = d_s[(wave * 16 + li) * kScbLd + kk + lk];
#pragma unroll
            for (int n = 0; n < NT; ++n)
                acc[n] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, pw_s[(n * 16 + li) * kScbLd + kk + lk], acc[n], 0, 0, 0);
        }
    }
#pragma unroll
    for (int n = 0; n < NT; ++n) {
        const int f = n * 16 + li;
        const float bf = bias[f];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int64_t p = p0 + wave * 16 + lk * 4 + r;
            if (p < M) gz[p * F + f] = gout[p * F + f] * mish_grad(acc[n][r] + bf);
        }
    }
}

// ---- stage B2: gd = gz pw, partial grad_pw = gz^T d, partial grad_bias ---------------------------------------------
// grid (pixel-block groups, 32-channel chunks).  A workgroup walks its pixel blocks in grid-stride order; wave w owns
// pixels 16 w .. 16 w + 15 of a block: two gd tiles (K = F) and 2 F / 16 grad_pw tiles (K = its 16 pixels), whose
// accumulators live across the walk.  At the end the four waves' grad_pw tiles are added in wave order through LDS
// (cg_tile_sum of conv_bwd_common.h, shared with the convolution backward passes).
template <int F>
__global__ __launch_bounds__(256) void sepconv_bwd_pw_kernel(const float* __restrict__ gz, const float* __restrict__ d,
                                                             const float* __restrict__ pw, float* __restrict__ gd,
                                                             float* __restrict__ part_pw, float* __restrict__ part_b,
                                                             int64_t M, int cpad, int64_t n_pb, int need_gd,
                                                             int need_pw, int need_b) {
    constexpr int SG = F + 20;  // gz_s row: rows 20 banks apart (the pixel-major A fragment is conflict free)
    constexpr int NT = F / 16;
    __shared__ __attribute__((aligned(16))) float gz_s[kScbPx * SG];
    __shared__ __attribute__((aligned(16))) float d_s[kScbPx * kScbLd];
    __shared__ __attribute__((aligned(16))) float pw_s[F * kScbLd];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int li = lane & 15, lk = lane >> 4;
    const int c0 = blockIdx.y * kScKC;
    f32x4v accw[NT][2];
#pragma unroll
    for (int n = 0; n < NT; ++n) accw[n][0] = accw[n][1] = f32x4v{0.0f, 0.0f, 0.0f, 0.0f};
    float bsum = 0.0f;
    const bool do_b = need_b && blockIdx.y == 0 && tid < F;
    if (need_gd)
        for (int i = tid; i < F * 8; i += 256) {
            const int r = i >> 3, q = i & 7;
            *reinterpret_cast<float4*>(&pw_s[r * kScbLd + q * 4]) = ldg_f4(pw + (int64_t)r * cpad + c0 + q * 4);
        }
    for (int64_t pb = blockIdx.x; pb < n_pb; pb += gridDim.x) {
        const int64_t p0 = pb * kScbPx;
        __syncthreads();  // the previous block's tiles are read
        for (int i = tid; i < kScbPx * (F / 4); i += 256) {
            const int r = i / (F / 4), q = i % (F / 4);
            const int64_t p = p0 + r;
            const float4 v = p < M ? ldg_f4(gz + p * F + q * 4) : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            *reinterpret_cast<float4*>(&gz_s[r * SG + q * 4]) = v;
        }
        if (need_pw)
            for (int i = tid; i < kScbPx * 8; i += 256) {
                const int r = i >> 3, q = i & 7;
                const int64_t p = p0 + r;
                const float4 v = p < M ? ldg_f4(d + p * cpad + c0 + q * 4) : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
                *reinterpret_cast<float4*>(&d_s[r * kScbLd + q * 4]) = v;
            }
        __syncthreads();
        if (need_gd) {
            f32x4v a0 = f32x4v{0.0f, 0.0f, 0.0f, 0.0f}, a1 = a0;
#pragma unroll 8
            for (int k = 0; k < F; k += 4) {
                const float a = gz_s[(wave * 16 + li) * SG + k + lk];
                a0 = __builtin_amdgcn_mfma_f32_16x16x4f32(a, pw_s[(k + lk) * kScbLd + li], a0, 0, 0, 0);
                a1 = __builtin_amdgcn_mfma_f32_16x16x4f32(a, pw_s[(k + lk) * kScbLd + 16 + li], a1, 0, 0, 0);
            }
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int64_t p = p0 + wave * 16 + lk * 4 + r;
                if (p < M) {
                    gd[p * cpad + c0 + li] = a0[r];
                    gd[p * cpad + c0 + 16 + li] = a1[r];
                }
            }
        }
        if (need_pw) {
#pragma unroll
            for (int k = 0; k < 16; k += 4) {
                const int row = wave * 16 + k + lk;
                const float b0 = d_s[row * kScbLd + li], b1 = d_s[row * kScbLd + 16 + li];
#pragma unroll
                for (int n = 0; n < NT; ++n) {
                    const float a = gz_s[row * SG + n * 16 + li];
                    accw[n][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, b0, accw[n][0], 0, 0, 0);
                    accw[n][1] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, b1, accw[n][1], 0, 0, 0);
                }
            }
        }
        if (do_b)
            for (int r = 0; r < kScbPx; ++r) bsum += gz_s[r * SG + tid];
    }
    if (need_pw)  // red = gz_s: F x 32 floats, smaller than the gz tile; every column of the chunk lies within cpad
        cg_tile_sum<NT, kScKC / 16>(accw, gz_s, part_pw, (int64_t)blockIdx.x * F, cpad, c0, cpad, tid);
    if (do_b) part_b[(int64_t)blockIdx.x * F + tid] = bsum;
}

// ---- stage C: grad_x = (transposed depthwise of gd) * Mish'(x), partial grad_dw -----------------------------------
// grid (strip groups, 32-channel chunks); thread = (slot of 8, channel of the chunk), one strip of 4 pixels per trip.
template <bool ACT, bool NEED_DW>
__global__ __launch_bounds__(256) void sepconv_bwd_dw_kernel(DwSrc src, ScbGrad gsrc, const float* __restrict__ dw,
                                                             const float* __restrict__ gd, float* __restrict__ part_dw,
                                                             int H, int W, int C, int cpad, int wq, int64_t n_strips,
                                                             int64_t n_groups) {
    __shared__ float red[NEED_DW ? kScbDwSlots * kScKC * 9 : 1];
    const int tid = threadIdx.x, cl = tid & 31, slot = tid >> 5;
    const int c = blockIdx.y * kScKC + cl;
    const bool live = c < C;
    const int cs = live ? c : C - 1;
    const DwPick k = dwsrc_pick(src, cs, C);
    const int e0 = src.ch[0], e1 = e0 + src.ch[1];
    // the gradient tensor of the source that holds channel cs, branch free like dwsrc_pick
    const uint64_t m0 = 0ull - (uint64_t)(cs < e0), m1 = (0ull - (uint64_t)(cs < e1)) & ~m0, m2 = ~(m0 | m1);
    float* gp = (float*)(((uint64_t)gsrc.ptr[0] & m0) | ((uint64_t)gsrc.ptr[1] & m1) | ((uint64_t)gsrc.ptr[2] & m2));
    const int gch = (src.ch[0] & (int)m0) | (src.ch[1] & (int)m1) | (src.ch[2] & (int)m2);
    float w[9], acc[9];
#pragma unroll
    for (int t = 0; t < 9; ++t) {
        w[t] = dw[cs * 9 + t];
        acc[t] = 0.0f;
    }
    for (int64_t g = blockIdx.x; g < n_groups; g += gridDim.x) {
        const int64_t strip = g * kScbDwSlots + slot;
        if (!live || strip >= n_strips) continue;
        const int x0 = (int)(strip % wq) * kScbStrip;
        const int64_t row = strip / wq;
        const int y = (int)(row % H);
        const int64_t b = row / H;
        float G[3][6];
        scb_window(gd + b * H * W * cpad + c, cpad, y, x0, H, W, G);
        const float* xp = (const float*)k.p + b * H * W * k.ps + k.cc;
        float raw[kScbStrip] = {0.0f, 0.0f, 0.0f, 0.0f};
        if (NEED_DW) {
            float a[3][6];
            scb_window(xp, k.ps, y, x0, H, W, a);
#pragma unroll
            for (int i = 0; i < kScbStrip; ++i) raw[i] = a[1][i + 1];
            if (ACT) {
#pragma unroll
                for (int r = 0; r < 3; ++r)
#pragma unroll
                    for (int j = 0; j < 6; ++j) a[r][j] = mishf(a[r][j]);
            }
            // G is zero outside the image, so a strip's pixels past W add nothing
#pragma unroll
            for (int i = 0; i < kScbStrip; ++i)
#pragma unroll
                for (int ky = 0; ky < 3; ++ky)
#pragma unroll
                    for (int kx = 0; kx < 3; ++kx) acc[ky * 3 + kx] = fmaf(G[1][i + 1], a[ky][i + kx], acc[ky * 3 + kx]);
        } else if (ACT) {
#pragma unroll
            for (int i = 0; i < kScbStrip; ++i)
                if (x0 + i < W) raw[i] = ldg_f1(xp + ((int64_t)y * W + x0 + i) * k.ps);
        }
        if (gp) {
            float* q = gp + ((row * W) + x0) * gch + k.cc;
#pragma unroll
            for (int i = 0; i < kScbStrip; ++i) {
                float s = 0.0f;
#pragma unroll
                for (int ky = 0; ky < 3; ++ky)
#pragma unroll
                    for (int kx = 0; kx < 3; ++kx) s = fmaf(w[ky * 3 + kx], G[2 - ky][i + 2 - kx], s);
                if (ACT) s *= mish_grad(raw[i]);
                if (x0 + i < W) q[(int64_t)i * gch] = s;
            }
        }
    }
    if (NEED_DW) {
#pragma unroll
        for (int t = 0; t < 9; ++t) red[(slot * kScKC + cl) * 9 + t] = acc[t];
        __syncthreads();
        if (slot == 0 && live) {
#pragma unroll
            for (int t = 0; t < 9; ++t) {
                float s = red[cl * 9 + t];
                for (int j = 1; j < kScbDwSlots; ++j) s += red[(j * kScKC + cl) * 9 + t];
                part_dw[((int64_t)blockIdx.x * C + c) * 9 + t] = s;
            }
        }
    }
}

// ---- stage D: out[i] = sum over the workgroups' partials, in workgroup order; columns >= row_valid of a row are 0 ---
__global__ __launch_bounds__(256) void sepconv_bwd_reduce_kernel(const float* __restrict__ part, float* __restrict__ out,
                                                                 int n_out, int n_part, int row_len, int row_valid) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n_out) return;
    float s = 0.0f;
    if (i % row_len < row_valid)
        for (int p = 0; p < n_part; ++p) s += part[(int64_t)p * n_out + i];
    out[i] = s;
}

// ---- host side -----------------------------------------------------------------------------------------------------
struct ScbPlan {
    int64_t M, n_pb, n_strips, n_groups;
    int cpad, chunks, wq, pw_x, dw_x;
    int64_t off_d, off_gd, off_gz, off_ppw, off_pb, off_pdw, total;  // workspace offsets, in floats, 16-byte aligned
};

static ScbPlan scb_plan(int B, int H, int W, int C, int F) {
    ScbPlan p;
    p.M = (int64_t)B * H * W;
    p.cpad = (C + kScKC - 1) / kScKC * kScKC;
    p.chunks = p.cpad / kScKC;
    p.n_pb = (p.M + kScbPx - 1) / kScbPx;
    p.wq = (W + kScbStrip - 1) / kScbStrip;
    p.n_strips = (int64_t)B * H * p.wq;
    p.n_groups = (p.n_strips + kScbDwSlots - 1) / kScbDwSlots;
    const int pw_cap = kScbPwBlocks / p.chunks > 0 ? kScbPwBlocks / p.chunks : 1;
    const int dw_cap = kScbDwBlocks / p.chunks > 0 ? kScbDwBlocks / p.chunks : 1;
    p.pw_x = (int)(p.n_pb < pw_cap ? p.n_pb : pw_cap);
    p.dw_x = (int)(p.n_groups < dw_cap ? p.n_groups : dw_cap);
    auto up4 = [](int64_t n) { return (n + 3) / 4 * 4; };
    p.off_d = 0;
    p.off_gd = p.off_d + p.M * p.cpad;
    p.off_gz = p.off_gd + p.M * p.cpad;
    p.off_ppw = p.off_gz + up4(p.M * F);
    p.off_pb = p.off_ppw + (int64_t)p.pw_x * F * p.cpad;
    p.off_pdw = p.off_pb + up4((int64_t)p.pw_x * F);
    p.total = p.off_pdw + up4((int64_t)p.dw_x * C * 9);
    return p;
}

int64_t sepconv3x3_bwd_workspace_floats(int B, int H, int W, int C, int F) { return scb_plan(B, H, W, C, F).total; }

// whether the launch grids of a shape fit (stage A is one thread per (strip, channel of Cpad))
bool sepconv3x3_bwd_shape_ok(int B, int H, int W, int C, int F) {
    const ScbPlan p = scb_plan(B, H, W, C, F);
    return p.chunks <= 65535 && (p.n_strips * p.cpad + 255) / 256 <= INT32_MAX && p.n_pb <= INT32_MAX &&
           (int64_t)F * p.cpad <= INT32_MAX / 2 && (int64_t)C * 9 <= INT32_MAX / 2;
}

template <int F>
static int scb_pointwise(const ScbPlan& p, const float* d, const float* pw, const float* bias, const float* gout,
                         float* gz_ws, float* gd, float* part_pw, float* part_b, bool act_out, bool need_gd,
                         bool need_pw, bool need_b, hipStream_t s) {
    const float* gz = gout;
    if (act_out) {
        hipLaunchKernelGGL((sepconv_bwd_gz_kernel<F>), dim3((unsigned)p.n_pb), dim3(256), 0, s, d, pw, bias, gout,
                           gz_ws, p.M, p.cpad);
        const int rc = check_launch("sepconv_bwd_gz_kernel");
        if (rc) return rc;
        gz = gz_ws;
    }
    // only grad_bias: one chunk column of workgroups that sums gz
    const unsigned gy = (need_gd || need_pw) ? (unsigned)p.chunks : 1u;
    hipLaunchKernelGGL((sepconv_bwd_pw_kernel<F>), dim3((unsigned)p.pw_x, gy), dim3(256), 0, s, gz, d, pw, gd, part_pw,
                       part_b, p.M, p.cpad, p.n_pb, (int)need_gd, (int)need_pw, (int)need_b);
    return check_launch("sepconv_bwd_pw_kernel");
}

static int scb_reduce(const float* part, float* out, int64_t n_out, int n_part, int row_len, int row_valid,
                      hipStream_t s) {
    hipLaunchKernelGGL(sepconv_bwd_reduce_kernel, dim3((unsigned)((n_out + 255) / 256)), dim3(256), 0, s, part, out,
                       (int)n_out, n_part, row_len, row_valid);
    return check_launch("sepconv_bwd_reduce_kernel");
}

int sepconv3x3_bwd_launch(const void* const* srcs, const int* chans, const int64_t* strides, int n_src, int flags,
                          const void* dw, const void* pw, const void* bias, const void* gout, void* const* gsrc,
                          void* gdw, void* gpw, void* gbias, void* ws, int B, int H, int W, int F, hipStream_t s) {
    DwSrc src;
    ScbGrad gs;
    int C = 0;
    bool need_src = false;
    for (int i = 0; i < 3; ++i) {
        src.ptr[i] = i < n_src ? srcs[i] : nullptr;
        src.ch[i] = i < n_src ? chans[i] : 0;
        src.stride[i] = i < n_src ? strides[i] : 0;
        gs.ptr[i] = (i < n_src && gsrc) ? (float*)gsrc[i] : nullptr;
        need_src |= gs.ptr[i] != nullptr;
        C += src.ch[i];
    }
    const ScbPlan p = scb_plan(B, H, W, C, F);
    float* w = (float*)ws;
    float *d = w + p.off_d, *gd = w + p.off_gd, *gz = w + p.off_gz, *part_pw = w + p.off_ppw, *part_b = w + p.off_pb,
          *part_dw = w + p.off_pdw;
    const bool act_in = flags & 1, act_out = flags & 2;
    const bool need_gd = need_src || gdw, need_pw = gpw != nullptr, need_b = gbias != nullptr;
    int rc;
    if (act_out || need_pw) {  // stage A: z and grad_pw read d
        const int64_t n_threads = p.n_strips * p.cpad;
        const dim3 grid((unsigned)((n_threads + 255) / 256));
        if (act_in)
            hipLaunchKernelGGL((sepconv_bwd_d_kernel<true>), grid, dim3(256), 0, s, src, (const float*)dw, d, H, W, C,
                               p.cpad, p.wq, n_threads);
        else
            hipLaunchKernelGGL((sepconv_bwd_d_kernel<false>), grid, dim3(256), 0, s, src, (const float*)dw, d, H, W, C,
                               p.cpad, p.wq, n_threads);
        if ((rc = check_launch("sepconv_bwd_d_kernel"))) return rc;
    }
#define QPWC_SCB(FF)                                                                                                   \
    rc = scb_pointwise<FF>(p, d, (const float*)pw, (const float*)bias, (const float*)gout, gz, gd, part_pw, part_b,   \
                           act_out, need_gd, need_pw, need_b, s)
    if (F == 16) QPWC_SCB(16);
    else if (F == 32) QPWC_SCB(32);
    else if (F == 64) QPWC_SCB(64);
    else QPWC_SCB(128);
#undef QPWC_SCB
    if (rc) return rc;
    if (need_gd) {  // stage C
        const dim3 grid((unsigned)p.dw_x, (unsigned)p.chunks);
#define QPWC_SCB_DW(ACT, NEED)                                                                                         \
    hipLaunchKernelGGL((sepconv_bwd_dw_kernel<ACT, NEED>), grid, dim3(256), 0, s, src, gs, (const float*)dw,          \
                       (const float*)gd, part_dw, H, W, C, p.cpad, p.wq, p.n_strips, p.n_groups)
        if (act_in && gdw) QPWC_SCB_DW(true, true);
        else if (act_in) QPWC_SCB_DW(true, false);
        else if (gdw) QPWC_SCB_DW(false, true);
        else QPWC_SCB_DW(false, false);
#undef QPWC_SCB_DW
        if ((rc = check_launch("sepconv_bwd_dw_kernel"))) return rc;
    }
    // stage D
    if (need_pw && (rc = scb_reduce(part_pw, (float*)gpw, (int64_t)F * p.cpad, p.pw_x, p.cpad, C, s))) return rc;
    if (need_b && (rc = scb_reduce(part_b, (float*)gbias, F, p.pw_x, F, F, s))) return rc;
    if (gdw && (rc = scb_reduce(part_dw, (float*)gdw, (int64_t)C * 9, p.dw_x, C * 9, C * 9, s))) return rc;
    return QPWC_OK;
}

}  // namespace qpwc

// Training side of the flow head (the tail of OptFlow.__call__, qpwcnet/core/non_layers.py:238-254, 268-273) and of
// Upsample (non_layers.py:183-193) for gfx950 (MI355X, CDNA4, wave64): the batch statistics of
// BatchNormalization(fused=False) in training mode, the backward of qpwc_flow_head_fwd in both BatchNorm modes, and the
// adjoint of qpwc_upsample2x_flow_fwd.  fp32, channels-last.  Formulas: include/qpwc.h.
//
//   m = Mish(z), a = W1 m + b1, u = Mish(a), h = s u + t, flow = scale conv3x3(h, wf)
//
// Lane roles as in flow_head_kernel (optflow.hip): lane = (pixel n = lane & 15, channel quad g = lane >> 4); the 1x1
// product is v_mfma_f32_16x16x4_f32 with rows = the 16 outputs (A = W1) and columns = 16 pixels, so a lane ends up
// with channels 4g .. 4g+3 of pixel n -- the same four channels whose z it loaded.  The backward's W1^T ga is the same
// instruction with A = W1^T, and lands in that layout again.
//
// Kernels:
//   flow_head_stats_kernel      per workgroup (count, mean as sample + rest, M2) of u per channel: every lane sums (u - c) and (u - c)^2
//                               with c = the first u it sees (a sample, so within the spread of the mean: no
//                               cancellation for |mean| >> std), the 256 lanes' partials are Chan-merged in lane order
//   flow_head_stats_final_kernel  Chan merge of the workgroups in order -> mean, biased var; writes the 592-float
//                               parameter vector of qpwc_flow_head_fwd, the statistics and the moving buffers
//   flow_head_bwd_gh_kernel     pass 1, per 16 x 16 tile: gh as a gather of g through the transposed taps; partials of
//                               sum gh, sum gh xh and grad_wf (as sum_q h[q] g[q - k + 1]: no halo of h is needed)
//   flow_head_bwd_z_kernel      pass 2: gh again, gu, ga = gu Mish'(a), grad_z = (W1^T ga) Mish'(z); partials of
//                               grad_w1 = ga^T m (matrix instruction, K = the pixels, operands transposed through LDS)
//                               and grad_b1
//   flow_head_bwd_reduce_kernel the workgroups' partials summed in workgroup order
//   upsample2x_flow_bwd_kernel  one thread per input pixel: 4 x 4 taps of grad_out, separable weights
//
// Determinism: grids depend on the shape only; a workgroup walks its tiles in grid-stride order; lanes are folded by
// xor shuffles (a + b = b + a: every lane holds the same bits), waves 0..3 in order, workgroups in order.  No
// atomics.  What is asked for is a kernel ARGUMENT, not a template parameter: one instantiation computes every
// subset, so an output's bits do not depend on its neighbours.  Contraction is off in the kernels (every fused
// multiply-add is written out) so that gh is the same bits in both passes.
#include "optflow_common.h"
#include "launch.h"

namespace qpwc {

constexpr int kFhbC = 16;
constexpr int kFhbTile = 16;          // pixels per tile edge, as flow_head_kernel
constexpr int kFhbTW = kFhbTile + 2;  // with the one-pixel halo of g
constexpr int kFhbTileBlocks = 512;   // workgroups of the two backward passes (each walks its tiles in grid-stride order)
constexpr int kFhbStatBlocks = 256;   // workgroups of flow_head_stats_kernel: 4 waves x 16 pixels per trip each
constexpr int kFhbUpBlocks = 256;     // workgroups of upsample2x_flow_bwd_kernel, 256 input pixels per trip each
constexpr int kFhbN1 = 32 + 288;      // pass 1 sums: sum gh | sum gh xh | grad_wf
constexpr int kFhbN2 = 256 + 16;      // pass 2 sums: grad_w1 | grad_b1

// a (+ b1) for channels 4g .. 4g+3 of this lane's pixel from m = Mish(z) of the same channels; w1v = W1[n][4g .. 4g+3]
__device__ __forceinline__ f32x4v fhb_w1m(const f32x4v w1v, const float4 m) {
    f32x4v d = {0.f, 0.f, 0.f, 0.f};
    d = __builtin_amdgcn_mfma_f32_16x16x4f32(w1v[0], m.x, d, 0, 0, 0);
    d = __builtin_amdgcn_mfma_f32_16x16x4f32(w1v[1], m.y, d, 0, 0, 0);
    d = __builtin_amdgcn_mfma_f32_16x16x4f32(w1v[2], m.z, d, 0, 0, 0);
    d = __builtin_amdgcn_mfma_f32_16x16x4f32(w1v[3], m.w, d, 0, 0, 0);
    return d;
}

// ---- batch statistics -------------------------------------------------------------------------------------------------
// count, mean = c + d and M2 of a set: c is one of its samples (an exact fp32 value), d the small rest, so the mean is
// known to a fraction of the SPREAD, not of its own size -- x^ = (u - mean) rstd then sums to zero over the batch as
// the backward's formulas assume (with one fp32 mean near 8 it misses by M ulp(8) rstd)
struct FhbMoment {
    float n, c, d, m2;
};

// Chan et al.: the moments of the union of two sets; an empty side changes nothing
__device__ __forceinline__ FhbMoment fhb_merge(const FhbMoment a, const FhbMoment b) {
#pragma clang fp contract(off)
    if (b.n == 0.0f) return a;
    if (a.n == 0.0f) return b;
    FhbMoment r;
    r.n = a.n + b.n;
    const float delta = (b.c - a.c) + (b.d - a.d), f = b.n / r.n;
    r.c = a.c;
    r.d = a.d + delta * f;
    r.m2 = a.m2 + b.m2 + (delta * delta) * (a.n * f);
    return r;
}

__global__ __launch_bounds__(256) void flow_head_stats_kernel(const float* __restrict__ z, const float* __restrict__ w1,
                                                              const float* __restrict__ b1, float* __restrict__ part,
                                                              int64_t M, int64_t n_groups) {
#pragma clang fp contract(off)
    __shared__ float red[256 * 4 * 4];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, n = lane & 15, g = lane >> 4;
    const f32x4v w1v = *reinterpret_cast<const f32x4v*>(w1 + n * kFhbC + 4 * g);
    const float4 b1v = *reinterpret_cast<const float4*>(b1 + 4 * g);
    float shift[4] = {0.f, 0.f, 0.f, 0.f}, s1[4] = {0.f, 0.f, 0.f, 0.f}, s2[4] = {0.f, 0.f, 0.f, 0.f};
    float cnt = 0.0f;
    const int64_t first = (int64_t)blockIdx.x * 4 + wave, step = (int64_t)gridDim.x * 4;
    for (int64_t q = first; q < n_groups; q += step) {  // wave-uniform: the matrix instruction runs with every lane
        const int64_t p = q * 16 + n;
        const bool ok = p < M;
        float4 zv = make_float4(0.f, 0.f, 0.f, 0.f);
        if (ok) zv = ldg_f4(z + p * kFhbC + 4 * g);
        const f32x4v d = fhb_w1m(w1v, make_float4(mishf(zv.x), mishf(zv.y), mishf(zv.z), mishf(zv.w)));
        const float u[4] = {mishf(d[0] + b1v.x), mishf(d[1] + b1v.y), mishf(d[2] + b1v.z), mishf(d[3] + b1v.w)};
        if (ok) {
            // pixels only run out at the end, so a lane's first trip is its first sample
            if (q == first) {
#pragma unroll
                for (int j = 0; j < 4; ++j) shift[j] = u[j];
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const float e = u[j] - shift[j];
                s1[j] += e;
                s2[j] = fmaf(e, e, s2[j]);
            }
            cnt += 1.0f;
        }
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        float* r = red + ((wave * 16 + n) * kFhbC + 4 * g + j) * 4;  // [wave][n][channel]
        const float mu = cnt > 0.0f ? s1[j] / cnt : 0.0f;
        r[0] = cnt;
        r[1] = shift[j];
        r[2] = mu;
        r[3] = cnt > 0.0f ? fmaxf(s2[j] - s1[j] * mu, 0.0f) : 0.0f;
    }
    __syncthreads();
    if (tid < kFhbC) {
        FhbMoment acc = {0.f, 0.f, 0.f, 0.f};
        for (int i = 0; i < 64; ++i) {
            const float* r = red + (i * kFhbC + tid) * 4;
            acc = fhb_merge(acc, FhbMoment{r[0], r[1], r[2], r[3]});
        }
        float* o = part + ((int64_t)blockIdx.x * kFhbC + tid) * 4;
        o[0] = acc.n;
        o[1] = acc.c;
        o[2] = acc.d;
        o[3] = acc.m2;
    }
}

__global__ __launch_bounds__(64) void flow_head_stats_final_kernel(
    const float* __restrict__ part, int n_part, const float* __restrict__ w1, const float* __restrict__ b1,
    const float* __restrict__ gamma, const float* __restrict__ beta, const float* __restrict__ wf,
    float* __restrict__ moving_mean, float* __restrict__ moving_var, float momentum, float eps,
    float* __restrict__ params, float* __restrict__ stats) {
#pragma clang fp contract(off)
    const int tid = threadIdx.x;
    for (int i = tid; i < 256; i += 64) params[i] = w1[i];
    for (int i = tid; i < 288; i += 64) params[304 + i] = wf[i];
    if (tid >= kFhbC) return;
    FhbMoment acc = {0.f, 0.f, 0.f, 0.f};
    for (int p = 0; p < n_part; ++p) {
        const float* r = part + ((int64_t)p * kFhbC + tid) * 4;
        acc = fhb_merge(acc, FhbMoment{r[0], r[1], r[2], r[3]});
    }
    const float mean = acc.c + acc.d, var = acc.m2 / acc.n;
    const float s = gamma[tid] / sqrtf(var + eps);
    params[256 + tid] = b1[tid];
    params[272 + tid] = s;
    params[288 + tid] = beta[tid] - mean * s;
    if (stats) {
        stats[tid] = mean;
        stats[kFhbC + tid] = var;
        stats[2 * kFhbC + tid] = (acc.c - mean) + acc.d;  // what the rounding of mean dropped (c - mean is exact)
    }
    if (moving_mean) {
        moving_mean[tid] = moving_mean[tid] * momentum + mean * (1.0f - momentum);
        moving_var[tid] = moving_var[tid] * momentum + var * (1.0f - momentum);
    }
}

// ---- what both backward passes share ----------------------------------------------------------------------------------
struct FhbTile {
    int b, y0, x0;
};
__device__ __forceinline__ FhbTile fhb_tile(int64_t t, int tiles_x, int tiles_y) {
    FhbTile r;
    r.x0 = (int)(t % tiles_x) * kFhbTile;
    r.y0 = (int)((t / tiles_x) % tiles_y) * kFhbTile;
    r.b = (int)(t / ((int64_t)tiles_x * tiles_y));
    return r;
}

// g of the tile and its one-pixel halo into LDS, zero outside the image
__device__ __forceinline__ void fhb_load_g(const float* __restrict__ g, float2* gs, const FhbTile t, int H, int W,
                                           int tid) {
    for (int i = tid; i < kFhbTW * kFhbTW; i += 256) {
        const int ly = i / kFhbTW, lx = i - ly * kFhbTW;
        const int gy = t.y0 - 1 + ly, gx = t.x0 - 1 + lx;
        float2 v = make_float2(0.f, 0.f);
        if (gy >= 0 && gy < H && gx >= 0 && gx < W) {
            const float* q = g + (((int64_t)t.b * H + gy) * W + gx) * 2;
            v = make_float2(ldg_f1(q), ldg_f1(q + 1));
        }
        gs[i] = v;
    }
}

// the 72 weights of this lane's 4 channels, wf[ky][kx][in][out]: [k][0] = (c0:x,y c1:x,y), [k][1] = (c2:x,y c3:x,y)
__device__ __forceinline__ void fhb_load_wf(const float* __restrict__ wf, int g, float4 (&wq)[9][2]) {
#pragma unroll
    for (int k = 0; k < 9; ++k) {
        wq[k][0] = *reinterpret_cast<const float4*>(wf + k * kFhbC * 2 + 8 * g);
        wq[k][1] = *reinterpret_cast<const float4*>(wf + k * kFhbC * 2 + 8 * g + 4);
    }
}

// gh[j] = scale sum_k sum_o wf[k][4g+j][o] g[p - k + 1][o] for the pixel at tile row ry, column n
__device__ __forceinline__ void fhb_gh(const float2* gs, const float4 (&wq)[9][2], int ry, int n, float scale,
                                       float (&gh)[4]) {
#pragma clang fp contract(off)
    float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
#pragma unroll
    for (int ky = 0; ky < 3; ++ky)
#pragma unroll
        for (int kx = 0; kx < 3; ++kx) {
            const float2 gv = gs[(ry + 2 - ky) * kFhbTW + n + 2 - kx];
            const float4 wa = wq[ky * 3 + kx][0], wb = wq[ky * 3 + kx][1];
            a0 = fmaf(wa.y, gv.y, fmaf(wa.x, gv.x, a0));
            a1 = fmaf(wa.w, gv.y, fmaf(wa.z, gv.x, a1));
            a2 = fmaf(wb.y, gv.y, fmaf(wb.x, gv.x, a2));
            a3 = fmaf(wb.w, gv.y, fmaf(wb.z, gv.x, a3));
        }
    gh[0] = scale * a0;
    gh[1] = scale * a1;
    gh[2] = scale * a2;
    gh[3] = scale * a3;
}

// sum over the 16 pixel lanes of a channel quad: every lane ends with the same bits
__device__ __forceinline__ float fhb_fold16(float v) {
    v += __shfl_xor(v, 1);
    v += __shfl_xor(v, 2);
    v += __shfl_xor(v, 4);
    v += __shfl_xor(v, 8);
    return v;
}

// ---- pass 1: sum gh, sum gh xh, grad_wf ----------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void flow_head_bwd_gh_kernel(const float* __restrict__ z,
                                                               const float* __restrict__ params,
                                                               const float* __restrict__ stats, float eps,
                                                               const float* __restrict__ g, float* __restrict__ part,
                                                               int H, int W, int tiles_x, int tiles_y, int64_t n_tiles,
                                                               float scale, int need_wf) {
#pragma clang fp contract(off)
    __shared__ float2 gs[kFhbTW * kFhbTW];
    __shared__ float red[4 * kFhbN1];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, n = lane & 15, q = lane >> 4;
    const f32x4v w1v = *reinterpret_cast<const f32x4v*>(params + n * kFhbC + 4 * q);
    const float4 b1v = *reinterpret_cast<const float4*>(params + 256 + 4 * q);
    const float4 bsv = *reinterpret_cast<const float4*>(params + 272 + 4 * q);
    const float4 btv = *reinterpret_cast<const float4*>(params + 288 + 4 * q);
    const float4 mu = *reinterpret_cast<const float4*>(stats + 4 * q);
    const float4 var = *reinterpret_cast<const float4*>(stats + kFhbC + 4 * q);
    const float rstd[4] = {1.0f / sqrtf(var.x + eps), 1.0f / sqrtf(var.y + eps), 1.0f / sqrtf(var.z + eps),
                           1.0f / sqrtf(var.w + eps)};
    const float mean[4] = {mu.x, mu.y, mu.z, mu.w};
    const float4 lov = *reinterpret_cast<const float4*>(stats + 2 * kFhbC + 4 * q);
    const float lo[4] = {lov.x, lov.y, lov.z, lov.w};
    const float b1a[4] = {b1v.x, b1v.y, b1v.z, b1v.w}, bs[4] = {bsv.x, bsv.y, bsv.z, bsv.w},
                bt[4] = {btv.x, btv.y, btv.z, btv.w};
    float4 wq[9][2];
    fhb_load_wf(params + 304, q, wq);
    float sgh[4] = {0.f, 0.f, 0.f, 0.f}, sgx[4] = {0.f, 0.f, 0.f, 0.f};
    float gw[9][4][2];
#pragma unroll
    for (int k = 0; k < 9; ++k)
#pragma unroll
        for (int j = 0; j < 4; ++j) gw[k][j][0] = gw[k][j][1] = 0.0f;
    for (int64_t t = blockIdx.x; t < n_tiles; t += gridDim.x) {
        const FhbTile tl = fhb_tile(t, tiles_x, tiles_y);
        __syncthreads();  // the previous tile's g is read
        fhb_load_g(g, gs, tl, H, W, tid);
        __syncthreads();
        for (int ry = wave; ry < kFhbTile; ry += 4) {
            const int gy = tl.y0 + ry, gx = tl.x0 + n;
            const bool inb = gy < H && gx < W;
            float4 zv = make_float4(0.f, 0.f, 0.f, 0.f);
            if (inb) zv = ldg_f4(z + (((int64_t)tl.b * H + gy) * W + gx) * kFhbC + 4 * q);
            const f32x4v d = fhb_w1m(w1v, make_float4(mishf(zv.x), mishf(zv.y), mishf(zv.z), mishf(zv.w)));
            float gh[4];
            fhb_gh(gs, wq, ry, n, scale, gh);
            float h[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const float u = mishf(d[j] + b1a[j]);
                const float xh = ((u - mean[j]) - lo[j]) * rstd[j];
                h[j] = inb ? fmaf(u, bs[j], bt[j]) : 0.0f;
                const float ghj = inb ? gh[j] : 0.0f;
                sgh[j] += ghj;
                sgx[j] = fmaf(ghj, xh, sgx[j]);
            }
            if (need_wf) {
#pragma unroll
                for (int ky = 0; ky < 3; ++ky)
#pragma unroll
                    for (int kx = 0; kx < 3; ++kx) {
                        const float2 gv = gs[(ry + 2 - ky) * kFhbTW + n + 2 - kx];
#pragma unroll
                        for (int j = 0; j < 4; ++j) {
                            gw[ky * 3 + kx][j][0] = fmaf(h[j], gv.x, gw[ky * 3 + kx][j][0]);
                            gw[ky * 3 + kx][j][1] = fmaf(h[j], gv.y, gw[ky * 3 + kx][j][1]);
                        }
                    }
            }
        }
    }
    // lanes of a quad folded by shuffles, then the four waves in order
    float* r = red + wave * kFhbN1;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const float a = fhb_fold16(sgh[j]), b = fhb_fold16(sgx[j]);
        if (n == 0) {
            r[4 * q + j] = a;
            r[kFhbC + 4 * q + j] = b;
        }
    }
#pragma unroll
    for (int k = 0; k < 9; ++k)
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int o = 0; o < 2; ++o) {
                const float a = fhb_fold16(gw[k][j][o]);
                if (n == 0) r[32 + (k * kFhbC + 4 * q + j) * 2 + o] = scale * a;
            }
    __syncthreads();
    for (int i = tid; i < kFhbN1; i += 256)
        part[(int64_t)blockIdx.x * kFhbN1 + i] = ((red[i] + red[kFhbN1 + i]) + red[2 * kFhbN1 + i]) + red[3 * kFhbN1 + i];
}

// ---- pass 2: grad_z, partials of grad_w1 and grad_b1 ----------------------------------------------------------------------
// sums: the reduced pass-1 sums (sum gh | sum gh xh), read in training mode only
__global__ __launch_bounds__(256) void flow_head_bwd_z_kernel(const float* __restrict__ z,
                                                              const float* __restrict__ params,
                                                              const float* __restrict__ stats, float eps,
                                                              const float* __restrict__ g,
                                                              const float* __restrict__ sums, float inv_m,
                                                              float* __restrict__ grad_z, float* __restrict__ part,
                                                              int H, int W, int tiles_x, int tiles_y, int64_t n_tiles,
                                                              float scale, int training, int need_w) {
#pragma clang fp contract(off)
    constexpr int LD = kFhbC + 4;  // 16-byte rows, 4 banks apart
    __shared__ float2 gs[kFhbTW * kFhbTW];
    __shared__ __attribute__((aligned(16))) float ga_s[4][16 * LD];
    __shared__ __attribute__((aligned(16))) float m_s[4][16 * LD];
    __shared__ float red[4 * kFhbN2];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, n = lane & 15, q = lane >> 4;
    const f32x4v w1v = *reinterpret_cast<const f32x4v*>(params + n * kFhbC + 4 * q);
    // W1^T as the A operand: row = input channel n, k = output 4q + s
    const float w1t[4] = {params[(4 * q + 0) * kFhbC + n], params[(4 * q + 1) * kFhbC + n],
                          params[(4 * q + 2) * kFhbC + n], params[(4 * q + 3) * kFhbC + n]};
    const float4 b1v = *reinterpret_cast<const float4*>(params + 256 + 4 * q);
    const float4 bsv = *reinterpret_cast<const float4*>(params + 272 + 4 * q);
    const float4 mu = *reinterpret_cast<const float4*>(stats + 4 * q);
    const float4 var = *reinterpret_cast<const float4*>(stats + kFhbC + 4 * q);
    const float rstd[4] = {1.0f / sqrtf(var.x + eps), 1.0f / sqrtf(var.y + eps), 1.0f / sqrtf(var.z + eps),
                           1.0f / sqrtf(var.w + eps)};
    const float mean[4] = {mu.x, mu.y, mu.z, mu.w};
    const float4 lov = *reinterpret_cast<const float4*>(stats + 2 * kFhbC + 4 * q);
    const float lo[4] = {lov.x, lov.y, lov.z, lov.w};
    const float b1a[4] = {b1v.x, b1v.y, b1v.z, b1v.w}, bs[4] = {bsv.x, bsv.y, bsv.z, bsv.w};
    float mgh[4] = {0.f, 0.f, 0.f, 0.f}, mgx[4] = {0.f, 0.f, 0.f, 0.f};  // sum gh / M, sum gh xh / M
    if (training) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            mgh[j] = sums[4 * q + j] * inv_m;
            mgx[j] = sums[kFhbC + 4 * q + j] * inv_m;
        }
    }
    float4 wq[9][2];
    fhb_load_wf(params + 304, q, wq);
    f32x4v accw = {0.f, 0.f, 0.f, 0.f};  // grad_w1[4 (lane >> 4) + r][lane & 15]
    float sb[4] = {0.f, 0.f, 0.f, 0.f};
    for (int64_t t = blockIdx.x; t < n_tiles; t += gridDim.x) {
        const FhbTile tl = fhb_tile(t, tiles_x, tiles_y);
        __syncthreads();
        fhb_load_g(g, gs, tl, H, W, tid);
        __syncthreads();
        for (int ry = wave; ry < kFhbTile; ry += 4) {  // four trips in every wave: the barriers below are uniform
            const int gy = tl.y0 + ry, gx = tl.x0 + n;
            const bool inb = gy < H && gx < W;
            const int64_t off = (((int64_t)tl.b * H + gy) * W + gx) * kFhbC + 4 * q;
            float4 zv = make_float4(0.f, 0.f, 0.f, 0.f);
            if (inb) zv = ldg_f4(z + off);
            const float4 m = make_float4(mishf(zv.x), mishf(zv.y), mishf(zv.z), mishf(zv.w));
            const f32x4v d = fhb_w1m(w1v, m);
            float gh[4], ga[4];
            fhb_gh(gs, wq, ry, n, scale, gh);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const float a = d[j] + b1a[j];
                float gu = gh[j];
                if (training) {
                    const float xh = ((mishf(a) - mean[j]) - lo[j]) * rstd[j];
                    gu = (gh[j] - mgh[j]) - xh * mgx[j];
                }
                const float sgu = inb ? bs[j] * gu : 0.0f;
                ga[j] = sgu * mish_grad(a);
                // batch statistics: sum_p gu = 0 by construction, so grad_b1 = sum_p s gu (Mish'(a) - 1), which does not
                // round M terms that cancel (for a near 8 Mish' - 1 is 1e-6: the terms' rounding exceeds their sum)
                sb[j] += training ? sgu * mish_grad_m1(a) : ga[j];
            }
            if (grad_z) {
                f32x4v e = {0.f, 0.f, 0.f, 0.f};
                e = __builtin_amdgcn_mfma_f32_16x16x4f32(w1t[0], ga[0], e, 0, 0, 0);
                e = __builtin_amdgcn_mfma_f32_16x16x4f32(w1t[1], ga[1], e, 0, 0, 0);
                e = __builtin_amdgcn_mfma_f32_16x16x4f32(w1t[2], ga[2], e, 0, 0, 0);
                e = __builtin_amdgcn_mfma_f32_16x16x4f32(w1t[3], ga[3], e, 0, 0, 0);
                if (inb)
                    *reinterpret_cast<float4*>(grad_z + off) =
                        make_float4(e[0] * mish_grad(zv.x), e[1] * mish_grad(zv.y), e[2] * mish_grad(zv.z),
                                    e[3] * mish_grad(zv.w));
            }
            if (need_w) {
                // grad_w1 += ga^T m over this wave's 16 pixels: K = pixel, so both operands go through LDS transposed
                __syncthreads();  // the previous row's fragments are read
                *reinterpret_cast<float4*>(&ga_s[wave][n * LD + 4 * q]) = make_float4(ga[0], ga[1], ga[2], ga[3]);
                *reinterpret_cast<float4*>(&m_s[wave][n * LD + 4 * q]) = m;
                __syncthreads();
#pragma unroll
                for (int k = 0; k < 16; k += 4)
                    accw = __builtin_amdgcn_mfma_f32_16x16x4f32(ga_s[wave][(k + q) * LD + n], m_s[wave][(k + q) * LD + n],
                                                                accw, 0, 0, 0);
            }
        }
    }
    float* r = red + wave * kFhbN2;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        r[(4 * q + j) * kFhbC + n] = accw[j];
        const float a = fhb_fold16(sb[j]);
        if (n == 0) r[256 + 4 * q + j] = a;
    }
    __syncthreads();
    for (int i = tid; i < kFhbN2; i += 256)
        part[(int64_t)blockIdx.x * kFhbN2 + i] = ((red[i] + red[kFhbN2 + i]) + red[2 * kFhbN2 + i]) + red[3 * kFhbN2 + i];
}

// ---- the partials of the workgroups, summed in workgroup order; up to three destinations take a slice each ---------------
struct FhbDst {
    float* ptr[3];
    int begin[3], end[3];
};
__global__ __launch_bounds__(64) void flow_head_bwd_reduce_kernel(const float* __restrict__ part, int n_part, int n_out,
                                                                  float* __restrict__ sums, FhbDst dst) {
#pragma clang fp contract(off)
    const int i = blockIdx.x * 64 + threadIdx.x;
    if (i >= n_out) return;
    float s = 0.0f;
#pragma unroll 8
    for (int p = 0; p < n_part; ++p) s += ldg_f1(part + (int64_t)p * n_out + i);
    if (sums) sums[i] = s;
#pragma unroll
    for (int k = 0; k < 3; ++k)
        if (dst.ptr[k] && i >= dst.begin[k] && i < dst.end[k]) dst.ptr[k][i - dst.begin[k]] = s;
}

// ---- adjoint of the x2 bilinear upsampling ------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void upsample2x_flow_bwd_kernel(const float* __restrict__ g, float* __restrict__ out,
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
        const float* gb = g + b * H2 * W2 * 2;
        float ax = 0.0f, ay = 0.0f;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            float rx = 0.0f, ry = 0.0f;
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                const float* p = gb + ((int64_t)ys[r] * W2 + xs[c]) * 2;
                rx = fmaf(wt[c], ldg_f1(p), rx);
                ry = fmaf(wt[c], ldg_f1(p + 1), ry);
            }
            ax = fmaf(wt[r], rx, ax);
            ay = fmaf(wt[r], ry, ay);
        }
        *reinterpret_cast<float2*>(out + idx * 2) = make_float2(scale * ax, scale * ay);
    }
}

// ---- host side --------------------------------------------------------------------------------------------------------------
struct FhbPlan {
    int64_t M, n_tiles, n_groups;
    int tiles_x, tiles_y, blocks, stat_blocks;
    int64_t off_p1, off_sums, off_p2, total;  // backward workspace offsets, in floats, 16-byte aligned
};

static FhbPlan fhb_plan(int B, int H, int W) {
    FhbPlan p;
    p.M = (int64_t)B * H * W;
    p.tiles_x = (W + kFhbTile - 1) / kFhbTile;
    p.tiles_y = (H + kFhbTile - 1) / kFhbTile;
    p.n_tiles = (int64_t)B * p.tiles_x * p.tiles_y;
    p.blocks = (int)(p.n_tiles < kFhbTileBlocks ? p.n_tiles : kFhbTileBlocks);
    p.n_groups = (p.M + 15) / 16;
    const int64_t want = (p.n_groups + 3) / 4;
    p.stat_blocks = (int)(want < kFhbStatBlocks ? want : kFhbStatBlocks);
    p.off_p1 = 0;
    p.off_sums = p.off_p1 + (int64_t)p.blocks * kFhbN1;
    p.off_p2 = p.off_sums + kFhbN1;
    p.total = p.off_p2 + (int64_t)p.blocks * kFhbN2;
    return p;
}

int64_t flow_head_stats_workspace_floats(int B, int H, int W) { return (int64_t)fhb_plan(B, H, W).stat_blocks * kFhbC * 4; }
int64_t flow_head_bwd_workspace_floats(int B, int H, int W) { return fhb_plan(B, H, W).total; }

int flow_head_stats_launch(const void* z, const void* w1, const void* b1, const void* gamma, const void* beta,
                           const void* wf, void* moving_mean, void* moving_var, float momentum, float eps, void* params,
                           void* stats, void* ws, int B, int H, int W, hipStream_t s) {
    const FhbPlan p = fhb_plan(B, H, W);
    hipLaunchKernelGGL(flow_head_stats_kernel, dim3((unsigned)p.stat_blocks), dim3(256), 0, s, (const float*)z,
                       (const float*)w1, (const float*)b1, (float*)ws, p.M, p.n_groups);
    int rc = check_launch("flow_head_stats_kernel");
    if (rc) return rc;
    hipLaunchKernelGGL(flow_head_stats_final_kernel, dim3(1), dim3(64), 0, s, (const float*)ws, p.stat_blocks,
                       (const float*)w1, (const float*)b1, (const float*)gamma, (const float*)beta, (const float*)wf,
                       (float*)moving_mean, (float*)moving_var, momentum, eps, (float*)params, (float*)stats);
    return check_launch("flow_head_stats_final_kernel");
}

int flow_head_bwd_launch(const void* z, const void* params, const void* stats, float eps, int training, float scale,
                         const void* gout, void* gz, void* gw1, void* gb1, void* ggamma, void* gbeta, void* gwf,
                         void* ws, int B, int H, int W, hipStream_t s) {
    const FhbPlan p = fhb_plan(B, H, W);
    float* w = (float*)ws;
    float *part1 = w + p.off_p1, *sums = w + p.off_sums, *part2 = w + p.off_p2;
    const bool pass2 = gz || gw1 || gb1;
    const bool pass1 = ggamma || gbeta || gwf || (training && pass2);
    int rc;
    if (pass1) {
        hipLaunchKernelGGL(flow_head_bwd_gh_kernel, dim3((unsigned)p.blocks), dim3(256), 0, s, (const float*)z,
                           (const float*)params, (const float*)stats, eps, (const float*)gout, part1, H, W, p.tiles_x,
                           p.tiles_y, p.n_tiles, scale, gwf ? 1 : 0);
        if ((rc = check_launch("flow_head_bwd_gh_kernel"))) return rc;
        FhbDst d;
        d.ptr[0] = (float*)gbeta, d.begin[0] = 0, d.end[0] = kFhbC;
        d.ptr[1] = (float*)ggamma, d.begin[1] = kFhbC, d.end[1] = 2 * kFhbC;
        d.ptr[2] = (float*)gwf, d.begin[2] = 2 * kFhbC, d.end[2] = kFhbN1;
        hipLaunchKernelGGL(flow_head_bwd_reduce_kernel, dim3((kFhbN1 + 63) / 64), dim3(64), 0, s, (const float*)part1,
                           p.blocks, kFhbN1, sums, d);
        if ((rc = check_launch("flow_head_bwd_reduce_kernel"))) return rc;
    }
    if (pass2) {
        hipLaunchKernelGGL(flow_head_bwd_z_kernel, dim3((unsigned)p.blocks), dim3(256), 0, s, (const float*)z,
                           (const float*)params, (const float*)stats, eps, (const float*)gout, (const float*)sums,
                           1.0f / (float)p.M, (float*)gz, part2, H, W, p.tiles_x, p.tiles_y, p.n_tiles, scale,
                           training ? 1 : 0, gw1 ? 1 : 0);
        if ((rc = check_launch("flow_head_bwd_z_kernel"))) return rc;
        if (gw1 || gb1) {
            FhbDst d;
            d.ptr[0] = (float*)gw1, d.begin[0] = 0, d.end[0] = 256;
            d.ptr[1] = (float*)gb1, d.begin[1] = 256, d.end[1] = kFhbN2;
            d.ptr[2] = nullptr, d.begin[2] = d.end[2] = 0;
            hipLaunchKernelGGL(flow_head_bwd_reduce_kernel, dim3((kFhbN2 + 63) / 64), dim3(64), 0, s,
                               (const float*)part2, p.blocks, kFhbN2, (float*)nullptr, d);
            if ((rc = check_launch("flow_head_bwd_reduce_kernel"))) return rc;
        }
    }
    return QPWC_OK;
}

int upsample2x_flow_bwd_launch(const void* gout, void* gin, int B, int h, int w, float scale, hipStream_t s) {
    const int64_t n = (int64_t)B * h * w, want = (n + 255) / 256;
    hipLaunchKernelGGL(upsample2x_flow_bwd_kernel, dim3((unsigned)(want < kFhbUpBlocks ? want : kFhbUpBlocks)),
                       dim3(256), 0, s, (const float*)gout, (float*)gin, n, h, w, scale);
    return check_launch("upsample2x_flow_bwd_kernel");
}

}  // namespace qpwc

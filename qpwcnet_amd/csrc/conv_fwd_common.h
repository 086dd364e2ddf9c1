// Shared by the forward convolution translation units of the encoder and decoder (encoder.hip: fp32 and fp16 storage,
// encoder_x3.hip: bf16x3): the activation, the 16-pixel-wide tile and its halo, the LDS layout of 2-byte pixels, the
// halo staging of the stride-1 and transposed kernels, the epilogue pieces and the launchers' tile plan.
//
// Every kernel works on tiles of TH x 16 pixels with 256 threads; lane l of a wave is pixel n = l & 15 of a tile row
// and k-slot / output quad g = l >> 4 of the 16x16 matrix instructions, so an accumulator holds outputs 4g .. 4g + 3 of
// pixel n.  Everything here is inlined into kernels whose template arguments make its parameters constants.
#pragma once
#include "common.h"
#include "launch.h"
#include "split_bf16.h"

namespace qpwc {

// Mish with v_exp_f32 / v_rcp_f32 directly: hipcc lowers __expf with denormal range handling and __fdividef to the
// full IEEE division sequence (div_scale / div_fmas / div_fixup), ~28 instructions per value.
// (optflow_common.h's mishf is the same formula compiled with fp contract(off); the two are not interchangeable.)
__device__ __forceinline__ float conv_mishf(float x) {
    const float e = __builtin_amdgcn_exp2f(fminf(x, 20.0f) * 1.4426950408889634f);
    const float t = e * (e + 2.0f);
    const float m = x * (t * __builtin_amdgcn_rcpf(t + 2.0f));
    return m;   // x > 20: e is clamped, t / (t + 2) rounds to 1 +- 1 ulp, m = x to 2 ulp -- no compare + select per value
}

typedef float f32x4e __attribute__((ext_vector_type(4)));
typedef _Float16 f16x8e __attribute__((ext_vector_type(8)));
typedef _Float16 f16x4e __attribute__((ext_vector_type(4)));

// tile width and halo row of every kernel of both files (encoder.hip checks its own kEcTW / kEcHW against them)
constexpr int kCfTW = 16, kCfHW = kCfTW + 2;

// LDS slot of 16-byte chunk q of pixel hp in an image whose pixels are CP 2-byte elements (32 / 64 / 128 / 256 / 512
// bytes): the sixteen consecutive pixels one matrix operand read covers, one chunk each, must spread over the 16
// sixteen-byte slots of the 64 banks
template <int CP>
__device__ __forceinline__ int px16_slot(int q, int hp) {
    return CP == 16 ? (q ^ ((hp >> 3) & 1)) : (CP == 32 ? (q ^ ((0 - (hp >> 2)) & 3)) : (CP == 64 ? (q ^ ((hp >> 1) & 7)) : (q ^ (hp & 15))));
}

// Stage the (TH + 2) x 18 halo tile of the TH x 16 tile at (Y0, X0) with all C channels of an fp16 image (zero outside
// it) as pixels of C halves, px16_slot layout: all global loads first, then the LDS writes
template <int C, int TH>
__device__ __forceinline__ void stage_halo_f16(const __half* __restrict__ xb, __half* in_s, int tid, int Y0, int X0,
                                               int H, int W) {
    constexpr int NQ = C / 8, NH = (TH + 2) * kCfHW;
    constexpr int NST = (NH * NQ + 255) / 256;
    uint4 st[NST];
#pragma unroll
    for (int it = 0; it < NST; ++it) {
        const int idx = tid + 256 * it;
        const int hp = idx / NQ, q = idx - hp * NQ;
        const int hy = hp / kCfHW, hx = hp - hy * kCfHW;
        const int gy = Y0 - 1 + hy, gx = X0 - 1 + hx;
        st[it] = (idx < NH * NQ && gy >= 0 && gy < H && gx >= 0 && gx < W)
                     ? *reinterpret_cast<const uint4*>(xb + ((int64_t)gy * W + gx) * C + 8 * q)
                     : make_uint4(0u, 0u, 0u, 0u);
    }
#pragma unroll
    for (int it = 0; it < NST; ++it) {
        const int idx = tid + 256 * it;
        const int hp = idx / NQ, q = idx - hp * NQ;
        if (idx < NH * NQ) *reinterpret_cast<uint4*>(in_s + hp * C + 8 * px16_slot<C>(q, hp)) = st[it];
    }
}

// The same tile of an fp32 image as three bf16 images, split while it is staged (split_bf16.h).  s1 = image 1; images
// 2 and 3 follow at PL = (TH + 2) * 18 * C halves each.
template <int C, int TH>
__device__ __forceinline__ void x3_stage_tile(const float* __restrict__ xb, unsigned short* s1, int tid, int Y0, int X0,
                                              int H, int W) {
    constexpr int NQ = C / 8, NH = (TH + 2) * kCfHW, PL = NH * C;
    constexpr int NST = (NH * NQ + 255) / 256;
    float4 st[NST][2];
#pragma unroll
    for (int it = 0; it < NST; ++it) {
        const int idx = tid + 256 * it;
        const int hp = idx / NQ, q = idx - hp * NQ;
        const int hy = hp / kCfHW, hx = hp - hy * kCfHW;
        const int gy = Y0 - 1 + hy, gx = X0 - 1 + hx;
        const bool ok = idx < NH * NQ && gy >= 0 && gy < H && gx >= 0 && gx < W;
        const float* p = xb + ((int64_t)gy * W + gx) * C + 8 * q;
        st[it][0] = ok ? *reinterpret_cast<const float4*>(p) : make_float4(0.f, 0.f, 0.f, 0.f);
        st[it][1] = ok ? *reinterpret_cast<const float4*>(p + 4) : make_float4(0.f, 0.f, 0.f, 0.f);
    }
#pragma unroll
    for (int it = 0; it < NST; ++it) {
        const int idx = tid + 256 * it;
        const int hp = idx / NQ, q = idx - hp * NQ;
        if (idx < NH * NQ) {
            uint4 p1, p2, p3;
            split8_bf16x3(st[it][0], st[it][1], p1, p2, p3);
            unsigned short* d = s1 + hp * C + 8 * px16_slot<C>(q, hp);
            *reinterpret_cast<uint4*>(d) = p1;
            *reinterpret_cast<uint4*>(d + PL) = p2;
            *reinterpret_cast<uint4*>(d + 2 * PL) = p3;
        }
    }
}

// Zero border of the padded (H + pad_h) x (W + pad_w) output image ob of C-channel pixels (columns W.., rows H..) --
// the 'SAME' padding the following stride-2 convolution reads -- for the NQ 16-byte chunks of every pixel from channel
// c0 on (a workgroup's slice of the outputs), written by the edge tiles of a TH x 16 tiling
template <typename T, int TH, int NQ>
__device__ __forceinline__ void zero_border(T* ob, int tid, int Y0, int X0, int H, int W, int pad_h, int pad_w, int C,
                                            int c0) {
    constexpr int EPC = 16 / (int)sizeof(T);   // elements per chunk
    const int Wo = W + pad_w;
    if (pad_w > 0 && X0 + kCfTW >= W) {
        for (int i = tid; i < TH * pad_w * NQ; i += 256) {
            const int q = i % NQ, r = i / NQ, col = r % pad_w, row = r / pad_w;
            const int gy = Y0 + row;
            if (gy < H) *reinterpret_cast<uint4*>(ob + ((int64_t)gy * Wo + W + col) * C + c0 + EPC * q) = make_uint4(0u, 0u, 0u, 0u);
        }
    }
    if (pad_h > 0 && Y0 + TH >= H) {
        const int x_end = (X0 + kCfTW >= W) ? Wo : X0 + kCfTW;   // the corner belongs to the last tile
        for (int i = tid; i < pad_h * (x_end - X0) * NQ; i += 256) {
            const int q = i % NQ, r = i / NQ, col = r % (x_end - X0), row = r / (x_end - X0);
            *reinterpret_cast<uint4*>(ob + ((int64_t)(H + row) * Wo + X0 + col) * C + c0 + EPC * q) = make_uint4(0u, 0u, 0u, 0u);
        }
    }
}

// Mish(acc + bias) of one accumulator quad (four consecutive outputs of a pixel), and its one 4-wide store: fp32, or
// fp16 with ONE rounding
__device__ __forceinline__ float4 bias_mish4(const f32x4e& acc, const float4& bq) {
    return make_float4(conv_mishf(acc[0] + bq.x), conv_mishf(acc[1] + bq.y), conv_mishf(acc[2] + bq.z), conv_mishf(acc[3] + bq.w));
}
__device__ __forceinline__ void bias_mish_store4(float* p, const f32x4e& acc, const float4& bq) {
    *reinterpret_cast<float4*>(p) = bias_mish4(acc, bq);
}
__device__ __forceinline__ void bias_mish_store4(__half* p, const f32x4e& acc, const float4& bq) {
    f16x4e o;
    o[0] = (_Float16)conv_mishf(acc[0] + bq.x);
    o[1] = (_Float16)conv_mishf(acc[1] + bq.y);
    o[2] = (_Float16)conv_mishf(acc[2] + bq.z);
    o[3] = (_Float16)conv_mishf(acc[3] + bq.w);
    *reinterpret_cast<f16x4e*>(p) = o;
}

// A launcher's tiling of B images of H x W pixels by TH x 16 tiles; the grid is n_wgs = n_tiles x slices workgroups
// (slices of the output channels), which must fit the int the kernels decode blockIdx.x with
struct TilePlan {
    int tiles_x, tiles_y;
    int64_t n_tiles, n_wgs;
};
inline bool tile_plan(TilePlan& p, int B, int H, int W, int TH, int slices, const char* what) {
    p.tiles_x = (W + kCfTW - 1) / kCfTW, p.tiles_y = (H + TH - 1) / TH;
    p.n_tiles = (int64_t)p.tiles_x * p.tiles_y * B;
    p.n_wgs = p.n_tiles * slices;
    if (p.n_wgs <= INT32_MAX) return true;
    set_error("%s: too many tiles", what);
    return false;
}

}  // namespace qpwc

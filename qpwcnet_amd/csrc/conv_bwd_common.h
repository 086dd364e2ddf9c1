// Shared by the convolution backward translation units (conv_bwd.hip, upconv_bwd.hip; sepconv_bwd.hip uses the tile
// sum): the implicit-GEMM pieces, the per-workgroup sums and the K-split plan that carry their determinism contract.
//
// v_mfma_f32_16x16x4_f32: lane l holds A[i = l & 15][k = l >> 4] and B[k = l >> 4][j = l & 15]; D register r of lane l
// is row (l >> 4) * 4 + r, column l & 15.  Below li = l & 15, lk = l >> 4, and wave w of the 256 threads owns rows
// 16 w .. 16 w + 15 of a 64-row block.
#pragma once
#include <type_traits>

#include "optflow_common.h"

namespace qpwc {

constexpr int kCgPx = 64;           // pixels (GEMM rows) per block: 16 per wave, 4 waves
constexpr int kCgKC = 32;           // K values staged per step
constexpr int kCgLd = kCgKC + 4;    // LDS row of a staged tile: 16-byte rows, 4 banks apart
constexpr int kCgWTile = 64;        // at most this many output x input channels per workgroup of a stage-W kernel
constexpr int kCgWPad = 20;         // LDS row padding of its pixel-major tiles
constexpr int kCgRedLanes = 16;     // lanes that share one output of conv_bwd_reduce_kernel

// ---- stages Z and X ---------------------------------------------------------------------------------------------------
// row p of a (B, Hr, Wr) row space -> image, row and column; n = -1 past its end
__device__ __forceinline__ void cg_row_decode(int64_t p, int64_t Mr, int Hr, int Wr, int& n, int& y, int& x) {
    n = -1, y = 0, x = 0;
    if (p < Mr) {
        x = (int)(p % Wr);
        const int64_t q = p / Wr;
        y = (int)(q % Hr);
        n = (int)(q / Hr);
    }
}

// The B tile of one K step from wt = w[t], whose rows hold ld floats.
//   rows of w:    b_s[j][k] = wt[j0 + j][k0 + k]
//   columns of w: b_s[j][k] = wt[k0 + k][j0 + j], four scalar LDS stores per float4; with EDGE columns from ncol on
//                 are 0, without it the caller's N columns all lie within ncol and the loads are unconditional
template <int NB, bool EDGE>
__device__ __forceinline__ void cg_stage_b(float* b_s, const float* wt, int ld, int ncol, int j0, int k0, int kc,
                                           bool columns, int tid) {
    if (!columns) {
        const int kq = kc >> 2;
        for (int i = tid; i < NB * kq; i += 256) {
            const int j = i / kq, q = i - j * kq;
            *reinterpret_cast<float4*>(&b_s[j * kCgLd + q * 4]) = ldg_f4(wt + (int64_t)(j0 + j) * ld + k0 + q * 4);
        }
    } else {
        for (int i = tid; i < kc * (NB / 4); i += 256) {
            const int k = i / (NB / 4), j4 = (i % (NB / 4)) * 4;
            const float4 v = !EDGE || j0 + j4 < ncol ? ldg_f4(wt + (int64_t)(k0 + k) * ld + j0 + j4)
                                                     : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            b_s[(j4 + 0) * kCgLd + k] = v.x;
            b_s[(j4 + 1) * kCgLd + k] = v.y;
            b_s[(j4 + 2) * kCgLd + k] = v.z;
            b_s[(j4 + 3) * kCgLd + k] = v.w;
        }
    }
}

// acc[n] += A B_n over the kc staged K values, four per instruction in ascending order
template <int NT>
__device__ __forceinline__ void cg_gemm_step(f32x4v (&acc)[NT], const float* a_s, const float* b_s, int kc, int tid) {
    const int wave = tid >> 6, li = tid & 15, lk = (tid & 63) >> 4;
    for (int kk = 0; kk < kc; kk += 4) {
        const float a = a_s[(wave * 16 + li) * kCgLd + kk + lk];
#pragma unroll
        for (int n = 0; n < NT; ++n)
            acc[n] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, b_s[(n * 16 + li) * kCgLd + kk + lk], acc[n], 0, 0, 0);
    }
}

// ---- stage W ----------------------------------------------------------------------------------------------------------
// A wave's NO x NI tiles += gz_s^T x_s over its 16 pixel rows (the tiles' K), four rows per instruction.  even takes rows
// 0-3 and 8-11, odd rows 4-7 and 12-15: the same tiles, or two sets that the caller adds up at the end.
template <int NO, int NI>
__device__ __forceinline__ void cg_w_mfma(f32x4v (&even)[NO][NI], f32x4v (&odd)[NO][NI], const float* gz_s,
                                          const float* x_s, int tid) {
    constexpr int SG = NO * 16 + kCgWPad, SX = NI * 16 + kCgWPad;
    const int wave = tid >> 6, li = tid & 15, lk = (tid & 63) >> 4;
#pragma unroll
    for (int k = 0; k < 16; k += 4) {
        const int row = wave * 16 + k + lk;
        float a[NO], b[NI];
#pragma unroll
        for (int n = 0; n < NO; ++n) a[n] = gz_s[row * SG + n * 16 + li];
#pragma unroll
        for (int m = 0; m < NI; ++m) b[m] = x_s[row * SX + m * 16 + li];
        f32x4v(&acc)[NO][NI] = (k & 4) ? odd : even;
#pragma unroll
        for (int n = 0; n < NO; ++n)
#pragma unroll
            for (int m = 0; m < NI; ++m) acc[n][m] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[n], b[m], acc[n][m], 0, 0, 0);
    }
}

// The four waves' NO x NI tiles added in wave order through red (NO 16 x NI 16 floats of LDS that every wave is done
// reading), then one partial per workgroup: element (o, c) of the sum -> part[(row0 + o) * ld + c0 + c] where
// c0 + c < ncol.
template <int NO, int NI>
__device__ __forceinline__ void cg_tile_sum(const f32x4v (&acc)[NO][NI], float* red, float* __restrict__ part,
                                            int64_t row0, int ld, int c0, int ncol, int tid) {
    constexpr int OB = NO * 16, IB = NI * 16;
    const int wave = tid >> 6, li = tid & 15, lk = (tid & 63) >> 4;
    for (int wv = 0; wv < 4; ++wv) {
        __syncthreads();
        if (wave == wv) {
#pragma unroll
            for (int n = 0; n < NO; ++n)
#pragma unroll
                for (int m = 0; m < NI; ++m)
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const int i = (n * 16 + lk * 4 + r) * IB + m * 16 + li;
                        red[i] = wv == 0 ? acc[n][m][r] : red[i] + acc[n][m][r];
                    }
        }
    }
    __syncthreads();
    for (int i = tid; i < OB * IB; i += 256) {
        const int o = i / IB, c = i % IB;
        if (c0 + c < ncol) part[(row0 + o) * ld + c0 + c] = red[i];
    }
}

// grad_b of a workgroup: thread = (column tid % OB, row group tid / OB) holds the sum of its rows; the 256 / OB groups
// are added in order through scr (256 floats of LDS) -> part_b[column]
template <int OB>
__device__ __forceinline__ void cg_bias_sum(float bsum, float* scr, float* __restrict__ part_b, int tid) {
    __syncthreads();  // whatever shared scr is read
    scr[tid] = bsum;
    __syncthreads();
    if (tid < OB) {
        float s = scr[tid];
        for (int j = 1; j < 256 / OB; ++j) s += scr[j * OB + tid];
        part_b[tid] = s;
    }
}

// ---- stage R ----------------------------------------------------------------------------------------------------------
// out[i] = sum of part[p * n_out + i] over the n_part workgroups: conv_bwd_reduce_kernel (conv_bwd.hip), 16 lanes per
// output striding over the partials in order, then a fixed binary tree.  The order depends on n_part only.
int conv_bwd_reduce_launch(const float* part, float* out, int64_t n_out, int n_part, hipStream_t s);

// ---- host side --------------------------------------------------------------------------------------------------------
// The K-splits of stage W and the workspace gz | part_w | part_b, offsets in floats, each 16-byte aligned.
struct CgSplit {
    int nsplit;
    int64_t off_gz, off_pw, off_pb, total;
};

// n_pb pixel blocks shared between at most w_blocks / (taps * n_blk) workgroups per (tap, channel block), at least one;
// gz holds gz_floats, a partial w_floats of grad_w and n_out of grad_b.
inline CgSplit cg_split(int64_t n_pb, int w_blocks, int taps, int n_blk, int64_t gz_floats, int64_t w_floats, int n_out) {
    CgSplit k;
    const int cap = w_blocks / (taps * n_blk) > 0 ? w_blocks / (taps * n_blk) : 1;
    k.nsplit = (int)(n_pb < cap ? n_pb : cap);
    auto up4 = [](int64_t n) { return (n + 3) / 4 * 4; };
    k.off_gz = 0;
    k.off_pw = k.off_gz + gz_floats;
    k.off_pb = k.off_pw + k.nsplit * w_floats;
    k.total = k.off_pb + up4((int64_t)k.nsplit * n_out);
    return k;
}

// f(std::integral_constant<int, n>) for n = 1, 2 or 4 tiles; any other n takes 4, the widest
template <class F>
inline void cg_tiles(int n, F&& f) {
    if (n == 1) f(std::integral_constant<int, 1>{});
    else if (n == 2) f(std::integral_constant<int, 2>{});
    else f(std::integral_constant<int, 4>{});
}

}  // namespace qpwc

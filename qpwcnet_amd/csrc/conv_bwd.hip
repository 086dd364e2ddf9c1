// Forward and backward of the encoder's Conv2D(3x3, stride 1 or 2, padding='same') (+ Mish) for gfx950 (MI355X, CDNA4,
// wave64): what training through layers.DownConv / layers.Encoder needs (reference: qpwcnet/core/non_layers.py:390-449,
// differentiated by the trainer).  fp32, channels-last, dense.  Formulas: include/qpwc.h, qpwc_conv3x3_same_bwd.
//
//   z = conv_s(x, w) + b over TensorFlow's 'SAME' window (pt rows above, pl columns left, zeros outside the image)
//   y = Mish(z) if mish else z,   gz = g Mish'(z) if mish else g
//   grad_b[o] = sum_p gz[p,o]     grad_w[t][o][i] = sum_p gz[p,o] x[src(p,t),i]     grad_x = gather of gz through w
//
// Mish is not invertible and the forward stores y only, so z is recomputed.  Stages, each skipped when nothing that is
// asked for consumes it:
//   Z  conv_bwd_gemm_kernel (mode 0)  implicit GEMM over 9 taps x C_in on v_mfma_f32_16x16x4_f32; the epilogue (a kernel
//                                     argument) stores z, Mish(z) (the forward entry point) or g Mish'(z) -> workspace
//   X  conv_bwd_gemm_kernel (mode 1)  grad_x as a gather: the same GEMM over gz with the taps transposed and C_in <-> C_out
//                                     exchanged.  Stride 2: grid.z = the four parity classes of the input pixel, which
//                                     meet 1, 2, 2 and 4 of the 9 taps -- no product with an inserted zero
//   W  conv_bwd_w_kernel              per (K-split, C_out x C_in block, tap): grad_w tiles = gz^T x_shifted kept in
//                                     registers across the workgroup's pixel blocks (grid-stride), one partial per
//                                     workgroup; the tap-0 workgroups of the first C_in block also sum gz for grad_b
//   R  conv_bwd_reduce_kernel         partials summed per output: 16 lanes stride over the workgroups, then a fixed tree
//                                     (also stage R of upconv_bwd.hip, through conv_bwd_reduce_launch)
// The lane layout of the matrix instruction, the B staging, the wave-order tile sum, the grad_b finish and the K-split
// plan are those of conv_bwd_common.h, shared with upconv_bwd.hip.
//
// Determinism: every output element is a sum in a fixed order; no atomics; grids and the number of K-splits depend on the
// shape only; what is asked for is a kernel argument and changes no arithmetic of the other outputs.  A row of the
// GEMMs (a pixel of gz / grad_x) is accumulated independently of every other row: grad_x of an image does not depend
// on the rest of the batch.
#include "conv_bwd_common.h"
#include "launch.h"

namespace qpwc {

// This file's names of the tile constants, which the host-side guards of the tests read from here; the shared helpers
// are written against those of conv_bwd_common.h, so the two sets must agree.
constexpr int kCbPx = 64;           // pixels (GEMM rows) per block: 16 per wave, 4 waves
constexpr int kCbKC = 32;           // K values staged per step
constexpr int kCbLd = kCbKC + 4;    // LDS row of a staged tile: 16-byte rows, 4 banks apart
constexpr int kCbWBlocks = 1024;    // workgroups of conv_bwd_w_kernel, shared between the K-splits, the blocks and the taps
constexpr int kCbWTile = 64;        // at most this many C_out x C_in per workgroup of conv_bwd_w_kernel
constexpr int kCbWPad = 20;         // LDS row padding of its pixel-major tiles
constexpr int kCbRedLanes = 16;     // lanes that share one output of conv_bwd_reduce_kernel
static_assert(kCbPx == kCgPx && kCbKC == kCgKC && kCbLd == kCgLd && kCbWTile == kCgWTile && kCbWPad == kCgWPad &&
                  kCbRedLanes == kCgRedLanes,
              "the tile constants differ from those of conv_bwd_common.h");

struct CbGeo {
    int H, W, Ho, Wo;    // input and output extent
    int s, pt, pl;       // stride, 'SAME' padding above / left
    int cin, cout, cp;   // cp = cin rounded up to 4: the row of the tap-major weights (9, cout, cp)
};

enum { kCbStoreZ = 0, kCbStoreMish = 1, kCbStoreGz = 2 };

// ---- stages Z and X: rows x N = sum over taps and K of A[row, tap, k] B[tap, k, n] ------------------------------------
// mode 0 (Z): row = output pixel (n, oy, ox); A = x at (oy s + ky - pt, ox s + kx - pl); K = cp; N = cout; B = w[t][n][k].
// mode 1 (X): row = input pixel (n, iy, ix) of parity class blockIdx.z; A = gz at ((iy + pt - ky) / s, (ix + pl - kx) / s)
//             over the taps where both are whole; K = cout; N = cin; B = w[t][k][n].
// Workgroup = 64 rows x 16 NT columns (blockIdx.y); wave w owns rows 16 w .. 16 w + 15 and NT accumulators.
template <int NT>
__global__ __launch_bounds__(256) void conv_bwd_gemm_kernel(const float* __restrict__ src, const float* __restrict__ w,
                                                            const float* __restrict__ bias,
                                                            const float* __restrict__ gout, float* __restrict__ dst,
                                                            CbGeo g, int B, int mode, int epi) {
    constexpr int NB = NT * 16;
    __shared__ __attribute__((aligned(16))) float a_s[kCbPx * kCbLd];
    __shared__ __attribute__((aligned(16))) float b_s[NB * kCbLd];
    __shared__ int row_n[kCbPx], row_y[kCbPx], row_x[kCbPx];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int li = lane & 15, lk = lane >> 4;
    const int j0 = blockIdx.y * NB;
    const int cy = mode ? (int)blockIdx.z / g.s : 0, cx = mode ? (int)blockIdx.z % g.s : 0;
    // extent of the row space: the output pixels, or the input pixels of this parity class
    const int Hr = mode ? (g.H > cy ? (g.H - cy + g.s - 1) / g.s : 0) : g.Ho;
    const int Wr = mode ? (g.W > cx ? (g.W - cx + g.s - 1) / g.s : 0) : g.Wo;
    const int64_t Mr = (int64_t)B * Hr * Wr;
    const int64_t p0 = (int64_t)blockIdx.x * kCbPx;
    if (p0 >= Mr) return;  // the grid is sized for the largest class
    const int K = mode ? g.cout : g.cp;       // reduction length per tap
    const int csrc = mode ? g.cout : g.cin;   // floats per pixel of src
    const int Hs = mode ? g.Ho : g.H, Ws = mode ? g.Wo : g.W;
    const int kc = K < kCbKC ? K : kCbKC, kq = kc >> 2;
    if (tid < kCbPx) {
        int n, y, x;
        cg_row_decode(p0 + tid, Mr, Hr, Wr, n, y, x);
        if (mode && n >= 0) {
            y = y * g.s + cy;
            x = x * g.s + cx;
        }
        row_n[tid] = n;
        row_y[tid] = y;
        row_x[tid] = x;
    }
    f32x4v acc[NT] = {};
    for (int ky = 0; ky < 3; ++ky)
        for (int kx = 0; kx < 3; ++kx) {
            // stride 2 gather: only the taps whose source row and column are whole
            if (mode && g.s == 2 && (((cy + g.pt - ky) & 1) || ((cx + g.pl - kx) & 1))) continue;
            const float* wt = w + (int64_t)(ky * 3 + kx) * g.cout * g.cp;
            for (int k0 = 0; k0 < K; k0 += kc) {
                __syncthreads();  // the row table is written; the previous step's fragments are read
                for (int i = tid; i < kCbPx * kq; i += 256) {
                    const int r = i / kq, q = i - r * kq;
                    const int n = row_n[r];
                    int sy, sx;
                    bool ok = n >= 0;
                    if (mode) {
                        const int ny = row_y[r] + g.pt - ky, nx = row_x[r] + g.pl - kx;
                        ok = ok && ny >= 0 && nx >= 0;
                        sy = ny / g.s;
                        sx = nx / g.s;
                    } else {
                        sy = row_y[r] * g.s + ky - g.pt;
                        sx = row_x[r] * g.s + kx - g.pl;
                        ok = ok && sy >= 0 && sx >= 0;
                    }
                    ok = ok && sy < Hs && sx < Ws;
                    float4 v = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
                    if (ok) {
                        const float* p = src + (((int64_t)n * Hs + sy) * Ws + sx) * csrc + k0 + q * 4;
                        if ((csrc & 3) == 0) {
                            v = ldg_f4(p);
                        } else {  // the 12-byte pixels of the first layer: K = 4, slot 3 is 0
                            v.x = ldg_f1(p);
                            v.y = ldg_f1(p + 1);
                            v.z = ldg_f1(p + 2);
                        }
                    }
                    *reinterpret_cast<float4*>(&a_s[r * kCbLd + q * 4]) = v;
                }
                cg_stage_b<NB, true>(b_s, wt, g.cp, g.cp, j0, k0, kc, mode != 0, tid);  // mode 1: the N columns past cp are 0
                __syncthreads();
                cg_gemm_step<NT>(acc, a_s, b_s, kc, tid);
            }
        }
#pragma unroll
    for (int n = 0; n < NT; ++n) {
        const int col = j0 + n * 16 + li;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int row = wave * 16 + lk * 4 + r;
            const int img = row_n[row];
            if (img < 0) continue;
            if (mode) {
                if (col < g.cin)
                    dst[(((int64_t)img * g.H + row_y[row]) * g.W + row_x[row]) * g.cin + col] = acc[n][r];
            } else {
                const int64_t o = (p0 + row) * g.cout + col;
                const float z = acc[n][r] + bias[col];
                dst[o] = epi == kCbStoreGz ? gout[o] * mish_grad(z) : (epi == kCbStoreMish ? mishf(z) : z);
            }
        }
    }
}

// ---- stage W: partial grad_w[t] = gz^T x_shifted(t), partial grad_b ---------------------------------------------------
// grid (K-splits, C_out blocks x C_in blocks, taps).  A workgroup walks its pixel blocks in grid-stride order; wave w
// owns pixels 16 w .. 16 w + 15 of a block (its K) and all NO x NI tiles, whose accumulators live across the walk (two
// per tile, over alternate K steps, when the workgroup has one tile only, added up at the end).  At the end the four
// waves' tiles are added in wave order through LDS.
template <int NO, int NI>
__global__ __launch_bounds__(256) void conv_bwd_w_kernel(const float* __restrict__ gz, const float* __restrict__ x,
                                                         float* __restrict__ part_w, float* __restrict__ part_b,
                                                         CbGeo g, int64_t M, int64_t n_pb, int n_ib, int need_w,
                                                         int need_b) {
    constexpr int OB = NO * 16, IB = NI * 16;
    constexpr int SG = OB + kCbWPad, SX = IB + kCbWPad;
    constexpr int NS = NO * NI == 1 ? 2 : 1;
    __shared__ __attribute__((aligned(16))) float gz_s[kCbPx * SG];
    __shared__ __attribute__((aligned(16))) float x_s[kCbPx * SX];
    const int tid = threadIdx.x;
    const int o0 = ((int)blockIdx.y / n_ib) * OB, i0 = ((int)blockIdx.y % n_ib) * IB;
    const int tap = blockIdx.z, ky = tap / 3, kx = tap % 3;
    const bool do_b = need_b && tap == 0 && i0 == 0;
    f32x4v acc[NS][NO][NI] = {};
    float bsum = 0.0f;
    for (int64_t pb = blockIdx.x; pb < n_pb; pb += gridDim.x) {
        const int64_t p0 = pb * kCbPx;
        __syncthreads();  // the previous block's tiles are read
        for (int i = tid; i < kCbPx * (OB / 4); i += 256) {
            const int r = i / (OB / 4), q = i % (OB / 4);
            const int64_t p = p0 + r;
            const float4 v = p < M ? ldg_f4(gz + p * g.cout + o0 + q * 4) : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            *reinterpret_cast<float4*>(&gz_s[r * SG + q * 4]) = v;
        }
        if (need_w)
            for (int i = tid; i < kCbPx * (IB / 4); i += 256) {
                const int r = i / (IB / 4), q = i % (IB / 4);
                const int64_t p = p0 + r;
                float4 v = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
                const int c = i0 + q * 4;
                if (p < M && c < g.cin) {
                    const int ox = (int)(p % g.Wo);
                    const int64_t t = p / g.Wo;
                    const int oy = (int)(t % g.Ho);
                    const int64_t n = t / g.Ho;
                    const int sy = oy * g.s + ky - g.pt, sx = ox * g.s + kx - g.pl;
                    if (sy >= 0 && sy < g.H && sx >= 0 && sx < g.W) {
                        const float* xp = x + ((n * g.H + sy) * g.W + sx) * g.cin + c;
                        if ((g.cin & 3) == 0) {
                            v = ldg_f4(xp);
                        } else {  // cin = 3: one group, slot 3 stays 0 (the pad slot of grad_w)
                            v.x = ldg_f1(xp);
                            v.y = ldg_f1(xp + 1);
                            v.z = ldg_f1(xp + 2);
                        }
                    }
                }
                *reinterpret_cast<float4*>(&x_s[r * SX + q * 4]) = v;
            }
        __syncthreads();
        if (need_w) cg_w_mfma<NO, NI>(acc[0], acc[NS - 1], gz_s, x_s, tid);
        if (do_b)  // thread = (column, row group): 256 / OB groups of rows, each in row order
            for (int r = tid / OB; r < kCbPx; r += 256 / OB) bsum += gz_s[r * SG + tid % OB];
    }
    if (need_w) {
        if (NS == 2) acc[0][0][0] += acc[NS - 1][0][0];
        // red = gz_s: OB x IB floats, smaller than the gz tile
        cg_tile_sum<NO, NI>(acc[0], gz_s, part_w, ((int64_t)blockIdx.x * 9 + tap) * g.cout + o0, g.cp, i0, g.cp, tid);
    }
    if (do_b) cg_bias_sum<OB>(bsum, x_s, part_b + (int64_t)blockIdx.x * g.cout + o0, tid);
}

// ---- stage R: out[i] = sum over the workgroups' partials ----------------------------------------------------------------
// 16 outputs per workgroup, 16 lanes per output: lane j adds partials j, j + 16, ... in order, then a fixed binary tree
// over the lanes.  The order depends on n_part only.  The one reduce kernel of the convolution backward passes.
__global__ __launch_bounds__(256) void conv_bwd_reduce_kernel(const float* __restrict__ part, float* __restrict__ out,
                                                              int n_out, int n_part) {
    __shared__ float red[kCbRedLanes * 16];
    const int tid = threadIdx.x, o = tid & 15, lane = tid >> 4;
    const int i = blockIdx.x * 16 + o;
    float s = 0.0f;
    if (i < n_out)
        for (int p = lane; p < n_part; p += kCbRedLanes) s += part[(int64_t)p * n_out + i];
    red[lane * 16 + o] = s;
    for (int h = kCbRedLanes / 2; h > 0; h >>= 1) {
        __syncthreads();
        if (lane < h) red[lane * 16 + o] += red[(lane + h) * 16 + o];
    }
    if (lane == 0 && i < n_out) out[i] = red[o];
}

// ---- host side -----------------------------------------------------------------------------------------------------
struct CbPlan {
    CbGeo g;
    int64_t M_out, M_in, n_pb;
    int w_ob, w_ib, n_ob, n_ib;   // stage W: tile, blocks
    CgSplit k;                    // its K-splits and the workspace
};

static CbPlan cb_plan(int B, int H, int W, int cin, int cout, int s) {
    CbPlan p;
    CbGeo& g = p.g;
    g.H = H, g.W = W, g.s = s, g.cin = cin, g.cout = cout;
    g.Ho = (H + s - 1) / s, g.Wo = (W + s - 1) / s;
    const int th = (g.Ho - 1) * s + 3 - H, tw = (g.Wo - 1) * s + 3 - W;
    g.pt = (th > 0 ? th : 0) / 2, g.pl = (tw > 0 ? tw : 0) / 2;
    g.cp = (cin + 3) / 4 * 4;
    p.M_out = (int64_t)B * g.Ho * g.Wo;
    p.M_in = (int64_t)B * H * W;
    p.n_pb = (p.M_out + kCbPx - 1) / kCbPx;
    const int ci16 = cin < 16 ? 16 : cin;
    p.w_ob = cout < kCbWTile ? cout : kCbWTile;
    p.w_ib = ci16 < kCbWTile ? ci16 : kCbWTile;
    p.n_ob = cout / p.w_ob;
    p.n_ib = ci16 / p.w_ib;
    p.k = cg_split(p.n_pb, kCbWBlocks, 9, p.n_ob * p.n_ib, p.M_out * cout, (int64_t)9 * cout * g.cp, cout);
    return p;
}

int64_t conv3x3_same_bwd_workspace_floats(int B, int H, int W, int cin, int cout, int s) {
    return cb_plan(B, H, W, cin, cout, s).k.total;
}

// whether the launch grids of a shape fit: one workgroup per 64 rows in stages Z and X
bool conv3x3_same_shape_ok(int B, int H, int W, int cin, int cout, int s) {
    const CbPlan p = cb_plan(B, H, W, cin, cout, s);
    return (p.M_in + kCbPx - 1) / kCbPx <= INT32_MAX && B <= (1 << 24);
}

static int cb_gemm(const CbPlan& p, int B, const float* src, const float* w, const float* bias, const float* gout,
                   float* dst, int mode, int epi, hipStream_t s) {
    const CbGeo& g = p.g;
    const int N = mode ? (g.cin < 16 ? 16 : g.cin) : g.cout;
    const int nt = N >= 64 ? 4 : N / 16;
    int64_t rows = p.M_out;
    unsigned gz = 1;
    if (mode) {  // class (0, 0) holds the most pixels
        rows = (int64_t)B * ((g.H + g.s - 1) / g.s) * ((g.W + g.s - 1) / g.s);
        gz = (unsigned)(g.s * g.s);
    }
    const dim3 grid((unsigned)((rows + kCbPx - 1) / kCbPx), (unsigned)(N / (16 * nt)), gz);
    cg_tiles(nt, [&](auto NT) {
        hipLaunchKernelGGL((conv_bwd_gemm_kernel<decltype(NT)::value>), grid, dim3(256), 0, s, src, w, bias, gout, dst, g,
                           B, mode, epi);
    });
    return check_launch("conv_bwd_gemm_kernel");
}

int conv_bwd_reduce_launch(const float* part, float* out, int64_t n_out, int n_part, hipStream_t s) {
    hipLaunchKernelGGL(conv_bwd_reduce_kernel, dim3((unsigned)((n_out + 15) / 16)), dim3(256), 0, s, part, out,
                       (int)n_out, n_part);
    return check_launch("conv_bwd_reduce_kernel");
}

int conv3x3_same_fwd_launch(const void* x, const void* w, const void* bias, void* out, int B, int H, int W, int cin,
                            int cout, int stride, int mish, hipStream_t s) {
    const CbPlan p = cb_plan(B, H, W, cin, cout, stride);
    return cb_gemm(p, B, (const float*)x, (const float*)w, (const float*)bias, nullptr, (float*)out, 0,
                   mish ? kCbStoreMish : kCbStoreZ, s);
}

int conv3x3_same_bwd_launch(const void* x, const void* w, const void* bias, const void* gout, void* gx, void* gw,
                            void* gb, void* ws, int B, int H, int W, int cin, int cout, int stride, int mish,
                            hipStream_t s) {
    const CbPlan p = cb_plan(B, H, W, cin, cout, stride);
    float* wsf = (float*)ws;
    float *gz_ws = wsf + p.k.off_gz, *part_w = wsf + p.k.off_pw, *part_b = wsf + p.k.off_pb;
    const float* gz = (const float*)gout;
    int rc;
    if (mish) {  // stage Z
        if ((rc = cb_gemm(p, B, (const float*)x, (const float*)w, (const float*)bias, (const float*)gout, gz_ws, 0,
                          kCbStoreGz, s)))
            return rc;
        gz = gz_ws;
    }
    if (gx && (rc = cb_gemm(p, B, gz, (const float*)w, nullptr, nullptr, (float*)gx, 1, 0, s))) return rc;  // stage X
    if (gw || gb) {  // stage W; only grad_b: the tap-0 workgroups of one C_in block
        const int n_ib = gw ? p.n_ib : 1;
        const dim3 grid((unsigned)p.k.nsplit, (unsigned)(p.n_ob * n_ib), gw ? 9u : 1u);
        cg_tiles(p.w_ob / 16, [&](auto NO) {
            cg_tiles(p.w_ib / 16, [&](auto NI) {
                hipLaunchKernelGGL((conv_bwd_w_kernel<decltype(NO)::value, decltype(NI)::value>), grid, dim3(256), 0, s,
                                   gz, (const float*)x, part_w, part_b, p.g, p.M_out, p.n_pb, n_ib, (int)(gw != nullptr),
                                   (int)(gb != nullptr));
            });
        });
        if ((rc = check_launch("conv_bwd_w_kernel"))) return rc;
        // stage R
        if (gw && (rc = conv_bwd_reduce_launch(part_w, (float*)gw, (int64_t)9 * cout * p.g.cp, p.k.nsplit, s))) return rc;
        if (gb && (rc = conv_bwd_reduce_launch(part_b, (float*)gb, cout, p.k.nsplit, s))) return rc;
    }
    return QPWC_OK;
}

}  // namespace qpwc

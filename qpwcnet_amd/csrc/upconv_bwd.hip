// Backward of the decoder's Mish(Conv2DTranspose(F, 4x4, strides 2, 'same')(x) + bias) for gfx950 (MI355X, CDNA4,
// wave64): what training through layers.UpConv / layers.Decoder needs (reference: qpwcnet/core/non_layers.py:196-210,
// differentiated by the trainer).  fp32, channels-last, dense.  Formulas: include/qpwc.h, qpwc_upconv4x4s2_bwd.
//
//   z[n,oy,ox,f] = b[f] + sum_{ky,kx,c} w[ky,kx][f][c] x[n,iy,ix,c]  over oy = 2 iy - 1 + ky, ox = 2 ix - 1 + kx
//   gz = g Mish'(z) if mish else g
//   grad_b[f] = sum gz     grad_w[ky,kx][f][c] = sum_p gz[2 iy - 1 + ky, 2 ix - 1 + kx, f] x[p,c]
//   grad_x[p,c] = sum_{ky,kx,f} w[ky,kx][f][c] gz[2 iy - 1 + ky, 2 ix - 1 + kx, f]       (p = input pixel (n,iy,ix))
//
// The forward stores Mish(z) only (into the concat buffer), so z is recomputed.  g is read in place from a buffer whose
// pixels are `gs` floats apart: the `up` half of the gradient of concat([up, skip]).  Stages, each skipped when nothing
// that is asked for consumes it:
//   Z  upconv_bwd_gemm_kernel (mode 0)  per output parity (grid.z): rows = the B H W output pixels of the class, which
//                                       meet 2 x 2 of the 16 taps; K = C per tap; N = F; the epilogue stores
//                                       g Mish'(z + b) to a dense (B 2H 2W, F) workspace.  mish = 0: not launched, the
//                                       later stages read g through its stride
//   X  upconv_bwd_gemm_kernel (mode 1)  grad_x as a 4x4 stride-2 gather over gz: rows = input pixels, every one of
//                                       which meets all 16 taps; K = F per tap; N = C
//   W  upconv_bwd_w_kernel              per (K-split, F x C block, tap): grad_w tiles = gz_shifted^T x kept in registers
//                                       across the workgroup's input-pixel blocks (grid-stride), one partial per
//                                       workgroup; the tap-0 workgroups of the first C block also sum gz over the
//                                       2 x 2 output pixels under each of their input pixels for grad_b
//   R  conv_bwd_reduce_kernel           partials summed per output: 16 lanes stride over the workgroups, then a fixed tree
//                                       (the kernel of conv_bwd.hip, through conv_bwd_reduce_launch)
// The lane layout of the matrix instruction, the B staging, the wave-order tile sum, the grad_b finish and the K-split
// plan are those of conv_bwd_common.h, shared with conv_bwd.hip.
//
// Determinism: every output element is a sum in a fixed order; no atomics; grids and the number of K-splits depend on the
// shape only; what is asked for is a kernel argument and changes no arithmetic of the other outputs.  A row of the
// GEMMs (a pixel of gz / grad_x) is accumulated independently of every other row: grad_x of an image does not depend
// on the rest of the batch.  Pixel offsets are 64-bit.
#include "conv_bwd_common.h"
#include "launch.h"

namespace qpwc {

// This file's names of the tile constants, which the host-side guards of the tests read from here; the shared helpers
// are written against those of conv_bwd_common.h, so the two sets must agree.
constexpr int kUbPx = 64;           // pixels (GEMM rows) per block: 16 per wave, 4 waves
constexpr int kUbKC = 32;           // K values staged per step
constexpr int kUbLd = kUbKC + 4;    // LDS row of a staged tile: 16-byte rows, 4 banks apart
constexpr int kUbWBlocks = 960;     // workgroups of upconv_bwd_w_kernel, shared between the K-splits, the blocks and the 16 taps
constexpr int kUbWTile = 64;        // at most this many F x C per workgroup of upconv_bwd_w_kernel
constexpr int kUbWPad = 20;         // LDS row padding of its pixel-major tiles
constexpr int kUbRedLanes = 16;     // lanes that share one output of stage R (conv_bwd_reduce_kernel of conv_bwd.hip)
static_assert(kUbPx == kCgPx && kUbKC == kCgKC && kUbLd == kCgLd && kUbWTile == kCgWTile && kUbWPad == kCgWPad &&
                  kUbRedLanes == kCgRedLanes,
              "the tile constants differ from those of conv_bwd_common.h");

struct UbGeo {
    int H, W;       // input extent; the output is 2H x 2W
    int C, F;       // input / output channels
    int64_t gs;     // floats between the pixels of gz as stages X and W read it
};

// ---- stages Z and X: rows x N = sum over taps and K of A[row, tap, k] B[tap, k, n] ------------------------------------
// mode 0 (Z): row = (n, ry, rx), the output pixel (2 ry + py, 2 rx + px) of parity class blockIdx.z = py * 2 + px;
//             A = x at (ry + (py + 1 - ky) / 2, rx + (px + 1 - kx) / 2) over the taps where both are whole; K = C;
//             N = F; B = w[t][n][k].
// mode 1 (X): row = input pixel (n, iy, ix); A = gz at (2 iy - 1 + ky, 2 ix - 1 + kx); K = F; N = C; B = w[t][k][n].
// Workgroup = 64 rows x 16 NT columns (blockIdx.y); wave w owns rows 16 w .. 16 w + 15 and NT accumulators.
template <int NT>
__global__ __launch_bounds__(256) void upconv_bwd_gemm_kernel(const float* __restrict__ src, const float* __restrict__ w,
                                                              const float* __restrict__ bias,
                                                              const float* __restrict__ gout, int64_t gout_stride,
                                                              float* __restrict__ dst, UbGeo g, int B, int mode) {
    constexpr int NB = NT * 16;
    __shared__ __attribute__((aligned(16))) float a_s[kUbPx * kUbLd];
    __shared__ __attribute__((aligned(16))) float b_s[NB * kUbLd];
    __shared__ int row_n[kUbPx], row_y[kUbPx], row_x[kUbPx];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int li = lane & 15, lk = lane >> 4;
    const int j0 = blockIdx.y * NB;
    const int py = mode ? 0 : (int)blockIdx.z >> 1, px = mode ? 0 : (int)blockIdx.z & 1;
    const int64_t Mr = (int64_t)B * g.H * g.W;   // rows: the input pixels, or the output pixels of one class
    const int64_t p0 = (int64_t)blockIdx.x * kUbPx;
    const int K = mode ? g.F : g.C;              // reduction length per tap
    const int64_t ssrc = mode ? g.gs : g.C;      // floats per pixel of src
    const int Hs = mode ? 2 * g.H : g.H, Ws = mode ? 2 * g.W : g.W;
    const int kc = K < kUbKC ? K : kUbKC, kq = kc >> 2;
    if (tid < kUbPx) {
        int n, y, x;
        cg_row_decode(p0 + tid, Mr, g.H, g.W, n, y, x);
        row_n[tid] = n;
        row_y[tid] = y;
        row_x[tid] = x;
    }
    f32x4v acc[NT] = {};
    for (int ky = 0; ky < 4; ++ky)
        for (int kx = 0; kx < 4; ++kx) {
            // an output pixel of parity (py, px) meets the taps of the other parity only
            if (mode == 0 && (((py + 1 - ky) & 1) || ((px + 1 - kx) & 1))) continue;
            const int dy = (py + 1 - ky) >> 1, dx = (px + 1 - kx) >> 1;   // mode 0: -1, 0 or 1
            const float* wt = w + (int64_t)(ky * 4 + kx) * g.F * g.C;
            for (int k0 = 0; k0 < K; k0 += kc) {
                __syncthreads();  // the row table is written; the previous step's fragments are read
                for (int i = tid; i < kUbPx * kq; i += 256) {
                    const int r = i / kq, q = i - r * kq;
                    const int n = row_n[r];
                    const int sy = mode ? 2 * row_y[r] - 1 + ky : row_y[r] + dy;
                    const int sx = mode ? 2 * row_x[r] - 1 + kx : row_x[r] + dx;
                    float4 v = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
                    if (n >= 0 && sy >= 0 && sx >= 0 && sy < Hs && sx < Ws)
                        v = ldg_f4(src + (((int64_t)n * Hs + sy) * Ws + sx) * ssrc + k0 + q * 4);
                    *reinterpret_cast<float4*>(&a_s[r * kUbLd + q * 4]) = v;
                }
                cg_stage_b<NB, false>(b_s, wt, g.C, g.C, j0, k0, kc, mode != 0, tid);  // every N column lies within C
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
                dst[(p0 + row) * g.C + col] = acc[n][r];
            } else {
                const int64_t o = ((int64_t)img * 2 * g.H + 2 * row_y[row] + py) * (2 * g.W) + 2 * row_x[row] + px;
                dst[o * g.F + col] = gout[o * gout_stride + col] * mish_grad(acc[n][r] + bias[col]);
            }
        }
    }
}

// ---- stage W: partial grad_w[t] = gz_shifted(t)^T x, partial grad_b ---------------------------------------------------
// grid (K-splits, F blocks x C blocks, taps).  A workgroup walks its blocks of input pixels in grid-stride order; wave w
// owns pixels 16 w .. 16 w + 15 of a block (its K) and all NO x NI tiles, whose accumulators live across the walk.  At
// the end the four waves' tiles are added in wave order through LDS.  The 2 x 2 output pixels (2 iy + a, 2 ix + b)
// under the input pixels tile the output exactly: the grad_b workgroups add those four values of gz per input pixel.
template <int NO, int NI>
__global__ __launch_bounds__(256) void upconv_bwd_w_kernel(const float* __restrict__ gz, const float* __restrict__ x,
                                                           float* __restrict__ part_w, float* __restrict__ part_b,
                                                           UbGeo g, int64_t M, int64_t n_pb, int n_ib, int need_w,
                                                           int need_b) {
    constexpr int OB = NO * 16, IB = NI * 16;
    constexpr int SG = OB + kUbWPad, SX = IB + kUbWPad;
    __shared__ __attribute__((aligned(16))) float gz_s[kUbPx * SG];
    __shared__ __attribute__((aligned(16))) float x_s[kUbPx * SX];
    const int tid = threadIdx.x;
    const int o0 = ((int)blockIdx.y / n_ib) * OB, i0 = ((int)blockIdx.y % n_ib) * IB;
    const int tap = blockIdx.z, ky = tap >> 2, kx = tap & 3;
    const bool do_b = need_b && tap == 0 && i0 == 0;
    const int Ho = 2 * g.H, Wo = 2 * g.W;
    f32x4v acc[NO][NI] = {};
    float bsum = 0.0f;
    for (int64_t pb = blockIdx.x; pb < n_pb; pb += gridDim.x) {
        const int64_t p0 = pb * kUbPx;
        if (need_w) {
            __syncthreads();  // the previous block's tiles are read
            for (int i = tid; i < kUbPx * (OB / 4); i += 256) {
                const int r = i / (OB / 4), q = i % (OB / 4);
                const int64_t p = p0 + r;
                float4 v = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
                if (p < M) {
                    const int ix = (int)(p % g.W);
                    const int64_t t = p / g.W;
                    const int iy = (int)(t % g.H);
                    const int64_t n = t / g.H;
                    const int sy = 2 * iy - 1 + ky, sx = 2 * ix - 1 + kx;
                    if (sy >= 0 && sy < Ho && sx >= 0 && sx < Wo)
                        v = ldg_f4(gz + ((n * Ho + sy) * Wo + sx) * g.gs + o0 + q * 4);
                }
                *reinterpret_cast<float4*>(&gz_s[r * SG + q * 4]) = v;
            }
            for (int i = tid; i < kUbPx * (IB / 4); i += 256) {
                const int r = i / (IB / 4), q = i % (IB / 4);
                const int64_t p = p0 + r;
                const float4 v = p < M ? ldg_f4(x + p * g.C + i0 + q * 4) : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
                *reinterpret_cast<float4*>(&x_s[r * SX + q * 4]) = v;
            }
            __syncthreads();
            cg_w_mfma<NO, NI>(acc, acc, gz_s, x_s, tid);
        }
        if (do_b)  // thread = (column, row group): 256 / OB groups of rows, each in row order
            for (int r = tid / OB; r < kUbPx; r += 256 / OB) {
                const int64_t p = p0 + r;
                if (p >= M) break;
                const int ix = (int)(p % g.W);
                const int64_t t = p / g.W;
                const int iy = (int)(t % g.H);
                const int64_t n = t / g.H;
                const float* q = gz + ((n * Ho + 2 * iy) * Wo + 2 * ix) * g.gs + o0 + tid % OB;
                bsum += (ldg_f1(q) + ldg_f1(q + g.gs)) + (ldg_f1(q + Wo * g.gs) + ldg_f1(q + (Wo + 1) * g.gs));
            }
    }
    if (need_w)  // red = gz_s: OB x IB floats, no larger than the gz tile
        cg_tile_sum<NO, NI>(acc, gz_s, part_w, ((int64_t)blockIdx.x * 16 + tap) * g.F + o0, g.C, i0, g.C, tid);
    if (do_b) cg_bias_sum<OB>(bsum, x_s, part_b + (int64_t)blockIdx.x * g.F + o0, tid);
}

// ---- host side -----------------------------------------------------------------------------------------------------
struct UbPlan {
    int64_t M_in, M_out, n_pb;
    int w_ob, n_ob, n_ib;   // stage W: F tile, blocks (the C tile is kUbWTile)
    CgSplit k;              // its K-splits and the workspace
};

static UbPlan ub_plan(int B, int H, int W, int C, int F) {
    UbPlan p;
    p.M_in = (int64_t)B * H * W;
    p.M_out = 4 * p.M_in;
    p.n_pb = (p.M_in + kUbPx - 1) / kUbPx;
    p.w_ob = F < kUbWTile ? F : kUbWTile;
    p.n_ob = F / p.w_ob;
    p.n_ib = C / kUbWTile;
    p.k = cg_split(p.n_pb, kUbWBlocks, 16, p.n_ob * p.n_ib, p.M_out * F, (int64_t)16 * F * C, F);
    return p;
}

int64_t upconv4x4s2_bwd_workspace_floats(int B, int H, int W, int C, int F) { return ub_plan(B, H, W, C, F).k.total; }

// whether the launch grids of a shape fit: one workgroup per 64 rows in stages Z and X
bool upconv4x4s2_bwd_shape_ok(int B, int H, int W, int C, int F) {
    const UbPlan p = ub_plan(B, H, W, C, F);
    return p.n_pb <= INT32_MAX && B <= (1 << 24) && H <= (1 << 29) && W <= (1 << 29);
}

static int ub_gemm(const UbGeo& g, int B, const float* src, const float* w, const float* bias, const float* gout,
                   int64_t gout_stride, float* dst, int mode, hipStream_t s) {
    const int N = mode ? g.C : g.F;
    const int nt = N >= 64 ? 4 : N / 16;
    const int64_t rows = (int64_t)B * g.H * g.W;
    const dim3 grid((unsigned)((rows + kUbPx - 1) / kUbPx), (unsigned)(N / (16 * nt)), mode ? 1u : 4u);
    cg_tiles(nt, [&](auto NT) {
        hipLaunchKernelGGL((upconv_bwd_gemm_kernel<decltype(NT)::value>), grid, dim3(256), 0, s, src, w, bias, gout,
                           gout_stride, dst, g, B, mode);
    });
    return check_launch("upconv_bwd_gemm_kernel");
}

int upconv4x4s2_bwd_launch(const void* x, const void* w, const void* bias, const void* gout, int64_t gout_stride,
                           void* gx, void* gw, void* gb, void* ws, int B, int H, int W, int C, int F, int mish,
                           hipStream_t s) {
    const UbPlan p = ub_plan(B, H, W, C, F);
    float* wsf = (float*)ws;
    float *gz_ws = wsf + p.k.off_gz, *part_w = wsf + p.k.off_pw, *part_b = wsf + p.k.off_pb;
    UbGeo g;
    g.H = H, g.W = W, g.C = C, g.F = F;
    g.gs = gout_stride;
    const float* gz = (const float*)gout;
    int rc;
    if (mish) {  // stage Z
        if ((rc = ub_gemm(g, B, (const float*)x, (const float*)w, (const float*)bias, (const float*)gout, gout_stride,
                          gz_ws, 0, s)))
            return rc;
        gz = gz_ws;
        g.gs = F;
    }
    if (gx && (rc = ub_gemm(g, B, gz, (const float*)w, nullptr, nullptr, 0, (float*)gx, 1, s))) return rc;  // stage X
    if (gw || gb) {  // stage W; only grad_b: the tap-0 workgroups of one C block
        const int n_ib = gw ? p.n_ib : 1;
        const dim3 grid((unsigned)p.k.nsplit, (unsigned)(p.n_ob * n_ib), gw ? 16u : 1u);
        cg_tiles(p.w_ob / 16, [&](auto NO) {
            hipLaunchKernelGGL((upconv_bwd_w_kernel<decltype(NO)::value, kUbWTile / 16>), grid, dim3(256), 0, s, gz,
                               (const float*)x, part_w, part_b, g, p.M_in, p.n_pb, n_ib, (int)(gw != nullptr),
                               (int)(gb != nullptr));
        });
        if ((rc = check_launch("upconv_bwd_w_kernel"))) return rc;
        // stage R
        if (gw && (rc = conv_bwd_reduce_launch(part_w, (float*)gw, (int64_t)16 * F * C, p.k.nsplit, s))) return rc;
        if (gb && (rc = conv_bwd_reduce_launch(part_b, (float*)gb, F, p.k.nsplit, s))) return rc;
    }
    return QPWC_OK;
}

}  // namespace qpwc

// Image quality of the frame interpolator's output (include/qpwc_quality.h): per-image MSE, PSNR and SSIM with
// tf.image.ssim's default 11 x 11 Gaussian window, in two launches:
//   quality_tile_kernel   one workgroup per (image, tile of kQualTH x kQualTW SSIM positions), all channels: the
//                         (TH + 10) x (TW + 10) window of both images goes through LDS once, with the value transform
//                         applied; per channel a row pass over vt, vp, vt^2 + vp^2 and vt * vp into LDS, a column pass
//                         from it, s, and the tile's sums by wave reductions and one LDS step.  The squared error covers
//                         every input pixel, SSIM only the inner (H - 10) x (W - 10): a tile owns the inputs under its own
//                         positions, and the last tile of a row or column also owns the 10-pixel rim.
//   quality_fold_kernel   one workgroup, a wave per image: sums the image's partials in tile order in double, writes
//                         out and adds the images to the running state in image order.
// No atomics and nothing kept between calls except the state: two runs are bit-identical, and a captured graph replays
// both launches unchanged.  One element-wise load form (4-byte loads for fp32, 2-byte loads for fp16), coalesced along
// the innermost axis: the inputs are read once and the work is in LDS.
#include <math.h>

#include "../../include/qpwc_quality.h"
#include "common.h"
#include "launch.h"

// the value transform and s are separately rounded products and sums, as include/qpwc_quality.h states them; the
// convolutions and the squared error name their fmaf
#pragma clang fp contract(off)

namespace qpwc {

constexpr int kQualThreads = 256;
constexpr int kQualFoldThreads = 1024;              // the fold launch: one workgroup, a wave per image
constexpr int kQualTH = 16, kQualTW = 32;          // SSIM positions per workgroup (_hip.QUALITY_TILE)
constexpr int kQualTaps = 11, kQualRim = kQualTaps - 1;
constexpr int kQualWH = kQualTH + kQualRim, kQualWW = kQualTW + kQualRim;   // the window of inputs: 26 x 42
constexpr int kQualMaps = 4;                       // vt, vp, vt^2 + vp^2, vt * vp

static_assert(kQualThreads == kQualTW * (kQualTH / 2), "the column pass gives every lane two rows of one column");

struct QualParams {
    float g[kQualTaps];
    float off_t, off_p, max_val, c1, c2;
    int flags, f16_t, f16_p;
};

namespace {

__device__ __forceinline__ float qual_load(const void* p, int f16, int o) {
    if (f16) return __half2float(reinterpret_cast<const __half*>(p)[o]);
    return reinterpret_cast<const float*>(p)[o];
}

__device__ __forceinline__ float qual_value(float x, float offset, int flags, float max_val) {
    float v = x + offset;
    if (flags & QPWC_QUALITY_CLIP) v = fminf(fmaxf(v, 0.0f), max_val);
    if (flags & QPWC_QUALITY_U8) v = truncf(255.0f * fminf(fmaxf(v, 0.0f), 1.0f));
    return v;
}

__device__ __forceinline__ float qual_wave_sum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

__device__ __forceinline__ double qual_wave_sum(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

}  // namespace

// blockIdx.x = (image * nty + tile row) * ntx + tile column; ws[blockIdx.x * (C + 1) + q]: q < C the tile's sum of s of
// channel q, q = C its sum of squared errors.  LDS: 2 * C * 26 * 42 + 4 * 26 * 32 + 4 * (C + 1) floats = 39.6 KB at
// C = 3, 48.3 KB at C = 4, static.
template <int C, int LAYOUT>
__global__ __launch_bounds__(kQualThreads) void quality_tile_kernel(const void* __restrict__ truth,
                                                                    const void* __restrict__ pred, int H, int W,
                                                                    int nty, int ntx, QualParams q,
                                                                    float* __restrict__ ws) {
    __shared__ float st[C][kQualWH][kQualWW];
    __shared__ float sp[C][kQualWH][kQualWW];
    __shared__ float rp[kQualMaps][kQualWH][kQualTW];
    __shared__ float red[kQualThreads / 64][C + 1];
    const int tid = threadIdx.x;
    const int bid = blockIdx.x;
    const int rest = bid / ntx, tx = bid - rest * ntx;
    const int n = rest / nty, ty = rest - n * nty;
    const int y0 = ty * kQualTH, x0 = tx * kQualTW;
    // the input pixels whose squared error this tile sums: those under its positions, and the rim behind the last tile
    const int own_h = ty == nty - 1 ? H - y0 : kQualTH;     // 11..26 for the last tile: inside the window
    const int own_w = tx == ntx - 1 ? W - x0 : kQualTW;

    // the window of both images, in the inputs' memory order (B * H * W * C fits 32 bits); zeros beyond the image
    float sq = 0.0f;
#pragma unroll 4
    for (int e = tid; e < C * kQualWH * kQualWW; e += kQualThreads) {
        int c, r, x;
        if (LAYOUT == QPWC_NHWC) {
            r = e / (kQualWW * C);
            const int j = e - r * (kQualWW * C);
            x = j / C;
            c = j - x * C;
        } else {
            c = e / (kQualWH * kQualWW);
            const int j = e - c * (kQualWH * kQualWW);
            r = j / kQualWW;
            x = j - r * kQualWW;
        }
        const int gy = y0 + r, gx = x0 + x;
        float vt = 0.0f, vp = 0.0f;
        if (gy < H && gx < W) {
            const int o = LAYOUT == QPWC_NHWC ? ((n * H + gy) * W + gx) * C + c : ((n * C + c) * H + gy) * W + gx;
            vt = qual_value(qual_load(truth, q.f16_t, o), q.off_t, q.flags, q.max_val);
            vp = qual_value(qual_load(pred, q.f16_p, o), q.off_p, q.flags, q.max_val);
            if (r < own_h && x < own_w) {
                const float d = vt - vp;
                sq = __fmaf_rn(d, d, sq);
            }
        }
        st[c][r][x] = vt;
        sp[c][r][x] = vp;
    }
    __syncthreads();

    const int OH = H - kQualRim, OW = W - kQualRim;
    const int cx = tid % kQualTW, cy = (tid / kQualTW) * 2;    // this lane's column and first row of the column pass
    float ssum[C];
#pragma unroll
    for (int c = 0; c < C; ++c) {
        // row pass: 26 rows x 32 columns of the four maps
        for (int i = tid; i < kQualWH * kQualTW; i += kQualThreads) {
            const int r = i / kQualTW, x = i - r * kQualTW;
            float a0 = 0.0f, a1 = 0.0f, a2 = 0.0f, a3 = 0.0f;
#pragma unroll
            for (int k = 0; k < kQualTaps; ++k) {
                const float a = st[c][r][x + k], b = sp[c][r][x + k];
                a0 = __fmaf_rn(q.g[k], a, a0);
                a1 = __fmaf_rn(q.g[k], b, a1);
                a2 = __fmaf_rn(q.g[k], a * a + b * b, a2);
                a3 = __fmaf_rn(q.g[k], a * b, a3);
            }
            rp[0][r][x] = a0;
            rp[1][r][x] = a1;
            rp[2][r][x] = a2;
            rp[3][r][x] = a3;
        }
        __syncthreads();
        // column pass and s: positions (cy, cx) and (cy + 1, cx) of the tile share 10 of their 11 rows, read once
        float m[2][kQualMaps] = {};
#pragma unroll
        for (int k = 0; k <= kQualTaps; ++k) {
#pragma unroll
            for (int i = 0; i < kQualMaps; ++i) {
                const float v = rp[i][cy + k][cx];
                if (k < kQualTaps) m[0][i] = __fmaf_rn(q.g[k], v, m[0][i]);
                if (k > 0) m[1][i] = __fmaf_rn(q.g[k - 1], v, m[1][i]);
            }
        }
        float acc = 0.0f;
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const float mt = m[j][0], mp = m[j][1], den1 = m[j][2], tp = m[j][3];
            const float num0 = 2.0f * mt * mp, den0 = mt * mt + mp * mp, num1 = 2.0f * tp;
            const float s = (num0 + q.c1) / (den0 + q.c1) * ((num1 - num0 + q.c2) / (den1 - den0 + q.c2));
            if (y0 + cy + j < OH && x0 + cx < OW) acc += s;
        }
        ssum[c] = acc;
        __syncthreads();    // the next channel's row pass overwrites rp
    }

    // the tile's C + 1 sums: wave reductions, then the four waves in order
    const int wave = tid >> 6;
#pragma unroll
    for (int c = 0; c < C; ++c) {
        const float v = qual_wave_sum(ssum[c]);
        if ((tid & 63) == 0) red[wave][c] = v;
    }
    sq = qual_wave_sum(sq);
    if ((tid & 63) == 0) red[wave][C] = sq;
    __syncthreads();
    if (tid <= C) ws[(int64_t)bid * (C + 1) + tid] = ((red[0][tid] + red[1][tid]) + red[2][tid]) + red[3][tid];
}

// One workgroup; wave w of its 16 takes images w, w + 16, ...: lane l sums tiles l, l + 64, ... in double, a wave reduction, and
// lane 0 writes the image's three values.  After every sixteen images thread 0 adds them to the running sums in image
// order.
__global__ __launch_bounds__(kQualFoldThreads) void quality_fold_kernel(const float* __restrict__ ws, int B, int tiles,
                                                                    int C, double elems, double positions,
                                                                    double psnr0, float* __restrict__ out,
                                                                    double* __restrict__ state) {
    __shared__ float res[kQualFoldThreads / 64][3];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int per = C + 1;
    double run[3] = {0.0, 0.0, 0.0};
    if (state != nullptr && tid == 0) {
        run[0] = state[0];
        run[1] = state[1];
        run[2] = state[2];
    }
    for (int n0 = 0; n0 < B; n0 += kQualFoldThreads / 64) {
        const int n = n0 + wave;
        if (n < B) {
            const float* p = ws + (int64_t)n * tiles * per;
            double sq = 0.0, ss[4] = {0.0, 0.0, 0.0, 0.0};
            for (int t = lane; t < tiles; t += 64) {
                const float* pt = p + (int64_t)t * per;
#pragma unroll
                for (int c = 0; c < 4; ++c)
                    if (c < C) ss[c] += (double)pt[c];
                sq += (double)pt[C];
            }
            sq = qual_wave_sum(sq);
            double ssim = 0.0;
#pragma unroll
            for (int c = 0; c < 4; ++c)
                if (c < C) ssim += qual_wave_sum(ss[c]) / positions;
            if (lane == 0) {
                const double mse = sq / elems;
                const float r0 = (float)mse;
                const float r1 = mse > 0.0 ? (float)(psnr0 - 10.0 * log10(mse)) : INFINITY;
                const float r2 = (float)(ssim / (double)C);
                out[n] = r0;
                out[(int64_t)B + n] = r1;
                out[2 * (int64_t)B + n] = r2;
                res[wave][0] = r0;
                res[wave][1] = r1;
                res[wave][2] = r2;
            }
        }
        __syncthreads();
        if (tid == 0) {
            for (int w = 0; w < kQualFoldThreads / 64 && n0 + w < B; ++w) {
                run[0] += (double)res[w][0];
                run[1] += (double)res[w][1];
                run[2] += (double)res[w][2];
            }
        }
        __syncthreads();
    }
    if (state != nullptr && tid == 0) {
        state[0] = run[0];
        state[1] = run[1];
        state[2] = run[2];
        state[3] += (double)B;
    }
}

// ---- host side ------------------------------------------------------------------------------------------------------

static int64_t qual_tiles(int H, int W) {
    return (int64_t)((H - kQualRim + kQualTH - 1) / kQualTH) * ((W - kQualRim + kQualTW - 1) / kQualTW);
}

// every count the launches index with fits 32 bits: B * H * W * C and the workgroups of the tile launch (the fold launch
// is one workgroup); for B >= 1, H, W >= 11 and C in 1..4
bool image_quality_shape_ok(int B, int H, int W, int C) {
    return (int64_t)B * H * W * C <= INT32_MAX && B * qual_tiles(H, W) <= INT32_MAX;
}

int64_t image_quality_workspace_floats(int B, int H, int W, int C) { return B * qual_tiles(H, W) * (C + 1); }

const char* image_quality_fwd_kernel() { return "quality_tile_kernel"; }

int image_quality_fwd_launch(const void* truth, bool f16_t, const void* pred, bool f16_p, int B, int H, int W, int C,
                             int layout, float off_t, float off_p, int flags, float max_val, float* out, double* state,
                             float* ws, hipStream_t s) {
    QualParams q;
    double e[kQualTaps], sum = 0.0;
    for (int k = 0; k < kQualTaps; ++k) sum += e[k] = exp(-(double)((k - 5) * (k - 5)) / 4.5);
    for (int k = 0; k < kQualTaps; ++k) q.g[k] = (float)(e[k] / sum);
    q.off_t = off_t;
    q.off_p = off_p;
    q.max_val = max_val;
    q.c1 = (float)((0.01 * (double)max_val) * (0.01 * (double)max_val));
    q.c2 = (float)((0.03 * (double)max_val) * (0.03 * (double)max_val));
    q.flags = flags;
    q.f16_t = f16_t;
    q.f16_p = f16_p;
    const int nty = (H - kQualRim + kQualTH - 1) / kQualTH, ntx = (W - kQualRim + kQualTW - 1) / kQualTW;
    const dim3 grid((unsigned)(B * qual_tiles(H, W))), block(kQualThreads);
#define QPWC_QUAL(CC)                                                                                                 \
    do {                                                                                                              \
        if (layout == QPWC_NHWC)                                                                                      \
            hipLaunchKernelGGL((quality_tile_kernel<CC, QPWC_NHWC>), grid, block, 0, s, truth, pred, H, W, nty, ntx,  \
                               q, ws);                                                                                \
        else                                                                                                          \
            hipLaunchKernelGGL((quality_tile_kernel<CC, QPWC_NCHW>), grid, block, 0, s, truth, pred, H, W, nty, ntx,  \
                               q, ws);                                                                                \
    } while (0)
    switch (C) {
        case 1: QPWC_QUAL(1); break;
        case 2: QPWC_QUAL(2); break;
        case 3: QPWC_QUAL(3); break;
        default: QPWC_QUAL(4); break;
    }
#undef QPWC_QUAL
    int rc = check_launch("quality_tile_kernel");
    if (rc != QPWC_OK) return rc;
    hipLaunchKernelGGL(quality_fold_kernel, dim3(1), dim3(kQualFoldThreads), 0, s, (const float*)ws, B, nty * ntx, C,
                       (double)H * W * C, (double)(H - kQualRim) * (W - kQualRim), 20.0 * log10((double)max_val), out,
                       state);
    return check_launch("quality_fold_kernel");
}

}  // namespace qpwc

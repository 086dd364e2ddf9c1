// The multi-scale flow losses as one kernel family: loss.hip (dense) and masked_loss.hip (over the valid pixels only)
// declare the grid constants, the __global__ shells and their shared memory, everything else is here once -- the level and
// gradient tables, the per-pixel term and its derivative, the tile walk, the pixel walk, the partial fold, the gradient
// scale loop, and on the host the table fill, the tile-or-pixel plan and the KIND x LAYOUT launch.  MASKED is a
// compile-time variant; where the two differ in bits it says so at the `if constexpr`.
#pragma once
#include "common.h"
#include "launch.h"

namespace qpwc {

// The grid constants kLossThreads, kLossPixBlocks, kLossTileBlocks, kLossTile and kLossBwdBlocks are the including
// file's: loss.hip and masked_loss.hip each state them, under these names, before this header (the CPU suite reads them
// from the .hip text to size its loop cases).  The walks below are written for the values asserted here.
static_assert(kLossThreads == 256 && kLossTile == 32, "the tile walk maps 512 float4 of a 32 x 32 tile to 256 threads");
static_assert(kLossPixBlocks <= kLossTileBlocks, "one workspace of kLossTileBlocks partials a level serves both walks");
constexpr int kLossMaxLevels = 8;
constexpr int kLossMaxSteps = 10;       // tile path: 2x2 / 2x1 / 1x2 sum steps from 1x1 up to 32x32
constexpr int kLossWaves = kLossThreads / 64;   // loss_sum4 adds four
constexpr float kFlowUnknown = 1e9f;    // |component| above it: unknown (the .flo convention); NaN and Inf fail it too

typedef float loss_f32x4 __attribute__((ext_vector_type(4)));

struct LossLevels {
    const void* pred[kLossMaxLevels];   // NULL: taken as zero (gt_out / valid_out only)
    float* dpred[kLossMaxLevels];       // NULL: not written
    float* gt_out[kLossMaxLevels];      // NULL: not written
    int h[kLossMaxLevels], w[kLossMaxLevels];
    int sh[kLossMaxLevels], sw[kLossMaxLevels];   // area factors H / h, W / w
    int f16[kLossMaxLevels];
    float fscale[kLossMaxLevels];       // flow scale h / H on both channels (1 for AutoResizeMseLoss)
    float inv_area[kLossMaxLevels];     // 1 / (sh * sw)                  } dense only: MASKED counts its divisors
    float inv_n[kLossMaxLevels];        // 1 / number of averaged terms   } on the device
    float lscale[kLossMaxLevels];       // FlowMseLossV2: 2 / (w + h)
    float ry_scale[kLossMaxLevels], rx_scale[kLossMaxLevels];   // bilinear: (float)H / h, (float)W / w
    // tile path: the sum pyramid of one tile; step s sums step_ry x step_rx cells (1 or 2 each) of the previous step
    // and evaluates level step_level[s] on the result (-1: an intermediate step)
    int nsteps;
    int step_ry[kLossMaxSteps], step_rx[kLossMaxSteps], step_level[kLossMaxSteps];
};
// The masked extension behind the dense table, whose layout (the dense kernels' kernarg) it leaves alone.
struct MaskedLevels : LossLevels {
    unsigned char* valid_out[kLossMaxLevels];   // NULL: not written
};

struct LossGradsBase {
    const float* d[kLossMaxLevels];
    void* g[kLossMaxLevels];
    int64_t n[kLossMaxLevels];
    int f16[kLossMaxLevels];
};
struct LossGrads : LossGradsBase {
    int vec[kLossMaxLevels];   // n % 4 == 0, d 16-byte and g 16-byte (fp32) / 8-byte (fp16) aligned
};
struct MaskedGrads : LossGradsBase {};   // the boundary holds d and g on the grid: n % 4 == 0 decides

namespace {

template <class T>
__device__ __forceinline__ T loss_wave_sum(T v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
    return v;
}

// the four waves' sums in a fixed order
template <class T>
__device__ __forceinline__ T loss_sum4(const T* r) { return (r[0] + r[1]) + (r[2] + r[3]); }

__device__ __forceinline__ float2 f2add(float2 a, float2 b) { return make_float2(a.x + b.x, a.y + b.y); }

__device__ __forceinline__ float huber(float e, float d) {
    const float a = fabsf(e);
    return a <= d ? 0.5f * e * e : d * a - 0.5f * d * d;     // Keras Huber: the quadratic branch at |e| <= delta
}

__device__ __forceinline__ float huber_grad(float e, float d) { return fabsf(e) <= d ? e : copysignf(d, e); }

__device__ __forceinline__ float sgn(float v) { return v > 0.0f ? 1.0f : (v < 0.0f ? -1.0f : 0.0f); }

__device__ __forceinline__ float ld_pred(const void* p, int64_t i, int f16) {
    if (!p) return 0.0f;
    return f16 ? __half2float(reinterpret_cast<const __half*>(p)[i]) : reinterpret_cast<const float*>(p)[i];
}

// false for NaN and +-Inf as well
__device__ __forceinline__ bool flow_known(float x, float y) { return fabsf(x) <= kFlowUnknown && fabsf(y) <= kFlowUnknown; }

// the number of averaged terms of a level with `count` valid pixels: max(count, 1), per element for the Huber kind
__device__ __forceinline__ double masked_denominator(int64_t count, int per_element) {
    return (double)(count > 0 ? count : 1) * (per_element ? 2.0 : 1.0);
}

// One flow pixel: (gx, gy) the resampled, flow-scaled ground truth, (px, py) the prediction.  Returns the pixel's
// term (FlowMseLossV2: the sum of its two per-element terms); (dx, dy) = d term / d (px, py).
template <int KIND>
__device__ __forceinline__ float flow_term(float gx, float gy, float px, float py, float lscale, float p0, float p1,
                                           float& dx, float& dy) {
    if (KIND == QPWC_LOSS_FLOW_MSE_V2) {
        // Keras Huber(delta = p0) of y_true = s * gt, y_pred = s * pred: error = y_pred - y_true
        const float ex = lscale * px - lscale * gx, ey = lscale * py - lscale * gy;
        dx = lscale * huber_grad(ex, p0);
        dy = lscale * huber_grad(ey, p0);
        return huber(ex, p0) + huber(ey, p0);
    } else if (KIND == QPWC_LOSS_FLOW_MSE) {
        const float rx = gx - px, ry = gy - py;
        const float n = sqrtf(rx * rx + ry * ry);
        const float inv = n > 0.0f ? 1.0f / n : 0.0f;        // 0 at a zero residual (TF: NaN, zeroed by train_step)
        dx = -rx * inv;
        dy = -ry * inv;
        return n;
    } else {                                                  // FlowMseLossFineTune: (|rx| + |ry| + eps)^q
        const float rx = gx - px, ry = gy - py;
        const float base = fabsf(rx) + fabsf(ry) + p1;
        const float t = powf(base, p0);
        const float c = base > 0.0f ? p0 * t / base : 0.0f;  // q * base^(q-1); sign(0) = 0 below
        dx = -c * sgn(rx);
        dy = -c * sgn(ry);
        return t;
    }
}

// element offset of channel 0 of pixel (b, y, x) of a (B, h, w, C) / (B, C, h, w) tensor, and the channel stride
template <int LAYOUT>
__device__ __forceinline__ int64_t pix_offset(int64_t b, int y, int x, int h, int w, int C) {
    return LAYOUT == QPWC_NHWC ? ((b * h + y) * w + x) * C : (b * C * h + y) * (int64_t)w + x;
}
template <int LAYOUT>
__device__ __forceinline__ int64_t chan_stride(int h, int w) {
    return LAYOUT == QPWC_NHWC ? 1 : (int64_t)h * w;
}

// the two channels of prediction pixel (b, y, x) of level l as fp32
template <int LAYOUT>
__device__ __forceinline__ float2 ld_pred_pixel(const LossLevels& lv, int l, int64_t b, int y, int x) {
    const int64_t o = pix_offset<LAYOUT>(b, y, x, lv.h[l], lv.w[l], 2), cs = chan_stride<LAYOUT>(lv.h[l], lv.w[l]);
    return make_float2(ld_pred(lv.pred[l], o, lv.f16[l]), ld_pred(lv.pred[l], o + cs, lv.f16[l]));
}

// One flow pixel of level l: m its validity (dense: true), (gx, gy) its resampled, scaled ground truth (used only where
// m), pv the prediction (may hold anything where !m).  Returns the term, 0 where !m; stores the derivative, the ground
// truth and the validity where asked.  Validity is a selection, never a product.
template <bool MASKED, int KIND, int LAYOUT, class LV>
__device__ __forceinline__ float flow_pixel(const LV& lv, int l, int64_t b, int y, int x, bool m, float gx, float gy,
                                            float p0, float p1, float2 pv) {
    const int h = lv.h[l], w = lv.w[l];
    const int64_t o = pix_offset<LAYOUT>(b, y, x, h, w, 2), cs = chan_stride<LAYOUT>(h, w);
    if constexpr (MASKED) {
        gx = m ? gx : 0.0f;
        gy = m ? gy : 0.0f;
        pv = make_float2(m ? pv.x : 0.0f, m ? pv.y : 0.0f);
    }
    float dx, dy;
    float t = flow_term<KIND>(gx, gy, pv.x, pv.y, lv.lscale[l], p0, p1, dx, dy);
    if constexpr (MASKED) t = m ? t : 0.0f;
    if (float* d = lv.dpred[l]) {
        if constexpr (MASKED) {          // not yet divided by the count; exactly 0 at an invalid pixel
            d[o] = m ? dx : 0.0f;
            d[o + cs] = m ? dy : 0.0f;
        } else {                         // d loss / d y_pred
            d[o] = dx * lv.inv_n[l];
            d[o + cs] = dy * lv.inv_n[l];
        }
    }
    if (float* g = lv.gt_out[l]) {
        g[o] = gx;
        g[o + cs] = gy;
    }
    if constexpr (MASKED)
        if (unsigned char* v = lv.valid_out[l]) v[(b * h + y) * (int64_t)w + x] = m ? 1 : 0;
    return t;
}

// The tile walk.  FlowMseLossV2 of every level from one read of the ground truth (and the mask): a workgroup owns 32x32
// GT pixels at a time (two 16-byte loads per thread, MASKED: and 4 mask bytes; the next tile's loads are in flight
// while this one is reduced), sums them in LDS by 2x2 steps up to every level's area factor (nested powers of two with
// sh * sw >= 4: at most one output per thread) and evaluates that level's pixels of the tile on the way.  MASKED
// carries sum v beside (sum v x, sum v y) through the steps (rawn / auxn; <= 1024, exact in fp32; a level pixel is
// valid iff it is >= 1) and counts the valid level pixels (redn, pcnt).  raw: 1024 cells, aux: 512.
template <bool MASKED, int LAYOUT, class LV>
__device__ __forceinline__ void loss_tile_body(const float* gt, const unsigned char* valid,
                                               const LV& lv, int n_levels, int B, int H, int W, float delta,
                                               float* psum, int* pcnt, float2* raw, float* rawn,
                                               float2* aux, float* auxn, float (*red)[kLossWaves],
                                               int (*redn)[kLossWaves]) {
    const int tid = threadIdx.x;
    const int tiles_x = W / kLossTile, tiles_y = H / kLossTile;
    const int ntiles = B * tiles_y * tiles_x;
    float acc[kLossMaxLevels];
    int cnt[kLossMaxLevels];
#pragma unroll
    for (int k = 0; k < kLossMaxLevels; ++k) {
        acc[k] = 0.0f;
        cnt[k] = 0;
    }

    // 512 float4 per tile, two per thread: float4 i = tid + 256 k.  NHWC: row i / 16 holds 16 float4 (2 pixels each);
    // NCHW: plane i / 256 (= k), row (i / 8) % 32 holds 8 float4 (4 pixels of one channel each)
    const loss_f32x4* g4 = reinterpret_cast<const loss_f32x4*>(gt);
    auto gt_index = [&](int tile, int i) -> int64_t {
        const int tx = tile % tiles_x, ty = (tile / tiles_x) % tiles_y, b = tile / (tiles_x * tiles_y);
        if (LAYOUT == QPWC_NHWC) {
            const int row = i >> 4, c4 = i & 15;
            return ((((int64_t)b * H + ty * kLossTile + row) * W + tx * kLossTile) * 2) / 4 + c4;
        }
        const int c = i >> 8, row = (i >> 3) & 31, c4 = i & 7;
        return ((((int64_t)b * 2 + c) * H + ty * kLossTile + row) * W + tx * kLossTile) / 4 + c4;
    };
    // the mask bytes of the pixels this thread holds: NHWC 2 bytes per k (a 2-byte load), NCHW 4 bytes (a 4-byte load)
    auto ld_mask = [&](int tile, unsigned* mk) {
        mk[0] = mk[1] = 0x01010101u;
        if (!valid) return;
        const int tx = tile % tiles_x, ty = (tile / tiles_x) % tiles_y, b = tile / (tiles_x * tiles_y);
        if (LAYOUT == QPWC_NHWC) {
#pragma unroll
            for (int k = 0; k < 2; ++k) {
                const int i = tid + k * kLossThreads, row = i >> 4, c4 = i & 15;
                const int64_t o = ((int64_t)b * H + ty * kLossTile + row) * W + tx * kLossTile + 2 * c4;
                mk[k] = __builtin_nontemporal_load(reinterpret_cast<const unsigned short*>(valid + o));
            }
        } else {
            const int row = tid >> 3, c4 = tid & 7;
            const int64_t o = ((int64_t)b * H + ty * kLossTile + row) * W + tx * kLossTile + 4 * c4;
            mk[0] = __builtin_nontemporal_load(reinterpret_cast<const unsigned*>(valid + o));
        }
    };
    loss_f32x4 v[2];
    unsigned mk[2];
    if ((int)blockIdx.x < ntiles) {
#pragma unroll
        for (int k = 0; k < 2; ++k) v[k] = __builtin_nontemporal_load(g4 + gt_index(blockIdx.x, tid + k * kLossThreads));
        if constexpr (MASKED) ld_mask(blockIdx.x, mk);
    }
    for (int tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const int tx = tile % tiles_x, ty = (tile / tiles_x) % tiles_y, b = tile / (tiles_x * tiles_y);
        // this thread's prediction pixel of every level of the tile, all loads issued up front: waiting for each
        // level's load inside its step serialised five memory latencies per tile
        float2 pv[kLossMaxSteps];
        {
            int fy = 1, fx = 1;
#pragma unroll
            for (int s = 0; s < kLossMaxSteps; ++s) {
                pv[s] = make_float2(0.0f, 0.0f);
                if (s < lv.nsteps) {
                    fy *= lv.step_ry[s];
                    fx *= lv.step_rx[s];
                    const int l = lv.step_level[s], nx = kLossTile / fx;
                    if (l >= 0 && tid < (kLossTile / fy) * nx)
                        pv[s] = ld_pred_pixel<LAYOUT>(lv, l, b, ty * (kLossTile / fy) + tid / nx, tx * nx + tid % nx);
                }
            }
        }
        __syncthreads();                                   // the previous tile's steps are done with raw / aux
        // Staging does no arithmetic.  Dense: the float4 go to LDS as they came (NCHW: one channel of 4 pixels each);
        // MASKED: a thread holds both channels of its pixels (NCHW: k is the channel) and selects on mask and range
        if constexpr (MASKED) {
            auto put = [&](int cell, float x, float y, unsigned mbyte) {
                const bool ok = mbyte != 0 && flow_known(x, y);
                raw[cell] = make_float2(ok ? x : 0.0f, ok ? y : 0.0f);
                rawn[cell] = ok ? 1.0f : 0.0f;
            };
            if (LAYOUT == QPWC_NHWC) {
#pragma unroll
                for (int k = 0; k < 2; ++k) {
                    const int cell = 2 * (tid + k * kLossThreads);
                    put(cell, v[k].x, v[k].y, mk[k] & 0xffu);
                    put(cell + 1, v[k].z, v[k].w, (mk[k] >> 8) & 0xffu);
                }
            } else {
                const int cell = (tid >> 3) * kLossTile + (tid & 7) * 4;
                put(cell, v[0].x, v[1].x, mk[0] & 0xffu);
                put(cell + 1, v[0].y, v[1].y, (mk[0] >> 8) & 0xffu);
                put(cell + 2, v[0].z, v[1].z, (mk[0] >> 16) & 0xffu);
                put(cell + 3, v[0].w, v[1].w, mk[0] >> 24);
            }
        } else {
#pragma unroll
            for (int k = 0; k < 2; ++k) {
                const int i = tid + k * kLossThreads;
                if (LAYOUT == QPWC_NHWC) {
                    reinterpret_cast<loss_f32x4*>(raw)[i] = v[k];   // 2 pixels = 2 cells
                } else {
                    const int c = i >> 8, row = (i >> 3) & 31, c4 = i & 7;
                    float* cell = reinterpret_cast<float*>(raw + row * kLossTile + c4 * 4) + c;
                    cell[0] = v[k].x;
                    cell[2] = v[k].y;
                    cell[4] = v[k].z;
                    cell[6] = v[k].w;
                }
            }
        }
        const int next = tile + gridDim.x;
        if (next < ntiles) {
#pragma unroll
            for (int k = 0; k < 2; ++k) v[k] = __builtin_nontemporal_load(g4 + gt_index(next, tid + k * kLossThreads));
            if constexpr (MASKED) ld_mask(next, mk);
        }
        __syncthreads();
        int fy = 1, fx = 1;
#pragma unroll
        for (int s = 0; s < kLossMaxSteps; ++s) {
            if (s >= lv.nsteps) continue;
            const int ry = lv.step_ry[s], rx = lv.step_rx[s], l = lv.step_level[s];
            const float2* src = (s & 1) ? aux : raw;
            const float* srcn = (s & 1) ? auxn : rawn;
            float2* dst = (s & 1) ? raw : aux;
            float* dstn = (s & 1) ? rawn : auxn;
            const int pnx = kLossTile / fx;
            fy *= ry;
            fx *= rx;
            const int ny = kLossTile / fy, nx = kLossTile / fx;
            for (int o = tid; o < ny * nx; o += kLossThreads) {
                const int oy = o / nx, ox = o - oy * nx;
                const int pi = (oy * ry) * pnx + ox * rx;
                float2 sum = src[pi];
                float n = MASKED ? srcn[pi] : 0.0f;
                if (rx == 2) {
                    sum = f2add(sum, src[pi + 1]);
                    if constexpr (MASKED) n += srcn[pi + 1];
                }
                if (ry == 2) {
                    float2 q = src[pi + pnx];
                    float qn = MASKED ? srcn[pi + pnx] : 0.0f;
                    if (rx == 2) {
                        q = f2add(q, src[pi + pnx + 1]);
                        if constexpr (MASKED) qn += srcn[pi + pnx + 1];
                    }
                    sum = f2add(sum, q);
                    n += qn;
                }
                dst[o] = sum;
                if constexpr (MASKED) dstn[o] = n;
                if (l >= 0) {
                    const bool m = !MASKED || n >= 1.0f;
                    float gx, gy;
                    if constexpr (MASKED) {
                        // the mean over the block's valid pixels times h / H with one division: for a full block (n a
                        // power of two) h / H / n is exact and the product is the dense branch's, bit for bit
                        const float r = lv.fscale[l] / (m ? n : 1.0f);
                        gx = sum.x * r;
                        gy = sum.y * r;
                    } else {
                        // power-of-two area: the mean is exact; then the flow scale h / H on both channels
                        gx = (sum.x * lv.inv_area[l]) * lv.fscale[l];
                        gy = (sum.y * lv.inv_area[l]) * lv.fscale[l];
                    }
                    const float t = flow_pixel<MASKED, QPWC_LOSS_FLOW_MSE_V2, LAYOUT>(
                        lv, l, b, ty * ny + oy, tx * nx + ox, m, gx, gy, delta, 0.0f, pv[s]);
#pragma unroll
                    for (int k = 0; k < kLossMaxLevels; ++k) {   // no dynamic register index
                        acc[k] += k == l ? t : 0.0f;
                        cnt[k] += (k == l && m) ? 1 : 0;
                    }
                }
            }
            __syncthreads();
        }
    }
    const int lane = tid & 63, wid = tid >> 6;
#pragma unroll
    for (int k = 0; k < kLossMaxLevels; ++k) {
        const float s = loss_wave_sum(acc[k]);
        const int c = MASKED ? loss_wave_sum(cnt[k]) : 0;
        if (lane == 0) {
            red[k][wid] = s;
            if constexpr (MASKED) redn[k][wid] = c;
        }
    }
    __syncthreads();
    if (tid < n_levels) {
        psum[tid * gridDim.x + blockIdx.x] = loss_sum4(red[tid]);
        if constexpr (MASKED) pcnt[tid * gridDim.x + blockIdx.x] = loss_sum4(redn[tid]);
    }
}

// area_pixel_compute_source_index (align_corners = false): src = scale * (dst + 0.5) - 0.5, 0 below 0.  Dense contracts
// the product and the difference (one fused multiply-add).  MASKED rounds them one by one, so that the point is the one
// loss.py's fp32 chain forms: where only corners of small weight are valid, the renormalisation by their sum magnifies
// an ulp of the point a hundredfold.
template <bool MASKED>
__device__ __forceinline__ float loss_sample_point(float scale, int o) {
    if constexpr (MASKED) {
#pragma clang fp contract(off)
        const float p = scale * ((float)o + 0.5f);
        return fmaxf(p - 0.5f, 0.0f);
    } else {
        return fmaxf(scale * ((float)o + 0.5f) - 0.5f, 0.0f);
    }
}

// The pixel walk.  One thread per level pixel, blockIdx.y = level: FlowMseLossV2 with area factors the tile path does
// not take (a loop over the sh x sw block), and the bilinear losses (the 4 ground-truth corners of the half-pixel sample
// point: tf.image.resize = F.interpolate(align_corners=False), no antialias; MASKED: their weights renormalised over the
// valid ones).  C: the ground truth's channels (AutoResizeMseLoss, dense only; the flow kinds have 2).
template <bool MASKED, int KIND, int LAYOUT, class LV>
__device__ __forceinline__ void loss_pixel_body(const float* gt, const unsigned char* valid,
                                                const LV& lv, int B, int H, int W, int C, float p0, float p1,
                                                float* psum, int* pcnt, float* red, int* redn) {
    static_assert(!MASKED || KIND != QPWC_LOSS_AUTORESIZE_MSE, "AutoResizeMseLoss has no masked form");
    const int l = blockIdx.y;
    const int h = lv.h[l], w = lv.w[l];
    const int64_t plane = (int64_t)h * w, n = (int64_t)B * plane;
    const int64_t gcs = chan_stride<LAYOUT>(H, W);
    float acc = 0.0f;
    int cnt = 0;   // a workgroup sees n / kLossPixBlocks pixels: below 2^31 for every tensor that fits a device
    // MASKED: the ground truth at element offset o = pixel (b, y, x) where it is valid: ok, and (gx, gy) only then
    auto known = [&](int64_t b, int y, int x, int64_t o, float& gx, float& gy) -> bool {
        if (valid && valid[(b * H + y) * (int64_t)W + x] == 0) return false;
        gx = gt[o];
        gy = gt[o + gcs];
        return flow_known(gx, gy);
    };
    for (int64_t i = (int64_t)blockIdx.x * kLossThreads + threadIdx.x; i < n; i += (int64_t)gridDim.x * kLossThreads) {
        const int64_t b = i / plane;
        const int r = (int)(i - b * plane);
        const int y = r / w, x = r - y * w;
        bool m = true;
        float gx = 0.0f, gy = 0.0f;    // the level's ground truth at this pixel, before the flow scale
        if (KIND == QPWC_LOSS_FLOW_MSE_V2) {
            const int sh = lv.sh[l], sw = lv.sw[l];
            // each row's sum first, then the rows: one running sum over all sh * sw terms put a 32 x 32 mean ~1e-6 of
            // the level's largest value off (the tile path's 2 x 2 steps: ~1e-7); MASKED counts the valid as an integer
            float sx = 0.0f, sy = 0.0f;
            int nv = 0;
            for (int yy = 0; yy < sh; ++yy) {
                const int64_t o = pix_offset<LAYOUT>(b, y * sh + yy, x * sw, H, W, 2);
                float rx = 0.0f, ry = 0.0f;
                for (int xx = 0; xx < sw; ++xx) {
                    const int64_t oo = o + (LAYOUT == QPWC_NHWC ? 2 * xx : xx);
                    if constexpr (MASKED) {
                        float kx, ky;
                        const bool ok = known(b, y * sh + yy, x * sw + xx, oo, kx, ky);
                        rx += ok ? kx : 0.0f;
                        ry += ok ? ky : 0.0f;
                        nv += ok ? 1 : 0;
                    } else {
                        rx += gt[oo];
                        ry += gt[oo + gcs];
                    }
                }
                sx += rx;
                sy += ry;
            }
            if constexpr (MASKED) {
                const float sn = (float)nv;
                m = sn >= 1.0f;
                const float dn = m ? sn : 1.0f;
                gx = sx / dn;
                gy = sy / dn;
            } else {
                gx = sx * lv.inv_area[l];
                gy = sy * lv.inv_area[l];
            }
        } else {
            const float fy = loss_sample_point<MASKED>(lv.ry_scale[l], y), fx = loss_sample_point<MASKED>(lv.rx_scale[l], x);
            // fy < H, fx < W: the min never binds
            const int y0 = MASKED ? min((int)fy, H - 1) : (int)fy, x0 = MASKED ? min((int)fx, W - 1) : (int)fx;
            const int y1 = y0 + (y0 < H - 1 ? 1 : 0), x1 = x0 + (x0 < W - 1 ? 1 : 0);
            const float ly1 = fy - (float)y0, lx1 = fx - (float)x0;
            const float ly0 = 1.0f - ly1, lx0 = 1.0f - lx1;
            const int cc = KIND == QPWC_LOSS_AUTORESIZE_MSE ? C : 2;
            const int64_t o00 = pix_offset<LAYOUT>(b, y0, x0, H, W, cc), o01 = pix_offset<LAYOUT>(b, y0, x1, H, W, cc);
            const int64_t o10 = pix_offset<LAYOUT>(b, y1, x0, H, W, cc), o11 = pix_offset<LAYOUT>(b, y1, x1, H, W, cc);
            auto sample = [&](int c) -> float {
                const int64_t k = c * gcs;
                return ly0 * (lx0 * gt[o00 + k] + lx1 * gt[o01 + k]) + ly1 * (lx0 * gt[o10 + k] + lx1 * gt[o11 + k]);
            };
            if constexpr (KIND == QPWC_LOSS_AUTORESIZE_MSE) {
                const int64_t o = pix_offset<LAYOUT>(b, y, x, h, w, C), cs = chan_stride<LAYOUT>(h, w);
                for (int c = 0; c < C; ++c) {
                    const float g = sample(c);
                    const float e = ld_pred(lv.pred[l], o + c * cs, lv.f16[l]) - g;
                    acc += e * e;
                    if (float* d = lv.dpred[l]) d[o + c * cs] = (2.0f * e) * lv.inv_n[l];
                    if (float* go = lv.gt_out[l]) go[o + c * cs] = g;
                }
                continue;
            } else if constexpr (MASKED) {
                const int cy[4] = {y0, y0, y1, y1}, cx[4] = {x0, x1, x0, x1};
                const int64_t co[4] = {o00, o01, o10, o11};
                const float cw[4] = {ly0 * lx0, ly0 * lx1, ly1 * lx0, ly1 * lx1};
                float sx = 0.0f, sy = 0.0f, sn = 0.0f;
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    float kx, ky;
                    const bool ok = known(b, cy[k], cx[k], co[k], kx, ky);
                    sx += ok ? cw[k] * kx : 0.0f;
                    sy += ok ? cw[k] * ky : 0.0f;
                    sn += ok ? cw[k] : 0.0f;
                }
                m = sn > 0.0f;
                const float dn = m ? sn : 1.0f;
                gx = sx / dn;
                gy = sy / dn;
            } else {
                gx = sample(0);
                gy = sample(1);
            }
        }
        if constexpr (KIND != QPWC_LOSS_AUTORESIZE_MSE) {
            acc += flow_pixel<MASKED, KIND, LAYOUT>(lv, l, b, y, x, m, gx * lv.fscale[l], gy * lv.fscale[l], p0, p1,
                                                    ld_pred_pixel<LAYOUT>(lv, l, b, y, x));
            cnt += m ? 1 : 0;
        }
    }
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    acc = loss_wave_sum(acc);
    if (lane == 0) red[wid] = acc;
    if constexpr (MASKED) {
        cnt = loss_wave_sum(cnt);
        if (lane == 0) redn[wid] = cnt;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        psum[l * gridDim.x + blockIdx.x] = loss_sum4(red);
        if constexpr (MASKED) pcnt[l * gridDim.x + blockIdx.x] = loss_sum4(redn);
    }
}

// The partial fold of level blockIdx.x: its nblk partial sums (MASKED: and counts) in a fixed order; leaves the four
// waves' totals in red (redn) behind a barrier, for loss_sum4.
template <bool MASKED>
__device__ __forceinline__ void loss_fold_body(const float* psum, const int* pcnt, int nblk, float* red, long long* redn) {
    const int l = blockIdx.x;
    float s = 0.0f;
    long long c = 0;
    for (int i = threadIdx.x; i < nblk; i += kLossThreads) {
        s += psum[l * nblk + i];
        if constexpr (MASKED) c += pcnt[l * nblk + i];
    }
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    s = loss_wave_sum(s);
    if (lane == 0) red[wid] = s;
    if constexpr (MASKED) {
        c = loss_wave_sum(c);
        if (lane == 0) redn[wid] = c;
    }
    __syncthreads();
}

// The gradient scale loop of level blockIdx.y: grad_pred = s * dpred in the prediction's dtype; 16 bytes of dpred per
// thread where the caller allows it (vec: n % 4 == 0 and both on the grid)
__device__ __forceinline__ void loss_scale_body(const LossGradsBase& lg, float s, bool vec) {
    const int l = blockIdx.y;
    const float* d = lg.d[l];
    const int64_t n = lg.n[l];
    const int64_t tid = (int64_t)blockIdx.x * kLossThreads + threadIdx.x, nthr = (int64_t)gridDim.x * kLossThreads;
    if (vec) {
        const loss_f32x4* d4 = reinterpret_cast<const loss_f32x4*>(d);
        for (int64_t i = tid; i < n / 4; i += nthr) {
            const loss_f32x4 v = __builtin_nontemporal_load(d4 + i);
            const float4 r = make_float4(s * v.x, s * v.y, s * v.z, s * v.w);
            if (lg.f16[l]) st4(reinterpret_cast<__half*>(lg.g[l]) + 4 * i, r);
            else st4(reinterpret_cast<float*>(lg.g[l]) + 4 * i, r);
        }
        return;
    }
    for (int64_t i = tid; i < n; i += nthr) {
        if (lg.f16[l]) st(reinterpret_cast<__half*>(lg.g[l]) + i, s * d[i]);
        else st(reinterpret_cast<float*>(lg.g[l]) + i, s * d[i]);
    }
}

// ---- host side ------------------------------------------------------------------------------------------------------

inline bool loss_pow2(int v) { return v > 0 && (v & (v - 1)) == 0; }

// The tile path's sum steps for these levels, or false when it does not apply: H, W multiples of the tile edge (32);
// every factor a power of two <= the edge with sh * sw >= 4; the factors nested (ordered by area, each divides the
// next), none repeated.
inline bool loss_tile_plan(int H, int W, const int* h, const int* w, int n, LossLevels& lv) {
    if (H % kLossTile || W % kLossTile) return false;
    int order[kLossMaxLevels];
    for (int i = 0; i < n; ++i) {
        if (H % h[i] || W % w[i]) return false;
        const int sh = H / h[i], sw = W / w[i];
        if (!loss_pow2(sh) || !loss_pow2(sw) || sh > kLossTile || sw > kLossTile || sh * sw < 4) return false;
        int k = i;
        while (k > 0 && (H / h[order[k - 1]]) * (W / w[order[k - 1]]) > sh * sw) {
            order[k] = order[k - 1];
            --k;
        }
        order[k] = i;
    }
    int cy = 1, cx = 1, ns = 0;
    for (int i = 0; i < n; ++i) {
        const int l = order[i], ty = H / h[l], tx = W / w[l];
        if (ty < cy || tx < cx || (ty == cy && tx == cx)) return false;   // not nested, or a repeated factor
        while (cy != ty || cx != tx) {
            const int ry = cy < ty ? 2 : 1, rx = cx < tx ? 2 : 1;
            cy *= ry;
            cx *= rx;
            lv.step_ry[ns] = ry;
            lv.step_rx[ns] = rx;
            lv.step_level[ns] = (cy == ty && cx == tx) ? l : -1;
            ++ns;
        }
    }
    lv.nsteps = ns;
    return true;
}

// Tile or pixel path -> the forward's workgroups along x = the partial sums per level, 0 < .. <= kLossTileBlocks;
// `tile`: the tile path, lv's steps filled.  gt_ok: the ground truth's 16-byte loads are allowed.
inline int loss_plan(int kind, bool gt_ok, int B, int H, int W, const int* h, const int* w, int n, LossLevels& lv,
                     bool& tile) {
    tile = kind == QPWC_LOSS_FLOW_MSE_V2 && gt_ok && loss_tile_plan(H, W, h, w, n, lv);
    if (!tile) return kLossPixBlocks;
    const int64_t ntiles = (int64_t)B * (H / kLossTile) * (W / kLossTile);
    return (int)(ntiles < kLossTileBlocks ? ntiles : kLossTileBlocks);
}

// the levels table but for its steps (loss_plan) and the masked extension
inline void loss_fill_levels(LossLevels& lv, int kind, int B, int H, int W, int C, const void* const* pred, const int* h,
                             const int* w, const int* pred_dtype, int n, void* const* dpred, void* const* gt_out) {
    // Huber and MSE: the mean over the last axis, then SUM_OVER_BATCH_SIZE -- for dense tensors the mean over every
    // element in both layouts; the two norm losses: the mean over pixels
    const bool per_element = kind == QPWC_LOSS_FLOW_MSE_V2 || kind == QPWC_LOSS_AUTORESIZE_MSE;
    for (int i = 0; i < n; ++i) {
        lv.pred[i] = pred[i];
        lv.dpred[i] = dpred ? (float*)dpred[i] : nullptr;
        lv.gt_out[i] = gt_out ? (float*)gt_out[i] : nullptr;
        lv.h[i] = h[i];
        lv.w[i] = w[i];
        lv.sh[i] = H / h[i];
        lv.sw[i] = W / w[i];
        lv.f16[i] = pred_dtype[i] == QPWC_F16;
        // h / H in fp32, as the reference's tf.cast(h) / tf.cast(H); AutoResizeMseLoss has no flow scale
        lv.fscale[i] = kind == QPWC_LOSS_AUTORESIZE_MSE ? 1.0f : (float)h[i] / (float)H;
        lv.inv_area[i] = lv.sh[i] > 0 && lv.sw[i] > 0 ? 1.0f / (float)(lv.sh[i] * lv.sw[i]) : 0.0f;
        const double pix = (double)B * h[i] * w[i];
        lv.inv_n[i] = (float)(1.0 / (per_element ? pix * C : pix));
        lv.lscale[i] = (float)(2.0 / ((double)w[i] + (double)h[i]));
        lv.ry_scale[i] = (float)H / (float)h[i];
        lv.rx_scale[i] = (float)W / (float)w[i];
    }
}

inline void loss_fill_grads(LossGradsBase& lg, const void* const* dpred, void* const* grad_pred, const int64_t* n_elems,
                            const int* pred_dtype, int n) {
    for (int i = 0; i < n; ++i) {
        lg.d[i] = (const float*)dpred[i];
        lg.g[i] = grad_pred[i];
        lg.n[i] = n_elems[i];
        lg.f16[i] = pred_dtype[i] == QPWC_F16;
    }
}

// The KIND x LAYOUT dispatch.  loss_launch: the NHWC or the NCHW instance of a kernel on kLossThreads threads;
// QPWC_LOSS_KIND(KERNEL, K, layout, grid, stream, args...): a switch case that launches KERNEL<K, layout>.
template <class... P, class... A>
inline void loss_launch(void (*nhwc)(P...), void (*nchw)(P...), int layout, dim3 grid, hipStream_t s, A... args) {
    hipLaunchKernelGGL(layout == QPWC_NHWC ? nhwc : nchw, grid, dim3(kLossThreads), 0, s, args...);
}
#define QPWC_LOSS_KIND(KERNEL, K, ...)                                          \
    case K:                                                                     \
        loss_launch(KERNEL<K, QPWC_NHWC>, KERNEL<K, QPWC_NCHW>, __VA_ARGS__);   \
        break

}  // namespace

}  // namespace qpwc

// What loss.hip (the dense losses) and masked_loss.hip (their valid-masked twins) share: the per-pixel term of the three
// flow losses and its derivative, the prediction loads, the pixel addressing, the wave sum and the tile path's sum-step
// plan.
#pragma once
#include "common.h"

namespace qpwc {

constexpr int kLossMaxLevels = 8;
constexpr int kLossMaxSteps = 10;       // tile path: 2x2 / 2x1 / 1x2 sum steps from 1x1 up to 32x32

typedef float loss_f32x4 __attribute__((ext_vector_type(4)));

namespace {

__device__ __forceinline__ float loss_wave_sum(float v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
    return v;
}

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

inline bool loss_pow2(int v) { return v > 0 && (v & (v - 1)) == 0; }

// The tile path's sum steps for these levels, or false when it does not apply: H, W multiples of the tile edge TILE (32);
// every factor a power of two <= TILE with sh * sw >= 4; the factors nested (ordered by area, each divides the next),
// none repeated.  LV: a levels struct with nsteps, step_ry, step_rx, step_level.
template <int TILE, class LV>
inline bool loss_tile_plan(int H, int W, const int* h, const int* w, int n, LV& lv) {
    if (H % TILE || W % TILE) return false;
    int order[kLossMaxLevels];
    for (int i = 0; i < n; ++i) {
        if (H % h[i] || W % w[i]) return false;
        const int sh = H / h[i], sw = W / w[i];
        if (!loss_pow2(sh) || !loss_pow2(sw) || sh > TILE || sw > TILE || sh * sw < 4) return false;
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

}  // namespace

}  // namespace qpwc

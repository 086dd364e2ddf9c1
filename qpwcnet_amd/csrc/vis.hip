// The trainer's flow panels (qpwcnet/core/vis.py:37-76 flow_to_image; app/train.py ShowImageCallback / train_custom:
// every flow coloured, nearest-resized to the label's size and converted for tf.summary.image), for up to 8 flows of
// different sizes in two launches (include/qpwc_vis.h):
//   flow_mag_max_kernel   one workgroup per (level, image, tile of 2048 source pixels) writes the tile's largest
//                         magnitude to the workspace;
//   flow_to_image_kernel  one workgroup per (level, image, tile of 1024 output pixels) folds the partials of its
//                         (level, image) -- 64 floats at 256x512 -- and colours its pixels, gathering each from its
//                         nearest source pixel.  In the <vec4> form the tile leaves through LDS in the output's own
//                         memory order: 16-byte stores for fp32, packed dwords for uint8.
// No atomics and no state between calls: a max does not depend on the order, two runs are bit-identical, and a captured
// graph replays both launches unchanged.  A workgroup's level is found from blockIdx.x by scalar code and every field of
// the by-value level table is then read at that uniform index (no per-lane selection).
#include <limits.h>

#include "../../include/qpwc_vis.h"
#include "launch.h"
#include "pixel_io.h"
#include "vis_common.h"

// (1 - s) + s * d and the hue are separately rounded products and sums, as include/qpwc_vis.h states them
#pragma clang fp contract(off)

namespace qpwc {

struct VisLevels {
    VisMaxLevels m;                              // the flows and their partials
    void* out[kVisMaxLevels];
    int h[kVisMaxLevels], w[kVisMaxLevels];      // the flow's own size
    int oh[kVisMaxLevels], ow[kVisMaxLevels];    // the picture's size
    float ry[kVisMaxLevels], rx[kVisMaxLevels];  // (float)h / oh, (float)w / ow
    int step_y[kVisMaxLevels], step_x[kVisMaxLevels];   // 256 output pixels further: 256 / ow rows and 256 % ow columns
    int ctiles[kVisMaxLevels];                   // colour tiles per image
    int cblk0[kVisMaxLevels];                    // the level's first workgroup of the colour launch
};                                               // unused levels: m.mblk0 = cblk0 = INT_MAX

namespace {

// the level of a workgroup: the last one whose first workgroup is not after it (scalar compares on blockIdx.x)
__device__ __forceinline__ int vis_level(const int* blk0, int bid) {
    int l = 0;
#pragma unroll
    for (int k = 1; k < kVisMaxLevels; ++k) l += bid >= blk0[k] ? 1 : 0;
    return l;
}

// tf.image.convert_image_dtype(uint8, saturate=True)
__device__ __forceinline__ uint8_t vis_u8(float x) { return (uint8_t)fminf(fmaxf(truncf(x * 255.5f), 0.0f), 255.0f); }

}  // namespace

constexpr int kVisPix = 4;                               // output pixels per lane of the colour launch
constexpr int kVisTile = kVisThreads * kVisPix;          // 1024

// blockIdx.x = mblk0[level] + image * mtiles[level] + tile; ws[blockIdx.x] = the tile's largest magnitude
template <int IN_LAYOUT>
__global__ __launch_bounds__(kVisThreads) void flow_mag_max_kernel(VisMaxLevels lv, float* __restrict__ ws) {
    __shared__ float red[kVisThreads / 64];
    const int bid = blockIdx.x;
    const int l = vis_level(lv.mblk0, bid);
    const int rel = bid - lv.mblk0[l], mt = lv.mtiles[l];
    const int n = rel / mt, tile = rel - n * mt;
    const int hw = lv.hw[l];
    const void* flow = lv.flow[l];
    const int f16 = lv.f16[l], pair = lv.pair[l];
    float m2 = 0.0f;
#pragma unroll
    for (int k = 0; k < kVisMaxPix; ++k) {
        const int pix = tile * kVisMaxTile + k * kVisThreads + (int)threadIdx.x;
        if (pix < hw) m2 = fmaxf(m2, vis_mag2(vis_load(flow, IN_LAYOUT == QPWC_NHWC, f16, pair, n, pix, hw)));
    }
    m2 = vis_block_max(m2, red);
    // the square root is monotone: the root of the largest square is the largest magnitude, bit for bit
    if (threadIdx.x == 0) ws[bid] = sqrtf(m2);
}

// blockIdx.x = cblk0[level] + image * ctiles[level] + tile; the tile's 1024 consecutive output pixels (row-major over
// oh x ow), lane t at pixels t, t + 256, t + 512, t + 768 of it.
template <int IN_LAYOUT, int OUT_LAYOUT, bool U8, bool VEC>
__global__ __launch_bounds__(kVisThreads) void flow_to_image_kernel(VisLevels lv, const float* __restrict__ ws) {
    __shared__ float red[kVisThreads / 64];
    using T = std::conditional_t<U8, uint8_t, float>;
    using Tile = TileStore<VEC, OUT_LAYOUT, 3, kVisTile, kVisThreads, T>;   // pixel_io.h
    __shared__ pix_f32x4 stage4[VEC ? kVisTile * 3 / (U8 ? 16 : 4) : 1];   // <vec4>: the tile in output order
    const int tid = threadIdx.x;
    const int bid = blockIdx.x;
    const int l = vis_level(lv.cblk0, bid);
    const int rel = bid - lv.cblk0[l], ct = lv.ctiles[l];
    const int n = rel / ct, tile = rel - n * ct;
    const int h = lv.h[l], w = lv.w[l], oh = lv.oh[l], ow = lv.ow[l];
    const int hw = h * w, ohw = oh * ow;
    const float ry = lv.ry[l], rx = lv.rx[l];
    const int step_y = lv.step_y[l], step_x = lv.step_x[l];
    const void* flow = lv.m.flow[l];
    const int f16 = lv.m.f16[l], pair = lv.m.pair[l];
    const float denom = vis_fold_max(ws, lv.m.mblk0[l], n, lv.m.mtiles[l], red) + 1e-6f;

    const int base = tile * kVisTile;       // first pixel of the tile
    const int64_t obase = (int64_t)n * ohw;  // first pixel of the image
    T* stage = reinterpret_cast<T*>(stage4);
    T* out = reinterpret_cast<T*>(lv.out[l]);

    // one division per lane: its further pixels lie 256 = step_y * ow + step_x pixels on
    int Y = (base + tid) / ow, X = (base + tid) - Y * ow;
#pragma unroll
    for (int k = 0; k < kVisPix; ++k, Y += step_y, X += step_x) {
        const int t = k * kVisThreads + tid, pix = base + t;
        if (X >= ow) {
            X -= ow;
            ++Y;
        }
        if (pix >= ohw) continue;
        const int sy = min((int)floorf(((float)Y + 0.5f) * ry), h - 1);
        const int sx = min((int)floorf(((float)X + 0.5f) * rx), w - 1);
        float rgb[3];
        vis_colour(vis_load(flow, IN_LAYOUT == QPWC_NHWC, f16, pair, n, sy * w + sx, hw), denom, rgb);
#pragma unroll
        for (int c = 0; c < 3; ++c)
            Tile::put(stage, out, obase, ohw, base, t, c, U8 ? (T)vis_u8(rgb[c]) : (T)rgb[c]);
    }
    if (!VEC) return;
    __syncthreads();
    Tile::flush(stage, out, obase, ohw, base, min(kVisTile, ohw - base));
}

// ---- host side ------------------------------------------------------------------------------------------------------

int flow_mag_max_launch(const VisMaxLevels& m, int blocks, int in_layout, float* ws, hipStream_t s) {
    dispatch_layout(in_layout, [&](auto I) {
        hipLaunchKernelGGL((flow_mag_max_kernel<decltype(I)::value>), dim3((unsigned)blocks), dim3(kVisThreads), 0, s, m, ws);
    });
    return check_launch("flow_mag_max_kernel");
}

// every count the launches index with fits 32 bits: 2 * B * h * w and 3 * B * oh * ow of each level (oh, ow may be
// NULL: the workspace query) and the workgroups of both launches
bool flow_to_image_shape_ok(int n, int B, const int* h, const int* w, const int* oh, const int* ow) {
    int64_t mblk = 0, cblk = 0;
    for (int l = 0; l < n; ++l) {
        if (2 * (int64_t)B * h[l] * w[l] > INT32_MAX) return false;
        mblk += B * ceil_div((int64_t)h[l] * w[l], kVisMaxTile);
        if (oh) {
            if (3 * (int64_t)B * oh[l] * ow[l] > INT32_MAX) return false;
            cblk += B * ceil_div((int64_t)oh[l] * ow[l], kVisTile);
        }
    }
    return mblk <= INT32_MAX && cblk <= INT32_MAX;
}

int64_t flow_to_image_workspace_floats(int n, int B, const int* h, const int* w) {
    int64_t f = 0;
    for (int l = 0; l < n; ++l) f += B * ceil_div((int64_t)h[l] * w[l], kVisMaxTile);
    return f;
}

static bool vis_vec(int n, const int* oh, const int* ow, const void* const* outs) {
    for (int l = 0; l < n; ++l)
        if (((int64_t)oh[l] * ow[l]) % 4 || (uintptr_t)outs[l] % 16) return false;
    return true;
}

const char* flow_to_image_fwd_kernel(int n, const int* oh, const int* ow, const void* const* outs) {
    return vis_vec(n, oh, ow, outs) ? "flow_to_image_kernel<vec4>" : "flow_to_image_kernel<scalar>";
}

int flow_to_image_fwd_launch(const void* const* flows, const int* f16, const int* h, const int* w, int n, int B,
                             int in_layout, void* const* outs, const int* oh, const int* ow, bool u8, int out_layout,
                             float* ws, hipStream_t s) {
    VisLevels lv = {};
    int mblk = 0, cblk = 0;
    for (int l = 0; l < kVisMaxLevels; ++l) {
        lv.m.mblk0[l] = lv.cblk0[l] = INT_MAX;
        if (l >= n) continue;
        lv.m.flow[l] = flows[l];
        lv.out[l] = outs[l];
        lv.h[l] = h[l];
        lv.w[l] = w[l];
        lv.oh[l] = oh[l];
        lv.ow[l] = ow[l];
        lv.m.f16[l] = f16[l];
        lv.m.pair[l] = in_layout == QPWC_NHWC && (uintptr_t)flows[l] % (f16[l] ? 4 : 8) == 0;
        lv.m.hw[l] = h[l] * w[l];
        lv.ry[l] = (float)h[l] / (float)oh[l];
        lv.rx[l] = (float)w[l] / (float)ow[l];
        lv.step_y[l] = kVisThreads / ow[l];
        lv.step_x[l] = kVisThreads % ow[l];
        lv.m.mtiles[l] = (int)ceil_div((int64_t)h[l] * w[l], kVisMaxTile);
        lv.ctiles[l] = (int)ceil_div((int64_t)oh[l] * ow[l], kVisTile);
        lv.m.mblk0[l] = mblk;
        lv.cblk0[l] = cblk;
        mblk += B * lv.m.mtiles[l];
        cblk += B * lv.ctiles[l];
    }
    const int rc = flow_mag_max_launch(lv.m, mblk, in_layout, ws, s);
    if (rc != QPWC_OK) return rc;

    const bool vec = vis_vec(n, oh, ow, outs);
    dispatch_layout(in_layout, [&](auto I) {
        dispatch_layout(out_layout, [&](auto O) {
            dispatch_bool(u8, [&](auto U) {
                dispatch_bool(vec, [&](auto V) {
                    hipLaunchKernelGGL((flow_to_image_kernel<decltype(I)::value, decltype(O)::value, decltype(U)::value,
                                                             decltype(V)::value>),
                                       dim3((unsigned)cblk), dim3(kVisThreads), 0, s, lv, (const float*)ws);
                });
            });
        });
    });
    return check_launch("flow_to_image_kernel");
}

}  // namespace qpwc

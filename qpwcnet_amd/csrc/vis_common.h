// flow_to_image's flow load, the table of its max launch, the fold of an image's partial maxima and the per-pixel
// colouring (include/qpwc_vis.h), shared by the trainer's flow panels (vis.hip) and the inference review panels
// (review.hip): one statement of the arithmetic, so that a flow's picture is the same bits whichever entry point draws it.
#pragma once
#include "common.h"

// (1 - s) + s * d and the hue are separately rounded products and sums, as include/qpwc_vis.h states them
#pragma clang fp contract(off)

namespace qpwc {

constexpr int kVisThreads = 256;
constexpr int kVisMaxPix = 8;                            // source pixels per lane of the max launch
constexpr int kVisMaxTile = kVisThreads * kVisMaxPix;    // 2048
constexpr int kVisMaxLevels = 8;

// What the max launch (flow_mag_max_kernel, vis.hip) reads of up to 8 flows, by value.  Level l's workgroups are
// mblk0[l] + image * mtiles[l] + tile, and each writes its tile's largest magnitude to the workspace at its own index.
struct VisMaxLevels {
    const void* flow[kVisMaxLevels];
    int f16[kVisMaxLevels];
    int pair[kVisMaxLevels];     // NHWC and the flow aligned to a whole pixel: one load per pixel
    int hw[kVisMaxLevels];       // pixels per image
    int mtiles[kVisMaxLevels];   // max-tiles per image
    int mblk0[kVisMaxLevels];    // the level's first workgroup = its first partial; unused levels: INT_MAX
};

namespace {

// (fx, fy) of pixel `pix` of image n of a (B,h,w,2) (nhwc) / (B,2,h,w) flow with hw pixels per image
__device__ __forceinline__ float2 vis_load(const void* flow, int nhwc, int f16, int pair, int64_t n, int pix, int hw) {
    if (nhwc) {
        const int64_t o = (n * hw + pix) * 2;
        if (f16) {
            const __half* p = reinterpret_cast<const __half*>(flow) + o;
            if (pair) return __half22float2(*reinterpret_cast<const __half2*>(p));
            return make_float2(__half2float(p[0]), __half2float(p[1]));
        }
        const float* p = reinterpret_cast<const float*>(flow) + o;
        if (pair) return *reinterpret_cast<const float2*>(p);
        return make_float2(p[0], p[1]);
    }
    const int64_t o = n * 2 * hw + pix;
    if (f16) {
        const __half* p = reinterpret_cast<const __half*>(flow) + o;
        return make_float2(__half2float(p[0]), __half2float(p[hw]));
    }
    const float* p = reinterpret_cast<const float*>(flow) + o;
    return make_float2(p[0], p[hw]);
}

// |f|^2 as both kernels form it: the colour kernel's magnitude never exceeds the maximum it is divided by
__device__ __forceinline__ float vis_mag2(float2 f) { return __fmaf_rn(f.x, f.x, f.y * f.y); }

__device__ __forceinline__ float vis_wave_max(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o));
    return v;
}

// the maximum of a workgroup's values, in every lane; `red` holds one float per wave
__device__ __forceinline__ float vis_block_max(float v, float* red) {
    v = vis_wave_max(v);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
}

// the largest magnitude of image n of a level, in every lane: the fold of its mt partials, which the max launch left
// from ws[blk0] on
__device__ __forceinline__ float vis_fold_max(const float* ws, int blk0, int n, int mt, float* red) {
    const float* part = ws + blk0 + (int64_t)n * mt;
    float m = 0.0f;
    for (int i = threadIdx.x; i < mt; i += kVisThreads) m = fmaxf(m, part[i]);
    return vis_block_max(m, red);
}

__device__ __forceinline__ float vis_clamp01(float v) { return fminf(fmaxf(v, 0.0f), 1.0f); }

// tf.image.hsv_to_rgb's functor at v = 1
__device__ __forceinline__ void vis_colour(float2 f, float denom, float* rgb) {
    const float pi = 3.1415927410125732f, two_pi = 6.2831854820251465f;   // float32(pi), float32(2 pi)
    const float hue = (atan2f(f.y, f.x) + pi) / two_pi;
    const float s = sqrtf(vis_mag2(f)) / denom;
    const float dh = 6.0f * hue;
    const float d[3] = {vis_clamp01(fabsf(dh - 3.0f) - 1.0f), vis_clamp01(2.0f - fabsf(dh - 2.0f)),
                        vis_clamp01(2.0f - fabsf(dh - 4.0f))};
#pragma unroll
    for (int c = 0; c < 3; ++c) rgb[c] = (1.0f - s) + s * d[c];
}

}  // namespace

}  // namespace qpwc

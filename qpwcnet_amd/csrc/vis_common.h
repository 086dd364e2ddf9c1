// flow_to_image's per-pixel colouring and the maximum of a tile's magnitudes (include/qpwc_vis.h), shared by the trainer's
// flow panels (vis.hip) and the inference review panels (review.hip): one statement of the arithmetic, so that a flow's
// picture is the same bits whichever entry point draws it.
#pragma once
#include "common.h"

// (1 - s) + s * d and the hue are separately rounded products and sums, as include/qpwc_vis.h states them
#pragma clang fp contract(off)

namespace qpwc {

constexpr int kVisThreads = 256;
constexpr int kVisMaxPix = 8;                            // source pixels per lane of the max launch
constexpr int kVisMaxTile = kVisThreads * kVisMaxPix;    // 2048

namespace {

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

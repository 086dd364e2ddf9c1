// What the input-pipeline kernels share (augment.hip, triplet.hip): the 256-pixel workgroup, tf.image.resize(BILINEAR)
// per axis (include/qpwc.h, qpwc_augment_fwd), the clamped source index and the source-pixel loads.
#pragma once
#include "common.h"

// a + (b - a) * t and u8 * (1/255) - 0.5 are separately rounded, as the reference's TF kernels round them
#pragma clang fp contract(off)

namespace qpwc {

constexpr int kAugThreads = 256;

namespace {

// index of floor / ceil of a source coordinate, clamped into the image whatever the parameters hold (NaN -> 0)
__device__ __forceinline__ int aug_index(float v, int n) { return (int)fminf(fmaxf(v, 0.0f), (float)(n - 1)); }

// one axis of tf.image.resize(BILINEAR) for output index i of `out` from `in` source pixels: half-pixel centres,
// scale = in / float(out), no antialias; the two clamped neighbours and the weight of the second
struct AugAxis {
    int lo, hi;
    float t;
};
__device__ __forceinline__ AugAxis aug_axis(int i, int in, int out) {
    const float s = ((float)i + 0.5f) * ((float)in / (float)out) - 0.5f;
    const float f = floorf(s);
    return {aug_index(f, in), aug_index(ceilf(s), in), s - f};
}

// columns, then rows
__device__ __forceinline__ float aug_lerp2(float a, float b, float c, float d, float tx, float ty) {
    const float top = a + (b - a) * tx;
    const float bot = c + (d - c) * tx;
    return top + (bot - top) * ty;
}

constexpr float kAugInv255 = 0.003921568859368563f;   // float32(1 / 255): a multiply, as train.py:56

// the 6 colour channels of source pixel `pix` of a two-frame image as fp32 in [0, 1]
template <bool U8>
__device__ __forceinline__ void aug_load_pixel(const void* ims, int64_t pix, float* v) {
    if (U8) {
        const uint16_t* p = reinterpret_cast<const uint16_t*>(reinterpret_cast<const uint8_t*>(ims) + pix * 6);
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            const unsigned w = p[i];
            v[2 * i] = (float)(w & 0xffu) * kAugInv255;
            v[2 * i + 1] = (float)(w >> 8) * kAugInv255;
        }
    } else {
        const float2* p = reinterpret_cast<const float2*>(reinterpret_cast<const float*>(ims) + pix * 6);
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            const float2 w = p[i];
            v[2 * i] = w.x;
            v[2 * i + 1] = w.y;
        }
    }
}

// the 3 colour channels of source pixel `pix` of a one-frame image: a uint8 pixel starts on any byte, an fp32 one on
// any dword
template <bool U8>
__device__ __forceinline__ void aug_load_rgb(const void* im, int64_t pix, float* v) {
    if (U8) {
        const uint8_t* p = reinterpret_cast<const uint8_t*>(im) + pix * 3;
#pragma unroll
        for (int i = 0; i < 3; ++i) v[i] = (float)p[i] * kAugInv255;
    } else {
        const float* p = reinterpret_cast<const float*>(im) + pix * 3;
#pragma unroll
        for (int i = 0; i < 3; ++i) v[i] = p[i];
    }
}

}  // namespace
}  // namespace qpwc

// Input pipeline of the frame interpolator (qpwcnet/data/triplet_dataset_ops.py read_and_resize / augment_triplet,
// data/augment.py photometric_augmentation, app/frame_interpolation/pre_train.py:110-124 preprocess), batched, in one
// launch: three uint8 (x 1/255) or fp32 frames per sample -> bilinear resize, one colour rotation / scale / offset and
// one field of Gaussian noise per sample for the three frames, flips, - 0.5, and the (first, last) pair and the middle
// frame written in the requested layout.  Every per-sample parameter is read from device memory.
//   One output pixel per lane, 256 pixels per workgroup (augment_pixel_kernel's launch shape).  A lane gathers the four
//   neighbours of its pixel in each frame (a 3-byte uint8 pixel is three 1-byte loads), draws its three normals from
//   Philox4x32-10 on the pixel's pre-flip index -- no noise tensor exists -- and, in the <vec4> form, the workgroup's
//   256 pixels leave through LDS in the outputs' own memory order as 16-byte stores.  No atomics: two runs are
//   bit-identical.
#include "../../include/qpwc_triplet.h"
#include "augment_common.h"
#include "launch.h"
#include "pixel_io.h"

namespace qpwc {

constexpr int kTriIParams = 4, kTriFParams = 16;

namespace {

// Philox4x32-10 (Salmon et al., SC'11) on counter (c0, 0, 0, 0)
__device__ __forceinline__ void tri_philox(uint32_t c0, uint32_t k0, uint32_t k1, uint32_t* r) {
    uint32_t c1 = 0, c2 = 0, c3 = 0;
#pragma unroll
    for (int i = 0; i < 10; ++i) {
        const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
        c1 = (uint32_t)p1;
        c3 = (uint32_t)p0;
        c0 = n0;
        c2 = n2;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    r[0] = c0;
    r[1] = c1;
    r[2] = c2;
    r[3] = c3;
}

// three standard normals (truncated at sqrt(48 ln 2)) from the four words: Box-Muller on u1 in (0, 1], u2 in [0, 1),
// both exact in fp32; cos and sin of the first pair, cos of the second (include/qpwc_triplet.h)
__device__ __forceinline__ void tri_normals(const uint32_t* r, float* z) {
    const float k = 5.9604644775390625e-8f, two_pi = 6.2831854820251465f;   // 2^-24, float32(2 pi)
    const float rad0 = sqrtf(-2.0f * logf((float)((r[0] >> 8) + 1u) * k));
    const float rad1 = sqrtf(-2.0f * logf((float)((r[2] >> 8) + 1u) * k));
    const float a0 = two_pi * ((float)(r[1] >> 8) * k), a1 = two_pi * ((float)(r[3] >> 8) * k);
    z[0] = rad0 * cosf(a0);
    z[1] = rad0 * sinf(a0);
    z[2] = rad1 * cosf(a1);
}

}  // namespace

// blockIdx.x = sample * nblk + chunk; the chunk's 256 consecutive pixels (row-major over the h x w output), one per lane.
template <bool U8, int LAYOUT, bool VEC>
__global__ __launch_bounds__(kAugThreads) void triplet_pixel_kernel(const void* __restrict__ fa,
                                                                   const void* __restrict__ fb,
                                                                   const void* __restrict__ fc, int H, int W,
                                                                   const int* __restrict__ iparams,
                                                                   const float* __restrict__ fparams, int h, int w,
                                                                   int nblk, int flags, float* __restrict__ out_pair,
                                                                   float* __restrict__ out_mid) {
    __shared__ pix_f32x4 stage4[kAugThreads * 9 / 4];   // <vec4>: the chunk in output order, pair then middle (9 KB)
    const int tid = threadIdx.x;
    const int b = blockIdx.x / nblk, chunk = blockIdx.x - b * nblk;
    const int hw = h * w;
    const int base = chunk * kAugThreads;                // first pixel of the chunk
    const int pix = base + tid;
    const bool valid = pix < hw;
    const float offset = (flags & QPWC_TRIPLET_RAW) ? 0.0f : 0.5f;

    const int* ip = iparams + (int64_t)b * kTriIParams;
    const float* fp = fparams + (int64_t)b * kTriFParams;

    float v[9];   // first frame, last frame, middle frame
#pragma unroll
    for (int c = 0; c < 9; ++c) v[c] = 0.0f;
    if (valid) {
        const int y = pix / w, x = pix - y * w;
        // the pixel's coordinate before the flips: the reference resizes, adds the noise and flips last
        const int sy = ip[0] ? h - 1 - y : y, sx = ip[1] ? w - 1 - x : x;
        const AugAxis ay = aug_axis(sy, H, h), ax = aug_axis(sx, W, w);
        const int64_t img = (int64_t)b * H * W;
        const int64_t p00 = img + (int64_t)ay.lo * W + ax.lo, p01 = img + (int64_t)ay.lo * W + ax.hi;
        const int64_t p10 = img + (int64_t)ay.hi * W + ax.lo, p11 = img + (int64_t)ay.hi * W + ax.hi;

        uint32_t r[4];
        float n[3];
        tri_philox((uint32_t)(sy * w + sx), (uint32_t)ip[2], (uint32_t)ip[3], r);
        tri_normals(r, n);
        const float sigma = fp[15];
#pragma unroll
        for (int c = 0; c < 3; ++c) n[c] *= sigma;

        const void* frames[3] = {fa, fc, fb};   // v's order
#pragma unroll
        for (int f = 0; f < 3; ++f) {
            float a[3], bb[3], c_[3], d[3], rgb[3];
            aug_load_rgb<U8>(frames[f], p00, a);
            aug_load_rgb<U8>(frames[f], p01, bb);
            aug_load_rgb<U8>(frames[f], p10, c_);
            aug_load_rgb<U8>(frames[f], p11, d);
#pragma unroll
            for (int c = 0; c < 3; ++c) rgb[c] = aug_lerp2(a[c], bb[c], c_[c], d[c], ax.t, ay.t);
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const float rot = (fp[3 * c] * rgb[0] + fp[3 * c + 1] * rgb[1]) + fp[3 * c + 2] * rgb[2];
                v[3 * f + c] = ((rot * fp[9 + c] + fp[12 + c]) + n[c]) - offset;
            }
        }
    }

    // the pair, then the middle frame: element by element, or <vec4> through LDS (pixel_io.h)
    using Pair = TileStore<VEC, LAYOUT, 6, kAugThreads, kAugThreads, float>;
    using Mid = TileStore<VEC, LAYOUT, 3, kAugThreads, kAugThreads, float>;
    const int64_t obase = (int64_t)b * hw;
    float* spair = reinterpret_cast<float*>(stage4);
    float* smid = spair + Pair::kElems;
    if (VEC || valid) {
#pragma unroll
        for (int c = 0; c < 6; ++c) Pair::put(spair, out_pair, obase, hw, base, tid, c, v[c]);
#pragma unroll
        for (int c = 0; c < 3; ++c) Mid::put(smid, out_mid, obase, hw, base, tid, c, v[6 + c]);
    }
    if (!VEC) return;
    __syncthreads();
    const int n = min(kAugThreads, hw - base);
    Pair::flush(spair, out_pair, obase, hw, base, n);
    Mid::flush(smid, out_mid, obase, hw, base, n);
}

// ---- host side ------------------------------------------------------------------------------------------------------

static bool tri_vec(int h, int w, const void* out_pair, const void* out_mid) {
    return ((int64_t)h * w) % 4 == 0 && (uintptr_t)out_pair % 16 == 0 && (uintptr_t)out_mid % 16 == 0;
}

const char* augment_triplet_fwd_kernel(int h, int w, const void* out_pair, const void* out_mid) {
    return tri_vec(h, w, out_pair, out_mid) ? "triplet_pixel_kernel<vec4>" : "triplet_pixel_kernel<scalar>";
}

int augment_triplet_fwd_launch(const void* a, const void* b, const void* c, bool u8, int B, int H, int W,
                               const int* iparams, const float* fparams, int h, int w, int flags, int layout,
                               float* out_pair, float* out_mid, hipStream_t s) {
    const int nblk = (int)ceil_div((int64_t)h * w, kAugThreads);
    const bool vec = tri_vec(h, w, out_pair, out_mid);
    const dim3 grid((unsigned)(B * nblk)), block(kAugThreads);
    dispatch_bool(u8, [&](auto U) {
        dispatch_layout(layout, [&](auto L) {
            dispatch_bool(vec, [&](auto V) {
                hipLaunchKernelGGL((triplet_pixel_kernel<decltype(U)::value, decltype(L)::value, decltype(V)::value>), grid,
                                   block, 0, s, a, b, c, H, W, iparams, fparams, h, w, nblk, flags, out_pair, out_mid);
            });
        });
    });
    return check_launch("triplet_pixel_kernel");
}

}  // namespace qpwc

// Training input pipeline (qpwcnet/data/augment.py:83-173, app/optical_flow/train.py:54-94), batched: uint8 -> x 1/255,
// flips, bilinear scale + crop, flow scaling, brightness / saturation / hue / contrast, - 0.5, NaN scrub and the layout
// change, with every per-sample parameter read from device memory.
//   pass 1 (augment_pixel_kernel): one output pixel per lane, 256 pixels per workgroup: flips, the four-neighbour
//           gather of all 8 channels, flow scaling and the per-pixel colour stages.  With the colour stage on it
//           writes the pre-contrast image and leaves the workgroup's sums of the three colour channels in the workspace;
//           with it off it writes the final image.  The flow is final either way.  (Flag QPWC_AUGMENT_RAW leaves out
//           the - 0.5 and the scrub: image_augment / image_resize on their own.)
//   pass 2 (augment_contrast_kernel): folds a sample's partial sums in a fixed order, then contrast, - 0.5 and the NaN
//           scrub in place.
// Lanes of a wave read neighbouring source pixels (a 6-byte uint8 pixel is three 2-byte loads: pixel addresses are even,
// never dword aligned) and, in the <vec4> form, the workgroup's 256 pixels leave through LDS in the output's own memory
// order as 16-byte stores.  No atomics: two runs are bit-identical.
// Sparse ground truth (augment_sparse_pixel_kernel, include/qpwc_sparse_augment.h) is the same pass 1 with another flow
// rule: the four flow corners and their mask bytes are loaded like the frames', the invalid ones are selected out, the
// rest are weighted over their own sum, and the pixel's validity leaves as a byte beside the flow.  A gather: every
// output pixel is written once, by the lane that owns it.
#include "augment_common.h"
#include "launch.h"
#include "pixel_io.h"

namespace qpwc {

constexpr int kAugPass2Pixels = 4096;   // pass 2: pixels of one sample per workgroup
constexpr int kAugIParams = 6, kAugFParams = 6;

namespace {

__device__ __forceinline__ float aug_wave_sum(float v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
    return v;
}

__device__ __forceinline__ float clip01(float v) { return fminf(fmaxf(v, 0.0f), 1.0f); }

// adjust_brightness, adjust_saturation and adjust_hue of one RGB pixel.  The reference makes two HSV round trips; the
// second RGB -> HSV returns the first one's (h, s', v) (s' = range' / v' and the hue of the rebuilt pixel are those it
// was built from, and a pixel with v <= 0 or s' = 0 is grey on both), so one round trip with both edits is the same
// function.  A NaN channel makes the pixel NaN.
__device__ __forceinline__ void aug_colour(float& r, float& g, float& b, float bright, float sat, float hue) {
    r += bright;
    g += bright;
    b += bright;
    const bool nan = r != r || g != g || b != b;
    const float mx = fmaxf(r, fmaxf(g, b)), mn = fminf(r, fminf(g, b));
    const float range = mx - mn, v = mx;
    float s = v > 0.0f ? range / v : 0.0f;
    float h = 0.0f;
    if (range > 0.0f) {
        const float norm = 1.0f / (6.0f * range);
        h = r == mx ? norm * (g - b) : (g == mx ? norm * (b - r) + 2.0f / 6.0f : norm * (r - g) + 4.0f / 6.0f);
        if (h < 0.0f) h += 1.0f;
    }
    s = clip01(s * sat);
    h += hue;
    h -= floorf(h);
    const float dr = clip01(fabsf(6.0f * h - 3.0f) - 1.0f);
    const float dg = clip01(2.0f - fabsf(6.0f * h - 2.0f));
    const float db = clip01(2.0f - fabsf(6.0f * h - 4.0f));
    const float q = nan ? __builtin_nanf("") : v;
    r = ((dr - 1.0f) * s + 1.0f) * q;
    g = ((dg - 1.0f) * s + 1.0f) * q;
    b = ((db - 1.0f) * s + 1.0f) * q;
}

__device__ __forceinline__ float aug_scrub(float v) { return v != v ? 0.0f : v; }

constexpr float kAugFlowUnknown = 1e9f;   // a flow component above it in magnitude marks the pixel unknown

// The flow of one output pixel from its four corners (00, 01, 10, 11) over the valid ones only
// (include/qpwc_sparse_augment.h): ok[k] = both components within kAugFlowUnknown and the mask byte non-zero.  An
// invalid corner's components are replaced before any arithmetic sees them.  Four valid corners give aug_lerp2's value;
// fewer the weighted sum over the sum of the valid weights, which is positive where there is one; none 0.
// Returns the number of valid corners.
__device__ __forceinline__ int aug_sparse_flow(const float2* f, const unsigned* m, float tx, float ty, float& u, float& v) {
    bool ok[4];
    float fx[4], fy[4];
    int n = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        ok[k] = fabsf(f[k].x) <= kAugFlowUnknown && fabsf(f[k].y) <= kAugFlowUnknown && m[k] != 0;   // NaN: false
        fx[k] = ok[k] ? f[k].x : 0.0f;
        fy[k] = ok[k] ? f[k].y : 0.0f;
        n += ok[k] ? 1 : 0;
    }
    const float ly0 = 1.0f - ty, lx0 = 1.0f - tx;
    const float wgt[4] = {ly0 * lx0, ly0 * tx, ty * lx0, ty * tx};
    float S = 0.0f, su = 0.0f, sv = 0.0f;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const float wk = ok[k] ? wgt[k] : 0.0f;
        S += wk;
        su += wk * fx[k];
        sv += wk * fy[k];
    }
    const float du = aug_lerp2(fx[0], fx[1], fx[2], fx[3], tx, ty), dv = aug_lerp2(fy[0], fy[1], fy[2], fy[3], tx, ty);
    const float safe = n > 0 ? S : 1.0f;                 // n = 0: 0 / 1
    u = n == 4 ? du : su / safe;
    v = n == 4 ? dv : sv / safe;
    return n;
}

}  // namespace

// Pass 1 of both pipelines.  blockIdx.x = sample * nblk + chunk; the chunk's 256 consecutive pixels (row-major over the
// h x w output), one per lane.  SPARSE: the flow over its valid corners and out_valid; MASKED: `valid` is given.
template <bool U8, int LAYOUT, bool VEC, bool SPARSE, bool MASKED>
__device__ __forceinline__ void aug_pixel_pass(const void* __restrict__ ims, const float* __restrict__ flo,
                                               const uint8_t* __restrict__ valid_in, int H, int W,
                                               const int* __restrict__ iparams, const float* __restrict__ fparams,
                                               int h, int w, int nblk, int flags, float* __restrict__ out_ims,
                                               float* __restrict__ out_flo, uint8_t* __restrict__ out_valid,
                                               float* __restrict__ partial) {
    __shared__ pix_f32x4 stage4[kAugThreads * 8 / 4];   // <vec4>: the chunk in output order, image then flow (8 KB)
    __shared__ uint32_t stagem[SPARSE && VEC ? kAugThreads / 4 : 1];   // <vec4>, sparse: the chunk's mask bytes
    __shared__ float red[3][kAugThreads / 64];
    const int tid = threadIdx.x;
    const int b = blockIdx.x / nblk, chunk = blockIdx.x - b * nblk;
    const int hw = h * w;
    const bool colour = flags & QPWC_AUGMENT_COLOR, raw = flags & QPWC_AUGMENT_RAW;
    const int base = chunk * kAugThreads;                // first pixel of the chunk
    const int pix = base + tid;
    const bool valid = pix < hw;

    const int* ip = iparams + (int64_t)b * kAugIParams;
    const float* fp = fparams + (int64_t)b * kAugFParams;
    const int rh = ip[0], rw = ip[1], oy = ip[2], ox = ip[3], flip_ud = ip[4], flip_lr = ip[5];
    const float mu = fp[0], mv = fp[1], bright = fp[2], sat = fp[3], hue = fp[4];

    float v[8];
#pragma unroll
    for (int c = 0; c < 8; ++c) v[c] = 0.0f;
    int corners = 0;                                     // sparse: the pixel's valid flow corners
    if (valid) {
        const int y = pix / w, x = pix - y * w;
        const AugAxis ay = aug_axis(oy + y, H, rh), ax = aug_axis(ox + x, W, rw);
        const float ty = ay.t, tx = ax.t;
        int y0 = ay.lo, y1 = ay.hi, x0 = ax.lo, x1 = ax.hi;
        if (flip_ud) {
            y0 = H - 1 - y0;
            y1 = H - 1 - y1;
        }
        if (flip_lr) {
            x0 = W - 1 - x0;
            x1 = W - 1 - x1;
        }
        const int64_t img = (int64_t)b * H * W;
        const int64_t p00 = img + (int64_t)y0 * W + x0, p01 = img + (int64_t)y0 * W + x1;
        const int64_t p10 = img + (int64_t)y1 * W + x0, p11 = img + (int64_t)y1 * W + x1;
        float a[8], bb[8], c_[8], d[8];
        aug_load_pixel<U8>(ims, p00, a);
        aug_load_pixel<U8>(ims, p01, bb);
        aug_load_pixel<U8>(ims, p10, c_);
        aug_load_pixel<U8>(ims, p11, d);
        const float2* f2 = reinterpret_cast<const float2*>(flo);
        const float2 fa = f2[p00], fb = f2[p01], fc = f2[p10], fd = f2[p11];
        a[6] = fa.x; a[7] = fa.y;
        bb[6] = fb.x; bb[7] = fb.y;
        c_[6] = fc.x; c_[7] = fc.y;
        d[6] = fd.x; d[7] = fd.y;
#pragma unroll
        for (int c = 0; c < (SPARSE ? 6 : 8); ++c) v[c] = aug_lerp2(a[c], bb[c], c_[c], d[c], tx, ty);
        if (SPARSE) {
            // the four mask bytes are loaded like the flow corners, whatever they will be selected to
            const float2 fk[4] = {fa, fb, fc, fd};
            unsigned mk[4] = {1u, 1u, 1u, 1u};
            if (MASKED) {
                mk[0] = valid_in[p00];
                mk[1] = valid_in[p01];
                mk[2] = valid_in[p10];
                mk[3] = valid_in[p11];
            }
            corners = aug_sparse_flow(fk, mk, tx, ty, v[6], v[7]);
        }
        v[6] *= mu;
        v[7] *= mv;
        if (SPARSE && corners == 0) v[6] = v[7] = 0.0f;   // + 0 whatever the multipliers' signs
        if (!SPARSE && !raw) {
            v[6] = aug_scrub(v[6]);
            v[7] = aug_scrub(v[7]);
        }
        if (colour) {
            aug_colour(v[0], v[1], v[2], bright, sat, hue);
            aug_colour(v[3], v[4], v[5], bright, sat, hue);
        } else if (!raw) {
#pragma unroll
            for (int c = 0; c < 6; ++c) v[c] = aug_scrub(v[c] - 0.5f);
        }
    }

    if (colour) {
        // sums of the three colour channels over both frames (an invalid lane holds zeros), lanes then waves in order
        const int lane = tid & 63, wid = tid >> 6;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const float s = aug_wave_sum(v[c] + v[c + 3]);
            if (lane == 0) red[c][wid] = s;
        }
        __syncthreads();
        if (tid < 3) partial[((int64_t)b * 3 + tid) * nblk + chunk] = (red[tid][0] + red[tid][1]) + (red[tid][2] + red[tid][3]);
    }

    // the image, then the flow: element by element, or <vec4> through LDS (pixel_io.h)
    using Ims = TileStore<VEC, LAYOUT, 6, kAugThreads, kAugThreads, float>;
    using Flo = TileStore<VEC, LAYOUT, 2, kAugThreads, kAugThreads, float>;
    const int64_t obase = (int64_t)b * hw;
    float* sims = reinterpret_cast<float*>(stage4);
    float* sflo = sims + Ims::kElems;
    if (VEC || valid) {
#pragma unroll
        for (int c = 0; c < 6; ++c) Ims::put(sims, out_ims, obase, hw, base, tid, c, v[c]);
#pragma unroll
        for (int c = 0; c < 2; ++c) Flo::put(sflo, out_flo, obase, hw, base, tid, c, v[6 + c]);
    }
    using Msk = TileStore<VEC, LAYOUT, 1, kAugThreads, kAugThreads, uint8_t>;
    uint8_t* smsk = reinterpret_cast<uint8_t*>(stagem);
    if (SPARSE && (VEC || valid)) Msk::put(smsk, out_valid, obase, hw, base, tid, 0, (uint8_t)(corners > 0));
    if (!VEC) return;
    __syncthreads();
    const int n = min(kAugThreads, hw - base);
    Ims::flush(sims, out_ims, obase, hw, base, n);
    Flo::flush(sflo, out_flo, obase, hw, base, n);
    if (SPARSE) Msk::flush(smsk, out_valid, obase, hw, base, n);
}

template <bool U8, int LAYOUT, bool VEC>
__global__ __launch_bounds__(kAugThreads) void augment_pixel_kernel(const void* __restrict__ ims,
                                                                   const float* __restrict__ flo, int H, int W,
                                                                   const int* __restrict__ iparams,
                                                                   const float* __restrict__ fparams, int h, int w,
                                                                   int nblk, int flags, float* __restrict__ out_ims,
                                                                   float* __restrict__ out_flo,
                                                                   float* __restrict__ partial) {
    aug_pixel_pass<U8, LAYOUT, VEC, false, false>(ims, flo, nullptr, H, W, iparams, fparams, h, w, nblk, flags, out_ims,
                                                  out_flo, nullptr, partial);
}

template <bool U8, int LAYOUT, bool VEC, bool MASKED>
__global__ __launch_bounds__(kAugThreads) void augment_sparse_pixel_kernel(
    const void* __restrict__ ims, const float* __restrict__ flo, const uint8_t* __restrict__ valid, int H, int W,
    const int* __restrict__ iparams, const float* __restrict__ fparams, int h, int w, int nblk, int flags,
    float* __restrict__ out_ims, float* __restrict__ out_flo, uint8_t* __restrict__ out_valid,
    float* __restrict__ partial) {
    aug_pixel_pass<U8, LAYOUT, VEC, true, MASKED>(ims, flo, valid, H, W, iparams, fparams, h, w, nblk, flags, out_ims,
                                                  out_flo, out_valid, partial);
}

// blockIdx.x = sample * nblk2 + chunk of kAugPass2Pixels pixels: adjust_contrast with the mean of each colour channel
// over both frames, then (unless raw) - 0.5 and NaN -> 0, in place.
template <int LAYOUT, bool VEC>
__global__ __launch_bounds__(kAugThreads) void augment_contrast_kernel(float* __restrict__ out_ims,
                                                                      const float* __restrict__ partial,
                                                                      const float* __restrict__ fparams, int h, int w,
                                                                      int nblk, int nblk2, int raw) {
    __shared__ float red[3][kAugThreads / 64];
    __shared__ float mean_s[3];
    const int tid = threadIdx.x;
    const int b = blockIdx.x / nblk2, chunk = blockIdx.x - b * nblk2;
    const int hw = h * w;
    const int lane = tid & 63, wid = tid >> 6;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float* p = partial + ((int64_t)b * 3 + c) * nblk;
        float s = 0.0f;
        for (int i = tid; i < nblk; i += kAugThreads) s += p[i];
        s = aug_wave_sum(s);
        if (lane == 0) red[c][wid] = s;
    }
    __syncthreads();
    if (tid < 3) mean_s[tid] = ((red[tid][0] + red[tid][1]) + (red[tid][2] + red[tid][3])) / (2.0f * (float)hw);
    __syncthreads();
    const float m0 = mean_s[0], m1 = mean_s[1], m2 = mean_s[2];
    const float factor = fparams[(int64_t)b * kAugFParams + 5];
    auto fin = [&](float x, int c) -> float {
        const float m = c == 0 ? m0 : (c == 1 ? m1 : m2);
        const float r = (x - m) * factor + m;
        return raw ? r : aug_scrub(r - 0.5f);
    };
    float* img = out_ims + (int64_t)b * hw * 6;
    const int64_t e0 = (int64_t)chunk * kAugPass2Pixels * 6;
    const int64_t e1 = min(e0 + (int64_t)kAugPass2Pixels * 6, (int64_t)hw * 6);
    if (VEC) {
        pix_f32x4* p4 = reinterpret_cast<pix_f32x4*>(img);
        for (int64_t i = e0 / 4 + tid; i < e1 / 4; i += kAugThreads) {
            pix_f32x4 x = p4[i];
            if (LAYOUT == QPWC_NHWC) {
                const int c = (int)((4 * i) % 6);   // 0, 4 or 2
                x.x = fin(x.x, c % 3);
                x.y = fin(x.y, (c + 1) % 3);
                x.z = fin(x.z, (c + 2) % 3);
                x.w = fin(x.w, c % 3);
            } else {
                const int c = (int)(((4 * i) / hw) % 3);   // hw % 4 == 0: one plane
                x.x = fin(x.x, c);
                x.y = fin(x.y, c);
                x.z = fin(x.z, c);
                x.w = fin(x.w, c);
            }
            p4[i] = x;
        }
        return;
    }
    for (int64_t i = e0 + tid; i < e1; i += kAugThreads) {
        const int c = LAYOUT == QPWC_NHWC ? (int)(i % 3) : (int)((i / hw) % 3);
        img[i] = fin(img[i], c);
    }
}

// ---- host side ------------------------------------------------------------------------------------------------------

static int64_t aug_nblk(int h, int w) { return ceil_div((int64_t)h * w, kAugThreads); }

// 3 partial sums per pass-1 workgroup
int64_t augment_workspace_floats(int B, int h, int w) { return 3 * (int64_t)B * aug_nblk(h, w); }

// both grids are one-dimensional over sample x chunk
bool augment_shape_ok(int B, int H, int W, int h, int w) {
    const int64_t lim = 0x7fffffff;
    return (int64_t)H * W <= lim && (int64_t)h * w <= lim / 6 && (int64_t)B * aug_nblk(h, w) <= lim;
}

static bool aug_vec(int h, int w, const void* out_ims, const void* out_flo) {
    return ((int64_t)h * w) % 4 == 0 && (uintptr_t)out_ims % 16 == 0 && (uintptr_t)out_flo % 16 == 0;
}

// pass 2 of both pipelines
static int aug_contrast_launch(int B, const float* fparams, int h, int w, int nblk, int flags, int layout, bool vec,
                               float* out_ims, const float* ws, hipStream_t s) {
    const int nblk2 = (int)ceil_div((int64_t)h * w, kAugPass2Pixels);
    const dim3 grid2((unsigned)(B * nblk2)), block(kAugThreads);
    dispatch_layout(layout, [&](auto L) {
        dispatch_bool(vec, [&](auto V) {
            hipLaunchKernelGGL((augment_contrast_kernel<decltype(L)::value, decltype(V)::value>), grid2, block, 0, s,
                               out_ims, ws, fparams, h, w, nblk, nblk2, flags & QPWC_AUGMENT_RAW);
        });
    });
    return check_launch("augment_contrast_kernel");
}

const char* augment_fwd_kernel(int h, int w, const void* out_ims, const void* out_flo) {
    return aug_vec(h, w, out_ims, out_flo) ? "augment_pixel_kernel<vec4>" : "augment_pixel_kernel<scalar>";
}

int augment_fwd_launch(const void* ims, bool u8, const float* flo, int B, int H, int W, const int* iparams,
                       const float* fparams, int h, int w, int flags, int layout, float* out_ims, float* out_flo,
                       float* ws, hipStream_t s) {
    const int nblk = (int)aug_nblk(h, w);
    const bool vec = aug_vec(h, w, out_ims, out_flo);
    const dim3 grid((unsigned)(B * nblk)), block(kAugThreads);
    dispatch_bool(u8, [&](auto U) {
        dispatch_layout(layout, [&](auto L) {
            dispatch_bool(vec, [&](auto V) {
                hipLaunchKernelGGL((augment_pixel_kernel<decltype(U)::value, decltype(L)::value, decltype(V)::value>), grid,
                                   block, 0, s, ims, flo, H, W, iparams, fparams, h, w, nblk, flags, out_ims, out_flo, ws);
            });
        });
    });
    const int rc = check_launch("augment_pixel_kernel");
    if (rc != QPWC_OK || !(flags & QPWC_AUGMENT_COLOR)) return rc;
    return aug_contrast_launch(B, fparams, h, w, nblk, flags, layout, vec, out_ims, ws, s);
}

// the sparse pipeline's form follows from the shape alone: qpwc_augment_sparse_fwd refuses outputs off its grid
static bool aug_sparse_vec(int h, int w) { return ((int64_t)h * w) % 4 == 0; }

const char* augment_sparse_fwd_kernel(int h, int w) {
    return aug_sparse_vec(h, w) ? "augment_sparse_pixel_kernel<vec4>" : "augment_sparse_pixel_kernel<scalar>";
}

size_t augment_sparse_out_align(int h, int w) { return aug_sparse_vec(h, w) ? 16 : 4; }

int augment_sparse_fwd_launch(const void* ims, bool u8, const float* flo, const unsigned char* valid, int B, int H, int W,
                              const int* iparams, const float* fparams, int h, int w, int flags, int layout,
                              float* out_ims, float* out_flo, unsigned char* out_valid, float* ws, hipStream_t s) {
    const int nblk = (int)aug_nblk(h, w);
    const bool vec = aug_sparse_vec(h, w);
    const dim3 grid((unsigned)(B * nblk)), block(kAugThreads);
    dispatch_bool(u8, [&](auto U) {
        dispatch_layout(layout, [&](auto L) {
            dispatch_bool(vec, [&](auto V) {
                dispatch_bool(valid != nullptr, [&](auto M) {
                    hipLaunchKernelGGL((augment_sparse_pixel_kernel<decltype(U)::value, decltype(L)::value,
                                                                    decltype(V)::value, decltype(M)::value>),
                                       grid, block, 0, s, ims, flo, valid, H, W, iparams, fparams, h, w, nblk, flags,
                                       out_ims, out_flo, out_valid, ws);
                });
            });
        });
    });
    const int rc = check_launch("augment_sparse_pixel_kernel");
    if (rc != QPWC_OK || !(flags & QPWC_AUGMENT_COLOR)) return rc;
    return aug_contrast_launch(B, fparams, h, w, nblk, flags, layout, vec, out_ims, ws, s);
}

}  // namespace qpwc

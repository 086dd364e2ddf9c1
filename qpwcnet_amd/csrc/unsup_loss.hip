// The label-free flow losses (include/qpwc_unsup_loss.h): census or Charbonnier photometric term between prv and nxt
// warped by the flow, masked where the sample leaves the image or is occluded, plus edge-aware first-order smoothness.
//   forward : one launch for all levels (unsup_loss_fwd_kernel), a workgroup per (level, image, tile of 8 x 32 pixels)
//             found through the per-level prefix table in the kernel arguments; the tile's prv grey and warped grey are
//             staged in LDS with the 3-pixel halo (14 x 38 cells each, 4.2 KB), every thread walks the 48 offsets of its
//             pixel, and the workgroup writes its three partial sums and its count; + one fixed-order fold
//             (unsup_loss_fold_kernel).  The forward saves per pixel what the backward needs -- m q (dist + eps)^(q-1),
//             both greys, d gw / d q, the two edge weights -- so that the backward's halo stays 3;
//   backward: one launch on the same grid (unsup_loss_bwd_kernel): a gather.  With G(p,d) = d dist_p / d gw(p+d), the pair
//             (r, -d) in which r is the centre has G(r,-d) = -G(r-d,d) (both ternaries change sign with D, the factor
//             0.81 / (0.81 + D^2)^1.5 does not), so d photo / d gw(r) = sum_d (s_{r-d} + s_r) G(r-d,d) / count: 48 terms
//             serve both the 48 pairs in which r is a neighbour and the 48 in which it is the centre.
// Deterministic: grids depend on the shapes only, fixed-order sums, no atomics.  Every global access is element-wise: no
// form depends on an address.
#include "common.h"
#include "launch.h"
#include "../../include/qpwc_unsup_loss.h"

namespace qpwc {

constexpr int kUnsupThreads = 256;
constexpr int kUnsupTileH = 8, kUnsupTileW = 32;   // a half-wave reads one row of 32 consecutive LDS cells: no conflict
constexpr int kUnsupHalo = 3;
constexpr int kUnsupRows = kUnsupTileH + 2 * kUnsupHalo, kUnsupCols = kUnsupTileW + 2 * kUnsupHalo;
constexpr int kUnsupCells = kUnsupRows * kUnsupCols;
constexpr int kUnsupMaxLevels = 8;
constexpr int kUnsupPlanes = 7;                    // saved per pixel: s, g(prv), gw, dgx, dgy, wx, wy
constexpr int kUnsupWaves = kUnsupThreads / 64;
static_assert(kUnsupThreads == kUnsupTileH * kUnsupTileW, "one thread per pixel of the tile");

struct UnsupLevels {
    const float* prv[kUnsupMaxLevels];
    const float* nxt[kUnsupMaxLevels];
    const void* flow[kUnsupMaxLevels];
    const unsigned char* occ[kUnsupMaxLevels];   // NULL: nothing occluded
    void* grad[kUnsupMaxLevels];                 // backward: d loss / d flow
    float* planes[kUnsupMaxLevels];              // the level's 7 saved planes of B * h * w floats
    int h[kUnsupMaxLevels], w[kUnsupMaxLevels], f16[kUnsupMaxLevels];
    int tiles_x[kUnsupMaxLevels], tiles_y[kUnsupMaxLevels];
    int tile_start[kUnsupMaxLevels + 1];         // prefix sums of B * tiles_y * tiles_x
};

namespace {

template <class T>
__device__ __forceinline__ T unsup_wave_sum(T v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
    return v;
}

// the workgroup's (level, image, tile origin)
struct UnsupTile {
    int l, b, y0, x0;
};
__device__ __forceinline__ UnsupTile unsup_tile(const UnsupLevels& lv, int n_levels) {
    const int bid = blockIdx.x;
    UnsupTile t;
    t.l = 0;
    for (int k = 1; k < n_levels; ++k)
        if (bid >= lv.tile_start[k]) t.l = k;
    int i = bid - lv.tile_start[t.l];
    const int tx = i % lv.tiles_x[t.l];
    i /= lv.tiles_x[t.l];
    t.y0 = (i % lv.tiles_y[t.l]) * kUnsupTileH;
    t.b = i / lv.tiles_y[t.l];
    t.x0 = tx * kUnsupTileW;
    return t;
}

template <int LAYOUT>
__device__ __forceinline__ float2 unsup_ld_flow(const void* f, int f16, int64_t b, int y, int x, int h, int w) {
    const int64_t o = LAYOUT == QPWC_NHWC ? ((b * h + y) * w + x) * 2 : (b * 2 * h + y) * (int64_t)w + x;
    const int64_t cs = LAYOUT == QPWC_NHWC ? 1 : (int64_t)h * w;
    if (f16) {
        const __half* p = reinterpret_cast<const __half*>(f);
        return make_float2(__half2float(p[o]), __half2float(p[o + cs]));
    }
    const float* p = reinterpret_cast<const float*>(f);
    return make_float2(p[o], p[o + cs]);
}

template <int LAYOUT>
__device__ __forceinline__ void unsup_st_flow(void* g, int f16, int64_t b, int y, int x, int h, int w, float gu, float gv) {
    const int64_t o = LAYOUT == QPWC_NHWC ? ((b * h + y) * w + x) * 2 : (b * 2 * h + y) * (int64_t)w + x;
    const int64_t cs = LAYOUT == QPWC_NHWC ? 1 : (int64_t)h * w;
    if (f16) {
        __half* p = reinterpret_cast<__half*>(g);
        p[o] = __float2half_rn(gu);
        p[o + cs] = __float2half_rn(gv);
    } else {
        float* p = reinterpret_cast<float*>(g);
        p[o] = gu;
        p[o + cs] = gv;
    }
}

struct Rgb {
    float r, g, b;
};
__device__ __forceinline__ Rgb unsup_ld_rgb(const float* img, int64_t b, int y, int x, int h, int w) {
    const float* p = img + ((b * h + y) * w + x) * 3;
    return Rgb{p[0], p[1], p[2]};
}

__device__ __forceinline__ float unsup_grey(Rgb c) {
#pragma clang fp contract(off)
    return 255.0f * ((0.2989f * c.r + 0.587f * c.g) + 0.114f * c.b);
}

// The CLAMP taps of one sample point: taps_clamp (common.h) with the second tap held inside an axis of extent 1.
struct UnsupTaps {
    int y0, y1, x0, x1;
    float ay, ax;
    bool inside;
};
__device__ __forceinline__ UnsupTaps unsup_taps(int y, int x, float u, float v, int h, int w) {
#pragma clang fp contract(off)
    UnsupTaps t;
    const float qy = (float)y + v, qx = (float)x + u;
    const float fl_y = fminf(fmaxf(0.0f, floorf(qy)), (float)max(h - 2, 0));
    const float fl_x = fminf(fmaxf(0.0f, floorf(qx)), (float)max(w - 2, 0));
    t.y0 = (int)fl_y;
    t.x0 = (int)fl_x;
    t.y1 = min(t.y0 + 1, h - 1);
    t.x1 = min(t.x0 + 1, w - 1);
    t.ay = fminf(fmaxf(0.0f, qy - fl_y), 1.0f);
    t.ax = fminf(fmaxf(0.0f, qx - fl_x), 1.0f);
    t.inside = qx >= 0.0f && qx <= (float)(w - 1) && qy >= 0.0f && qy <= (float)(h - 1);
    return t;
}

// value, d / d qx and d / d qy of the blend of four corner values; the derivatives are those of the bilinear form (the
// caller zeroes them where the sample is outside the image)
__device__ __forceinline__ float unsup_blend(const UnsupTaps& t, float tl, float tr, float bl, float br, float& dx, float& dy) {
#pragma clang fp contract(off)
    const float top = t.ax * (tr - tl) + tl;
    const float bot = t.ax * (br - bl) + bl;
    dx = (1.0f - t.ay) * (tr - tl) + t.ay * (br - bl);
    dy = bot - top;
    return t.ay * (bot - top) + top;
}

// nxt's grey sampled at (x, y) + flow: the value and its two derivatives
template <int LAYOUT>
__device__ __forceinline__ float unsup_warp_grey(const UnsupLevels& lv, int l, int64_t b, int y, int x, float& dx, float& dy,
                                                 bool& inside) {
    const int h = lv.h[l], w = lv.w[l];
    const float2 f = unsup_ld_flow<LAYOUT>(lv.flow[l], lv.f16[l], b, y, x, h, w);
    const UnsupTaps t = unsup_taps(y, x, f.x, f.y, h, w);
    const float* nxt = lv.nxt[l];
    const float tl = unsup_grey(unsup_ld_rgb(nxt, b, t.y0, t.x0, h, w)), tr = unsup_grey(unsup_ld_rgb(nxt, b, t.y0, t.x1, h, w));
    const float bl = unsup_grey(unsup_ld_rgb(nxt, b, t.y1, t.x0, h, w)), br = unsup_grey(unsup_ld_rgb(nxt, b, t.y1, t.x1, h, w));
    inside = t.inside;
    return unsup_blend(t, tl, tr, bl, br, dx, dy);
}

// sqrt(D^2 + eps^2) of one flow difference
__device__ __forceinline__ float unsup_robust(float d, float eps_s) { return sqrtf(d * d + eps_s * eps_s); }

}  // namespace

template <int KIND, int LAYOUT>
__global__ __launch_bounds__(kUnsupThreads) void unsup_loss_fwd_kernel(UnsupLevels lv, int n_levels, int B, float q,
                                                                     float eps, float edge, float eps_s,
                                                                     float* __restrict__ part) {
    __shared__ float sgp[kUnsupCells], sgw[kUnsupCells];
    __shared__ float red[3][kUnsupWaves];
    __shared__ int redn[kUnsupWaves];
    const UnsupTile t = unsup_tile(lv, n_levels);
    const int l = t.l, h = lv.h[l], w = lv.w[l];
    const int64_t b = t.b;
    const int tid = threadIdx.x, ty = tid / kUnsupTileW, tx = tid % kUnsupTileW;
    const int y = t.y0 + ty, x = t.x0 + tx;
    const bool in_image = y < h && x < w;
    const int64_t np = (int64_t)B * h * w;
    float* const planes = lv.planes[l];
    const int64_t pix = (b * h + y) * (int64_t)w + x;

    if constexpr (KIND == QPWC_UNSUP_CENSUS) {
        for (int c = tid; c < kUnsupCells; c += kUnsupThreads) {
            const int cy = t.y0 - kUnsupHalo + c / kUnsupCols, cx = t.x0 - kUnsupHalo + c % kUnsupCols;
            float gp = 0.0f, gw = 0.0f;
            if (cy >= 0 && cy < h && cx >= 0 && cx < w) {
                float dx, dy;
                bool inside;
                gp = unsup_grey(unsup_ld_rgb(lv.prv[l], b, cy, cx, h, w));
                gw = unsup_warp_grey<LAYOUT>(lv, l, b, cy, cx, dx, dy, inside);
            }
            sgp[c] = gp;
            sgw[c] = gw;
        }
        __syncthreads();
    }

    float term = 0.0f, sx = 0.0f, sy = 0.0f;
    int cnt = 0;
    if (in_image) {
        const float2 f = unsup_ld_flow<LAYOUT>(lv.flow[l], lv.f16[l], b, y, x, h, w);
        const Rgb p0 = unsup_ld_rgb(lv.prv[l], b, y, x, h, w);
        const bool occluded = lv.occ[l] && lv.occ[l][pix] != 0;
        float s = 0.0f, gp0 = 0.0f, gw0 = 0.0f, dgx = 0.0f, dgy = 0.0f;
        if constexpr (KIND == QPWC_UNSUP_CENSUS) {
            bool inside;
            gp0 = unsup_grey(p0);
            gw0 = unsup_warp_grey<LAYOUT>(lv, l, b, y, x, dgx, dgy, inside);
            dgx = inside ? dgx : 0.0f;
            dgy = inside ? dgy : 0.0f;
            const bool m = inside && !occluded && x >= kUnsupHalo && x < w - kUnsupHalo && y >= kUnsupHalo && y < h - kUnsupHalo;
            float dist = 0.0f;
#pragma unroll
            for (int dy = 0; dy < 7; ++dy) {
#pragma unroll
                for (int dx = 0; dx < 7; ++dx) {
                    if (dy == kUnsupHalo && dx == kUnsupHalo) continue;
                    const int c = (ty + dy) * kUnsupCols + tx + dx;
                    const float a = sgp[c] - gp0, bb = sgw[c] - gw0;
                    const float tp = a * rsqrtf(0.81f + a * a), tw = bb * rsqrtf(0.81f + bb * bb);
                    const float df = tp - tw, e = df * df;
                    dist += e / (0.1f + e);
                }
            }
            const float base = dist + eps;
            const float tm = powf(base, q);
            term = m ? tm : 0.0f;
            s = m ? q * tm / base : 0.0f;
            cnt = m ? 1 : 0;
        } else {
            const UnsupTaps tp = unsup_taps(y, x, f.x, f.y, h, w);
            const bool m = tp.inside && !occluded;
            const Rgb tl = unsup_ld_rgb(lv.nxt[l], b, tp.y0, tp.x0, h, w), tr = unsup_ld_rgb(lv.nxt[l], b, tp.y0, tp.x1, h, w);
            const Rgb bl = unsup_ld_rgb(lv.nxt[l], b, tp.y1, tp.x0, h, w), br = unsup_ld_rgb(lv.nxt[l], b, tp.y1, tp.x1, h, w);
            const float pc[3] = {p0.r, p0.g, p0.b};
            const float ctl[3] = {tl.r, tl.g, tl.b}, ctr[3] = {tr.r, tr.g, tr.b};
            const float cbl[3] = {bl.r, bl.g, bl.b}, cbr[3] = {br.r, br.g, br.b};
            float tsum = 0.0f;
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                float wx_, wy_;
                const float wv = unsup_blend(tp, ctl[c], ctr[c], cbl[c], cbr[c], wx_, wy_);
                const float d = pc[c] - wv;
                const float base = d * d + eps * eps;
                const float tc = powf(base, q);
                tsum += tc;
                const float k = -(q * tc / base) * (2.0f * d) * (1.0f / 3.0f);   // d term / d warped_c
                dgx += k * wx_;
                dgy += k * wy_;
            }
            term = m ? tsum * (1.0f / 3.0f) : 0.0f;
            dgx = m ? dgx : 0.0f;
            dgy = m ? dgy : 0.0f;
            cnt = m ? 1 : 0;
        }
        // edge-aware smoothness towards the right and the lower neighbour
        float wxv = 0.0f, wyv = 0.0f;
        if (x + 1 < w) {
            const Rgb p1 = unsup_ld_rgb(lv.prv[l], b, y, x + 1, h, w);
            const float2 f1 = unsup_ld_flow<LAYOUT>(lv.flow[l], lv.f16[l], b, y, x + 1, h, w);
            wxv = expf(-edge * ((fabsf(p1.r - p0.r) + fabsf(p1.g - p0.g) + fabsf(p1.b - p0.b)) * (1.0f / 3.0f)));
            sx = wxv * unsup_robust(f1.x - f.x, eps_s) + wxv * unsup_robust(f1.y - f.y, eps_s);
        }
        if (y + 1 < h) {
            const Rgb p1 = unsup_ld_rgb(lv.prv[l], b, y + 1, x, h, w);
            const float2 f1 = unsup_ld_flow<LAYOUT>(lv.flow[l], lv.f16[l], b, y + 1, x, h, w);
            wyv = expf(-edge * ((fabsf(p1.r - p0.r) + fabsf(p1.g - p0.g) + fabsf(p1.b - p0.b)) * (1.0f / 3.0f)));
            sy = wyv * unsup_robust(f1.x - f.x, eps_s) + wyv * unsup_robust(f1.y - f.y, eps_s);
        }
        planes[pix] = s;
        planes[np + pix] = gp0;
        planes[2 * np + pix] = gw0;
        planes[3 * np + pix] = dgx;
        planes[4 * np + pix] = dgy;
        planes[5 * np + pix] = wxv;
        planes[6 * np + pix] = wyv;
    }

    const int lane = tid & 63, wid = tid >> 6;
    term = unsup_wave_sum(term);
    sx = unsup_wave_sum(sx);
    sy = unsup_wave_sum(sy);
    cnt = unsup_wave_sum(cnt);
    if (lane == 0) {
        red[0][wid] = term;
        red[1][wid] = sx;
        red[2][wid] = sy;
        redn[wid] = cnt;
    }
    __syncthreads();
    if (tid < 3) part[(int64_t)blockIdx.x * 4 + tid] = (red[tid][0] + red[tid][1]) + (red[tid][2] + red[tid][3]);
    if (tid == 3) reinterpret_cast<int*>(part)[(int64_t)blockIdx.x * 4 + 3] = (redn[0] + redn[1]) + (redn[2] + redn[3]);
}

// Level blockIdx.x: its tiles' partial sums and counts in a fixed order, in double; then the three means and the total.
__global__ __launch_bounds__(kUnsupThreads) void unsup_loss_fold_kernel(UnsupLevels lv, int B, float smooth_weight,
                                                                      const float* __restrict__ part,
                                                                      float* __restrict__ out_losses,
                                                                      float* __restrict__ out_photo,
                                                                      float* __restrict__ out_smooth,
                                                                      int64_t* __restrict__ out_counts) {
    __shared__ double red[3][kUnsupWaves];
    __shared__ long long redn[kUnsupWaves];
    const int l = blockIdx.x;
    double s[3] = {0.0, 0.0, 0.0};
    long long c = 0;
    for (int i = lv.tile_start[l] + threadIdx.x; i < lv.tile_start[l + 1]; i += kUnsupThreads) {
        s[0] += part[(int64_t)i * 4];
        s[1] += part[(int64_t)i * 4 + 1];
        s[2] += part[(int64_t)i * 4 + 2];
        c += reinterpret_cast<const int*>(part)[(int64_t)i * 4 + 3];
    }
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        s[k] = unsup_wave_sum(s[k]);
        if (lane == 0) red[k][wid] = s[k];
    }
    c = unsup_wave_sum(c);
    if (lane == 0) redn[wid] = c;
    __syncthreads();
    if (threadIdx.x == 0) {
        const int h = lv.h[l], w = lv.w[l];
        const long long count = (redn[0] + redn[1]) + (redn[2] + redn[3]);
        double tot[3];
        for (int k = 0; k < 3; ++k) tot[k] = (red[k][0] + red[k][1]) + (red[k][2] + red[k][3]);
        const double photo = tot[0] / (double)(count > 0 ? count : 1);
        const double nx = 2.0 * B * h * (double)(w - 1), ny = 2.0 * B * (double)(h - 1) * w;
        const double smooth = 0.5 * ((w > 1 ? tot[1] / nx : 0.0) + (h > 1 ? tot[2] / ny : 0.0));
        out_counts[l] = count;
        out_photo[l] = (float)photo;
        out_smooth[l] = (float)smooth;
        out_losses[l] = (float)(photo + (double)smooth_weight * smooth);
    }
}

template <int KIND, int LAYOUT>
__global__ __launch_bounds__(kUnsupThreads) void unsup_loss_bwd_kernel(UnsupLevels lv, int n_levels, int B,
                                                                     float smooth_weight, float eps_s,
                                                                     const int64_t* __restrict__ counts,
                                                                     const float* __restrict__ grad_losses) {
    __shared__ float ss[kUnsupCells], sgp[kUnsupCells], sgw[kUnsupCells];
    const UnsupTile t = unsup_tile(lv, n_levels);
    const int l = t.l, h = lv.h[l], w = lv.w[l];
    const int64_t b = t.b;
    const int tid = threadIdx.x, ty = tid / kUnsupTileW, tx = tid % kUnsupTileW;
    const int y = t.y0 + ty, x = t.x0 + tx;
    const int64_t np = (int64_t)B * h * w;
    const float* const planes = lv.planes[l];

    if constexpr (KIND == QPWC_UNSUP_CENSUS) {
        for (int c = tid; c < kUnsupCells; c += kUnsupThreads) {
            const int cy = t.y0 - kUnsupHalo + c / kUnsupCols, cx = t.x0 - kUnsupHalo + c % kUnsupCols;
            float s = 0.0f, gp = 0.0f, gw = 0.0f;
            if (cy >= 0 && cy < h && cx >= 0 && cx < w) {
                const int64_t o = (b * h + cy) * (int64_t)w + cx;
                s = planes[o];
                gp = planes[np + o];
                gw = planes[2 * np + o];
            }
            ss[c] = s;
            sgp[c] = gp;
            sgw[c] = gw;
        }
        __syncthreads();
    }
    if (y >= h || x >= w) return;

    const int64_t pix = (b * h + y) * (int64_t)w + x;
    const int64_t count = counts[l];
    const float gl = grad_losses[l];
    float c_r = 1.0f;
    if constexpr (KIND == QPWC_UNSUP_CENSUS) {
        const int c0 = (ty + kUnsupHalo) * kUnsupCols + tx + kUnsupHalo;
        const float s0 = ss[c0], gp0 = sgp[c0], gw0 = sgw[c0];
        c_r = 0.0f;
#pragma unroll
        for (int dy = 0; dy < 7; ++dy) {
#pragma unroll
            for (int dx = 0; dx < 7; ++dx) {
                if (dy == kUnsupHalo && dx == kUnsupHalo) continue;
                // the centre p = r - d: D = g(r) - g(p)
                const int c = (ty + 2 * kUnsupHalo - dy) * kUnsupCols + tx + 2 * kUnsupHalo - dx;
                const float a = gp0 - sgp[c], bb = gw0 - sgw[c];
                const float rw = rsqrtf(0.81f + bb * bb);
                const float tp = a * rsqrtf(0.81f + a * a), tw = bb * rw;
                const float df = tp - tw, e = df * df, den = 0.1f + e;
                // d dist_p / d gw(r) = phi'(e) * d e / d t_w * d t_w / d D
                const float g = (0.1f / (den * den)) * (-2.0f * df) * (0.81f * (rw * rw * rw));
                c_r += (ss[c] + s0) * g;
            }
        }
    }
    const float inv = (float)((double)gl / (double)(count > 0 ? count : 1));
    float gu = (inv * c_r) * planes[3 * np + pix], gv = (inv * c_r) * planes[4 * np + pix];

    if (smooth_weight > 0.0f) {
        const float2 f = unsup_ld_flow<LAYOUT>(lv.flow[l], lv.f16[l], b, y, x, h, w);
        const float kx = w > 1 ? (float)((double)gl * 0.5 * smooth_weight / (2.0 * B * h * (double)(w - 1))) : 0.0f;
        const float ky = h > 1 ? (float)((double)gl * 0.5 * smooth_weight / (2.0 * B * (double)(h - 1) * w)) : 0.0f;
        float su = 0.0f, sv = 0.0f;
        auto pair = [&](int yy, int xx, float wgt, float sign, float k) {   // the difference f(yy, xx) - f(y, x), signed
            const float2 fn = unsup_ld_flow<LAYOUT>(lv.flow[l], lv.f16[l], b, yy, xx, h, w);
            const float du = sign * (fn.x - f.x), dv = sign * (fn.y - f.y);   // D of the pair, later minus earlier
            // this pixel is the earlier one (sign = +1): d / d f = -psi(D); the later one: +psi(D)
            su += -sign * k * wgt * (du / unsup_robust(du, eps_s));
            sv += -sign * k * wgt * (dv / unsup_robust(dv, eps_s));
        };
        if (x + 1 < w) pair(y, x + 1, planes[5 * np + pix], 1.0f, kx);
        if (x > 0) pair(y, x - 1, planes[5 * np + pix - 1], -1.0f, kx);
        if (y + 1 < h) pair(y + 1, x, planes[6 * np + pix], 1.0f, ky);
        if (y > 0) pair(y - 1, x, planes[6 * np + pix - w], -1.0f, ky);
        gu += su;
        gv += sv;
    }
    unsup_st_flow<LAYOUT>(lv.grad[l], lv.f16[l], b, y, x, h, w, gu, gv);
}

// ---- host side ------------------------------------------------------------------------------------------------------

// tiles of level (h, w) over the batch
static int64_t unsup_level_tiles(int B, int h, int w) {
    return (int64_t)B * ((h + kUnsupTileH - 1) / kUnsupTileH) * ((w + kUnsupTileW - 1) / kUnsupTileW);
}

int64_t unsup_loss_total_tiles(int B, const int* h, const int* w, int n) {
    int64_t tiles = 0;
    for (int i = 0; i < n; ++i) tiles += unsup_level_tiles(B, h[i], w[i]);
    return tiles;
}

// floats: 4 per tile, then 7 planes per level
int64_t unsup_loss_workspace_floats(int B, const int* h, const int* w, int n) {
    int64_t pixels = 0;
    for (int i = 0; i < n; ++i) pixels += (int64_t)B * h[i] * w[i];
    return 4 * unsup_loss_total_tiles(B, h, w, n) + kUnsupPlanes * pixels;
}

const char* unsup_loss_fwd_kernel(int kind) {
    return kind == QPWC_UNSUP_CENSUS ? "unsup_loss_fwd_kernel<census>" : "unsup_loss_fwd_kernel<charbonnier>";
}

static void unsup_fill(UnsupLevels& lv, int B, const int* h, const int* w, const int* flow_dtype, int n,
                       const void* const* flow, float* ws) {
    float* planes = ws + 4 * unsup_loss_total_tiles(B, h, w, n);
    lv.tile_start[0] = 0;
    for (int i = 0; i < n; ++i) {
        lv.flow[i] = flow[i];
        lv.h[i] = h[i];
        lv.w[i] = w[i];
        lv.f16[i] = flow_dtype[i] == QPWC_F16;
        lv.tiles_y[i] = (h[i] + kUnsupTileH - 1) / kUnsupTileH;
        lv.tiles_x[i] = (w[i] + kUnsupTileW - 1) / kUnsupTileW;
        lv.tile_start[i + 1] = lv.tile_start[i] + (int)unsup_level_tiles(B, h[i], w[i]);
        lv.planes[i] = planes;
        planes += (int64_t)kUnsupPlanes * B * h[i] * w[i];
    }
}

template <class... P, class... A>
static void unsup_launch(void (*nhwc)(P...), void (*nchw)(P...), int layout, int grid, hipStream_t s, A... args) {
    hipLaunchKernelGGL(layout == QPWC_NHWC ? nhwc : nchw, dim3(grid), dim3(kUnsupThreads), 0, s, args...);
}

int unsup_loss_fwd_launch(int kind, float q, float eps, float smooth_weight, float edge, float eps_s,
                          const void* const* prv, const void* const* nxt, const void* const* flow,
                          const void* const* occluded, int B, const int* h, const int* w, const int* flow_dtype,
                          int layout, int n, float* out_losses, float* out_photo, float* out_smooth, int64_t* out_counts,
                          float* ws, hipStream_t s) {
    UnsupLevels lv = {};
    unsup_fill(lv, B, h, w, flow_dtype, n, flow, ws);
    for (int i = 0; i < n; ++i) {
        lv.prv[i] = (const float*)prv[i];
        lv.nxt[i] = (const float*)nxt[i];
        lv.occ[i] = occluded ? (const unsigned char*)occluded[i] : nullptr;
    }
    const int grid = lv.tile_start[n];
    if (kind == QPWC_UNSUP_CENSUS)
        unsup_launch(unsup_loss_fwd_kernel<QPWC_UNSUP_CENSUS, QPWC_NHWC>, unsup_loss_fwd_kernel<QPWC_UNSUP_CENSUS, QPWC_NCHW>,
                     layout, grid, s, lv, n, B, q, eps, edge, eps_s, ws);
    else
        unsup_launch(unsup_loss_fwd_kernel<QPWC_UNSUP_CHARBONNIER, QPWC_NHWC>,
                     unsup_loss_fwd_kernel<QPWC_UNSUP_CHARBONNIER, QPWC_NCHW>, layout, grid, s, lv, n, B, q, eps, edge,
                     eps_s, ws);
    const int rc = check_launch(unsup_loss_fwd_kernel(kind));
    if (rc != QPWC_OK) return rc;
    hipLaunchKernelGGL(unsup_loss_fold_kernel, dim3(n), dim3(kUnsupThreads), 0, s, lv, B, smooth_weight, ws, out_losses,
                       out_photo, out_smooth, out_counts);
    return check_launch("unsup_loss_fold_kernel");
}

int unsup_loss_bwd_launch(int kind, float smooth_weight, float eps_s, const void* const* flow, const float* ws,
                          const int64_t* counts, const float* grad_losses, void* const* grad_flow, int B, const int* h,
                          const int* w, const int* flow_dtype, int layout, int n, hipStream_t s) {
    UnsupLevels lv = {};
    unsup_fill(lv, B, h, w, flow_dtype, n, flow, const_cast<float*>(ws));
    for (int i = 0; i < n; ++i) lv.grad[i] = grad_flow[i];
    const int grid = lv.tile_start[n];
    if (kind == QPWC_UNSUP_CENSUS)
        unsup_launch(unsup_loss_bwd_kernel<QPWC_UNSUP_CENSUS, QPWC_NHWC>, unsup_loss_bwd_kernel<QPWC_UNSUP_CENSUS, QPWC_NCHW>,
                     layout, grid, s, lv, n, B, smooth_weight, eps_s, counts, grad_losses);
    else
        unsup_launch(unsup_loss_bwd_kernel<QPWC_UNSUP_CHARBONNIER, QPWC_NHWC>,
                     unsup_loss_bwd_kernel<QPWC_UNSUP_CHARBONNIER, QPWC_NCHW>, layout, grid, s, lv, n, B, smooth_weight, eps_s,
                     counts, grad_losses);
    return check_launch("unsup_loss_bwd_kernel");
}

}  // namespace qpwc

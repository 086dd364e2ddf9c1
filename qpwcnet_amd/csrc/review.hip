// The inference review panels (include/qpwc_review.h): every picture qpwcnet/app/optical_flow/test_infer.py:104-154
// (set 1, ten pictures) and qpwcnet/app/frame_interpolation/pre_train_test.py:45-79, 121-163 (set 2, seven pictures, the
// alignment grid and the 8-bit export) show for a batch, in two launches:
//   flow_mag_max_kernel    vis.hip's, with the one or two flows as its levels: one workgroup per (flow, image, tile of
//                          2048 flow pixels) writes the tile's largest magnitude to the workspace;
//   review_panels_kernel   one workgroup per (image, tile of 256 pixels), one lane per pixel: the lane reads its image
//                          values and flows, gathers the corners of its tf_warp samples (2 x 4 x 3 values in set 1,
//                          4 x 3 in set 2), folds the partials of its image and writes its pixel of every picture: 30
//                          values in set 1, 18 in set 2.  Set 2's flow picture has the flow's own size: a tail of the
//                          grid, one workgroup per (image, tile of 256 flow pixels), colours it.
// The stores are the cost.  In the <vec4> form a workgroup's pixels leave through LDS in each picture's own memory order
// (channels-last pictures have 12-byte pixels): 16-byte stores for fp32, packed dwords for uint8.  The form follows from
// the shape alone (every picture's pixel count a multiple of 4); the boundary demands the alignment it needs, so no
// pointer's low bits are looked at here.  No atomics and no state between calls: two runs are bit-identical and a
// captured graph replays both launches unchanged.  The sampling rule is common.h's taps_tfwarp / blend, the flow load,
// the fold and the colouring vis_common.h's, the tile store pixel_io.h's: the code of qpwc_warp_fwd and
// qpwc_flow_to_image_fwd, not a copy of it.
#include <limits.h>

#include "../../include/qpwc_review.h"
#include "launch.h"
#include "pixel_io.h"
#include "vis_common.h"

// every product and sum of include/qpwc_review.h is rounded separately
#pragma clang fp contract(off)

namespace qpwc {

constexpr int kRevTile = kVisThreads;    // pixels per workgroup of the panel launch, one per lane

struct RevArgs {
    const void* img[3];      // set 1: ims; set 2: img_pair, img1, pred
    const float* flow[2];    // set 1: flo, flo_pred; set 2: flow
    void* out[10];           // set 1: the ten pictures in order; set 2: 0-prv .. 4-overlay, 6-warp, then 5-flow
    int B, H, W, h, w, s;    // pictures H x W; set 2: flow h x w, H = s * h, W = s * w
    int f16, nhwc;           // the images are fp16; the inputs are channels-last
    int grid;
    int mtiles;              // max-tiles per image and flow
    int tiles;               // panel tiles per image of the H x W pictures
    int ftiles;              // set 2: panel tiles per image of the flow picture
};

namespace {

__device__ __forceinline__ float rev_ld(const void* img, int f16, int64_t at) {
    return f16 ? __half2float(reinterpret_cast<const __half*>(img)[at]) : reinterpret_cast<const float*>(img)[at];
}

// _show's export: (255 * np.clip(x, 0, 1)).astype(np.uint8)
__device__ __forceinline__ uint8_t rev_u8(float x) { return (uint8_t)truncf(255.0f * fminf(fmaxf(x, 0.0f), 1.0f)); }

// tf_warp of 3 channels of image n at pixel (Y, X); ib: the image's first element, ps / cs: its pixel and channel strides
__device__ __forceinline__ void rev_warp3(const void* img, int f16, int64_t ib, int ps, int64_t cs, int Y, int X,
                                          float2 f, int H, int W, float* out) {
    const Taps t = taps_tfwarp(Y, X, f.x, f.y, H, W);
    const int64_t tl = ib + ((int64_t)t.y0 * W + t.x0) * ps, tr = ib + ((int64_t)t.y0 * W + t.x1) * ps;
    const int64_t bl = ib + ((int64_t)t.y1 * W + t.x0) * ps, br = ib + ((int64_t)t.y1 * W + t.x1) * ps;
#pragma unroll
    for (int c = 0; c < 3; ++c)
        out[c] = blend<QPWC_WARP_TFWARP>(t, rev_ld(img, f16, tl + c * cs), rev_ld(img, f16, tr + c * cs),
                                         rev_ld(img, f16, bl + c * cs), rev_ld(img, f16, br + c * cs));
}

// The lane's pixel base + threadIdx.x of NP pictures of ohw = oh * ow pixels per image: the grid, the conversion and the
// stores.  outs[p]: (B,oh,ow,3) / (B,3,oh,ow).  Every lane of the workgroup calls it (<vec4> has a barrier).
template <int OUT_LAYOUT, bool U8, bool VEC, int NP>
__device__ __forceinline__ void rev_emit(const float (&v)[NP][3], void* const* outs, int n, int base, int ohw, int ow,
                                         int grid, pix_f32x4* stage4) {
    using T = std::conditional_t<U8, uint8_t, float>;
    using Tile = TileStore<VEC, OUT_LAYOUT, 3, kRevTile, kVisThreads, T>;   // pixel_io.h; a picture's tile
    const int tid = threadIdx.x, pix = base + tid;
    const int64_t obase = (int64_t)n * ohw;   // first pixel of the image
    T* stage = reinterpret_cast<T*>(stage4);
    if (pix < ohw) {
        bool line = false;
        if (grid > 0) {
            const int Y = pix / ow, X = pix - Y * ow;
            line = Y % grid == 0 || X % grid == 0;
        }
#pragma unroll
        for (int p = 0; p < NP; ++p) {
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const float x = line ? 1.0f : v[p][c];
                Tile::put(stage + p * Tile::kElems, reinterpret_cast<T*>(outs[p]), obase, ohw, base, tid, c,
                          U8 ? (T)rev_u8(x) : (T)x);
            }
        }
    }
    if (!VEC) return;
    // the pictures' alignment is the boundary's demand: it refuses an output off the piece's grid
    __syncthreads();
    const int cnt = min(kRevTile, ohw - base);
#pragma unroll
    for (int p = 0; p < NP; ++p) Tile::flush(stage + p * Tile::kElems, reinterpret_cast<T*>(outs[p]), obase, ohw, base, cnt);
}

}  // namespace

// The partials of flow k lie from ws[k * B * mtiles] on (the max launch: flow_mag_max_kernel, vis.hip).
// blockIdx.x = image * tiles + tile for the H x W pictures; SET 2: from B * tiles on, image * ftiles + tile of 5-flow.
// Lane t owns pixel tile * 256 + t (row-major).
template <int SET, int OUT_LAYOUT, bool U8, bool VEC>
__global__ __launch_bounds__(kVisThreads) void review_panels_kernel(RevArgs a, const float* __restrict__ ws) {
    constexpr int NP = SET == 1 ? 10 : 6;
    __shared__ float red[2][kVisThreads / 64];
    __shared__ pix_f32x4 stage4[VEC ? NP * kRevTile * 3 / (U8 ? 16 : 4) : 1];   // <vec4>: the tiles in output order
    const int tid = threadIdx.x;
    const int bid = blockIdx.x;
    const int H = a.H, W = a.W, HW = H * W;
    const int f16 = a.f16, nhwc = a.nhwc;

    if (SET == 2 && bid >= a.B * a.tiles) {   // uniform: the flow picture, at the flow's own size
        const int rel = bid - a.B * a.tiles;
        const int n = rel / a.ftiles, tile = rel - n * a.ftiles;
        const int hw = a.h * a.w, base = tile * kRevTile, pix = base + tid;
        const float denom = vis_fold_max(ws, 0, n, a.mtiles, red[0]) + 1e-6f;
        float v[1][3] = {{0.0f, 0.0f, 0.0f}};
        if (pix < hw) vis_colour(vis_load(a.flow[0], nhwc, 0, 0, n, pix, hw), denom, v[0]);
        rev_emit<OUT_LAYOUT, U8, VEC, 1>(v, a.out + 6, n, base, hw, a.w, a.grid, stage4);
        return;
    }

    const int n = bid / a.tiles, tile = bid - n * a.tiles;
    const int base = tile * kRevTile, pix = base + tid;
    const int Y = pix / W, X = pix - Y * W;
    const bool live = pix < HW;
    const int ps6 = nhwc ? 6 : 1, ps3 = nhwc ? 3 : 1;   // pixel strides of 6- and 3-channel images
    const int64_t cs = nhwc ? 1 : HW;                   // channel stride
    float v[NP][3] = {};

    if (SET == 1) {
        const float denom0 = vis_fold_max(ws, 0, n, a.mtiles, red[0]) + 1e-6f;
        const float denom1 = vis_fold_max(ws, a.B * a.mtiles, n, a.mtiles, red[1]) + 1e-6f;
        if (live) {
            const void* ims = a.img[0];
            const int64_t ib = (int64_t)n * 6 * HW, at = ib + (int64_t)pix * ps6;
            const float2 flo = vis_load(a.flow[0], nhwc, 0, 0, n, pix, HW);
            const float2 flo_pred = vis_load(a.flow[1], nhwc, 0, 0, n, pix, HW);
            float w_pred[3], w_gt[3];
            rev_warp3(ims, f16, ib + 3 * cs, ps6, cs, Y, X, flo_pred, H, W, w_pred);
            rev_warp3(ims, f16, ib + 3 * cs, ps6, cs, Y, X, flo, H, W, w_gt);
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const float prv = 0.5f + rev_ld(ims, f16, at + c * cs), nxt = 0.5f + rev_ld(ims, f16, at + (3 + c) * cs);
                const float nxt_w = 0.5f + w_pred[c], nxt_w_gt = 0.5f + w_gt[c];
                v[0][c] = prv;
                v[1][c] = nxt;
                v[2][c] = nxt_w;
                v[3][c] = 0.5f * prv + 0.5f * nxt;
                v[4][c] = 0.5f * prv + 0.5f * nxt_w;
                v[5][c] = 0.5f * prv + 0.5f * nxt_w_gt;
                v[6][c] = fabsf(0.5f * prv - 0.5f * nxt_w);
                v[7][c] = fabsf(0.5f * prv - 0.5f * nxt_w_gt);
            }
            vis_colour(flo, denom0, v[8]);
            vis_colour(flo_pred, denom1, v[9]);
        }
    } else if (live) {
        const void *pair = a.img[0], *img1 = a.img[1], *pred = a.img[2];
        const int64_t ib6 = (int64_t)n * 6 * HW, ib3 = (int64_t)n * 3 * HW;
        const int64_t at6 = ib6 + (int64_t)pix * ps6, at3 = ib3 + (int64_t)pix * ps3;
        const int s = a.s;
        const float2 f = vis_load(a.flow[0], nhwc, 0, 0, n, (Y / s) * a.w + X / s, a.h * a.w);
        const float2 up = make_float2((float)s * f.x, (float)s * f.y);
        rev_warp3(img1, f16, ib3, ps3, cs, Y, X, up, H, W, v[5]);
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const float prv = 0.5f + rev_ld(pair, f16, at6 + c * cs), nxt = 0.5f + rev_ld(pair, f16, at6 + (3 + c) * cs);
            v[0][c] = prv;
            v[1][c] = nxt;
            v[2][c] = rev_ld(img1, f16, at3 + c * cs);
            v[3][c] = 0.5f + rev_ld(pred, f16, at3 + c * cs);
            v[4][c] = 0.5f * prv + 0.5f * nxt;
        }
    }
    rev_emit<OUT_LAYOUT, U8, VEC, NP>(v, a.out, n, base, HW, W, a.grid, stage4);
}

// ---- host side ------------------------------------------------------------------------------------------------------

// every count the launches index with fits 32 bits: 6 * B * H * W (the largest tensor) and the workgroups of both launches
bool review_shape_ok(int n_flows, int B, int H, int W, int h, int w) {
    if (6 * (int64_t)B * H * W > INT32_MAX || 2 * (int64_t)B * h * w > INT32_MAX) return false;
    const int64_t HW = (int64_t)H * W, hw = (int64_t)h * w;
    const int64_t pblk = B * (ceil_div(HW, kRevTile) + (n_flows == 1 ? ceil_div(hw, kRevTile) : 0));
    return review_workspace_floats(n_flows, B, h, w) <= INT32_MAX && pblk <= INT32_MAX;
}

// one partial per workgroup of the max launch
int64_t review_workspace_floats(int n_flows, int B, int h, int w) {
    return (int64_t)n_flows * B * ceil_div((int64_t)h * w, kVisMaxTile);
}

bool review_panels_vec(int n_flows, int H, int W, int h, int w) {
    return ((int64_t)H * W) % 4 == 0 && (n_flows == 2 || ((int64_t)h * w) % 4 == 0);
}

const char* review_panels_fwd_kernel(int n_flows, int H, int W, int h, int w) {
    return review_panels_vec(n_flows, H, W, h, w) ? "review_panels_kernel<vec4>" : "review_panels_kernel<scalar>";
}

template <int SET>
static int review_launch(RevArgs a, bool u8, int out_layout, float* ws, hipStream_t s) {
    const int n_flows = SET == 1 ? 2 : 1;
    a.mtiles = (int)ceil_div((int64_t)a.h * a.w, kVisMaxTile);
    a.tiles = (int)ceil_div((int64_t)a.H * a.W, kRevTile);
    a.ftiles = SET == 2 ? (int)ceil_div((int64_t)a.h * a.w, kRevTile) : 0;
    // the max launch: the fp32 flows as levels of one size, each read element by element
    VisMaxLevels m = {};
    for (int k = 0; k < kVisMaxLevels; ++k) {
        m.mblk0[k] = INT_MAX;
        if (k >= n_flows) continue;
        m.flow[k] = a.flow[k];
        m.hw[k] = a.h * a.w;
        m.mtiles[k] = a.mtiles;
        m.mblk0[k] = k * a.B * a.mtiles;
    }
    const int rc = flow_mag_max_launch(m, n_flows * a.B * a.mtiles, a.nhwc ? QPWC_NHWC : QPWC_NCHW, ws, s);
    if (rc != QPWC_OK) return rc;

    const bool vec = review_panels_vec(n_flows, a.H, a.W, a.h, a.w);
    dispatch_layout(out_layout, [&](auto O) {
        dispatch_bool(u8, [&](auto U) {
            dispatch_bool(vec, [&](auto V) {
                hipLaunchKernelGGL((review_panels_kernel<SET, decltype(O)::value, decltype(U)::value, decltype(V)::value>),
                                   dim3((unsigned)(a.B * (a.tiles + a.ftiles))), dim3(kVisThreads), 0, s, a,
                                   (const float*)ws);
            });
        });
    });
    return check_launch("review_panels_kernel");
}

int inference_panels_launch(const void* ims, bool f16, const float* flo, const float* flo_pred, int B, int H, int W,
                            int in_layout, void* const* outs, bool u8, int out_layout, int grid, float* ws,
                            hipStream_t s) {
    RevArgs a = {};
    a.img[0] = ims;
    a.flow[0] = flo;
    a.flow[1] = flo_pred;
    for (int p = 0; p < 10; ++p) a.out[p] = outs[p];
    a.B = B, a.H = a.h = H, a.W = a.w = W, a.s = 1;
    a.f16 = f16, a.nhwc = in_layout == QPWC_NHWC, a.grid = grid;
    return review_launch<1>(a, u8, out_layout, ws, s);
}

int interpolation_panels_launch(const void* img_pair, const void* img1, const void* pred, bool f16, const float* flow,
                                int B, int H, int W, int h, int w, int in_layout, void* const* outs, bool u8,
                                int out_layout, int grid, float* ws, hipStream_t s) {
    RevArgs a = {};
    a.img[0] = img_pair, a.img[1] = img1, a.img[2] = pred;
    a.flow[0] = flow;
    for (int p = 0; p < 5; ++p) a.out[p] = outs[p];
    a.out[5] = outs[6];   // 6-warp: with the H x W pictures
    a.out[6] = outs[5];   // 5-flow: the tail's
    a.B = B, a.H = H, a.W = W, a.h = h, a.w = w, a.s = H / h;
    a.f16 = f16, a.nhwc = in_layout == QPWC_NHWC, a.grid = grid;
    return review_launch<2>(a, u8, out_layout, ws, s);
}

}  // namespace qpwc

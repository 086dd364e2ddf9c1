// extern "C" boundary of libqpwc_hip.so (declared in include/qpwc.h).
// Validates arguments, then enqueues on the caller's stream.  No allocation,
// no synchronisation, no global state besides a thread-local error string.
#include <float.h>
#include <stdarg.h>
#include <stdio.h>

#include <initializer_list>

#include "../../include/qpwc_flow_quality.h"
#include "../../include/qpwc_image_loss.h"
#include "../../include/qpwc_masked_loss.h"
#include "../../include/qpwc_optim.h"
#include "../../include/qpwc_quality.h"
#include "../../include/qpwc_review.h"
#include "../../include/qpwc_sparse_augment.h"
#include "../../include/qpwc_triplet.h"
#include "../../include/qpwc_unsup_loss.h"
#include "../../include/qpwc_vis.h"
#include "launch.h"

namespace qpwc {

static thread_local char g_err[512] = "";
thread_local const char* g_dry_kernel = nullptr;
thread_local bool g_dry_run = false;

void set_error(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}

int check_launch(const char* what) {
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) {
        set_error("%s: %s", what, hipGetErrorString(e));
        return QPWC_E_LAUNCH;
    }
    return QPWC_OK;
}

// 16-byte-per-lane streaming copy: the box's achievable HBM ceiling (read + write) for bench.py's roofline
// block.  tools/micro/copybench.hip on MI355X: one float4 per thread over a one-shot grid with non-temporal
// loads and stores 6.5 TB/s (plain 6.1; 4 float4 per thread over a grid-strided loop 5.5-6.2; hipMemcpyAsync 5.3).
typedef unsigned int copy_u32x4 __attribute__((ext_vector_type(4)));
__global__ __launch_bounds__(256) void device_copy_kernel(const copy_u32x4* __restrict__ src,
                                                         copy_u32x4* __restrict__ dst, int64_t n16) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n16) __builtin_nontemporal_store(__builtin_nontemporal_load(src + i), dst + i);
}

static int fail(int code, const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
    return code;
}

static size_t esize(int dtype) { return dtype == QPWC_F16 ? 2 : 4; }

static bool overlaps(const void* a, size_t na, const void* b, size_t nb) {
    const uintptr_t a0 = (uintptr_t)a, b0 = (uintptr_t)b;
    return a0 < b0 + nb && b0 < a0 + na;
}

static int check_common(int B, int H, int W, int C, int layout, int dtype) {
    if (layout != QPWC_NHWC && layout != QPWC_NCHW)
        return fail(QPWC_E_LAYOUT, "Unsupported data format : %d", layout);
    if (dtype != QPWC_F32 && dtype != QPWC_F16) return fail(QPWC_E_DTYPE, "unsupported dtype %d", dtype);
    if (B <= 0 || H <= 0 || W <= 0 || C <= 0)
        return fail(QPWC_E_SHAPE, "non-positive extent B=%d H=%d W=%d C=%d", B, H, W, C);
    return QPWC_OK;
}

static int cost_volume_checked(const void* prv, const void* nxt, const void* flo, void* out, int B,
                               int H, int W, int C, int r, int layout, int dtype, float slope,
                               int64_t ops, int64_t off, bool strided, bool fuse, void* stream) {
    if (!prv || !nxt || !out || (fuse && !flo)) return fail(QPWC_E_NULL, "null pointer argument");
    int rc = check_common(B, H, W, C, layout, dtype);
    if (rc != QPWC_OK) return rc;
    if (r < 0 || r > 16) return fail(QPWC_E_RANGE, "search_range %d outside [0,16]", r);
    if (fuse && (H < 2 || W < 2))
        return fail(QPWC_E_SHAPE, "warp needs H,W >= 2 (got %dx%d)", H, W);
    const int64_t DD = (int64_t)(2 * r + 1) * (2 * r + 1);
    if (!strided) {
        ops = DD;
        off = 0;
    } else if (off < 0 || ops < off + DD) {
        return fail(QPWC_E_STRIDE, "out_pixel_stride %lld cannot hold %lld channels at offset %lld",
                    (long long)ops, (long long)DD, (long long)off);
    }
    const size_t es = esize(dtype);
    if ((uintptr_t)prv % es || (uintptr_t)nxt % es || (uintptr_t)out % es ||
        (fuse && (uintptr_t)flo % 4))
        return fail(QPWC_E_ALIGN, "pointer not aligned to its element size");
    const size_t n_in = (size_t)B * H * W * C * es;
    const size_t n_out = ((size_t)B * H * W * ops) * es;
    if (overlaps(out, n_out, prv, n_in) || overlaps(out, n_out, nxt, n_in) ||
        (fuse && overlaps(out, n_out, flo, (size_t)B * H * W * 2 * 4)))
        return fail(QPWC_E_ALIAS, "out overlaps an input");
    // every fused kernel reads prv and nxt as 16-byte vectors and there is no element-wise form behind them
    // (cost_volume_impl); a shape they do not take (C % 4, search_range) stays the launcher's to answer
    if (fuse && r == 4 && C % 4 == 0) {
        if ((uintptr_t)prv % 16) return fail(QPWC_E_ALIGN, "prv must be 16-byte aligned for the fused warp+cost volume");
        if ((uintptr_t)nxt % 16) return fail(QPWC_E_ALIGN, "nxt must be 16-byte aligned for the fused warp+cost volume");
    }
    char* o = (char*)out + (size_t)off * es;
    // 84-float pixels holding the 81 channels at offset 0: the 3 pad channels are written as zeros
    const bool pad84 = strided && r == 4 && ops == 84 && off == 0;
    return cost_volume_launch(prv, nxt, flo, o, B, H, W, C, r, layout, dtype, ops, slope, fuse, pad84,
                              (hipStream_t)stream);
}

// the shape rules of the training losses, shared by qpwc_loss_workspace_floats / _fwd / _fwd_kernel
static int loss_check_shapes(int kind, int B, int H, int W, int C, const int* h, const int* w, int n_levels) {
    if (kind < QPWC_LOSS_FLOW_MSE_V2 || kind > QPWC_LOSS_AUTORESIZE_MSE) return fail(QPWC_E_MODE, "unknown loss kind %d", kind);
    if (!h || !w) return fail(QPWC_E_NULL, "null pointer argument");
    if (n_levels < 1 || n_levels > 8) return fail(QPWC_E_SHAPE, "n_levels %d outside [1,8]", n_levels);
    if (B <= 0 || H <= 0 || W <= 0 || C <= 0)
        return fail(QPWC_E_SHAPE, "non-positive extent B=%d H=%d W=%d C=%d", B, H, W, C);
    if (kind != QPWC_LOSS_AUTORESIZE_MSE && C != 2) return fail(QPWC_E_SHAPE, "flow losses take 2 channels, got %d", C);
    // loss_pixel_kernel decodes a pixel inside its image in 32 bits
    if ((int64_t)H * W > INT32_MAX)
        return fail(QPWC_E_SHAPE, "H=%d W=%d: more than 2^31 - 1 pixels per image", H, W);
    // loss_area_tile_kernel, which only FlowMseLossV2 can take, counts the ground truth's 32 x 32 tiles in 32 bits
    if (kind == QPWC_LOSS_FLOW_MSE_V2 && (int64_t)B * (((int64_t)H + 31) / 32) * (((int64_t)W + 31) / 32) > INT32_MAX)
        return fail(QPWC_E_SHAPE, "B=%d H=%d W=%d: more than 2^31 - 1 tiles of 32 x 32 pixels", B, H, W);
    for (int i = 0; i < n_levels; ++i) {
        if (h[i] <= 0 || w[i] <= 0) return fail(QPWC_E_SHAPE, "level %d: non-positive extent %dx%d", i, h[i], w[i]);
        if ((int64_t)h[i] * w[i] > INT32_MAX)
            return fail(QPWC_E_SHAPE, "level %d: %dx%d is more than 2^31 - 1 pixels per image", i, h[i], w[i]);
        // einops.reduce('(h sh) (w sw)') in the reference fails the same way
        if (kind == QPWC_LOSS_FLOW_MSE_V2 && (H % h[i] || W % w[i]))
            return fail(QPWC_E_SHAPE, "level %d: %dx%d is not a whole-block area reduction of %dx%d", i, h[i], w[i], H, W);
    }
    return QPWC_OK;
}

// the shape rules of the masked flow losses, shared by qpwc_masked_loss_workspace_floats / _fwd / _fwd_kernel: those of
// the dense losses for the three flow kinds
static int masked_loss_check_shapes(int kind, int B, int H, int W, int C, const int* h, const int* w, int n_levels) {
    if (kind < QPWC_LOSS_FLOW_MSE_V2 || kind > QPWC_LOSS_FLOW_FINETUNE)
        return fail(QPWC_E_MODE, "loss kind %d is not one of the three flow losses", kind);
    return loss_check_shapes(kind, B, H, W, C, h, w, n_levels);
}

// the kind and shape rules of the label-free losses, shared by qpwc_unsup_loss_workspace_floats / _fwd / _fwd_kernel /
// _bwd: the kernels index a level's pixels and all levels' tiles in 32 bits
static int unsup_loss_check_shapes(int kind, int B, const int* h, const int* w, int n_levels) {
    if (kind != QPWC_UNSUP_CENSUS && kind != QPWC_UNSUP_CHARBONNIER)
        return fail(QPWC_E_MODE, "unknown photometric kind %d", kind);
    if (n_levels < 1 || n_levels > 8) return fail(QPWC_E_SHAPE, "n_levels %d outside [1,8]", n_levels);
    if (B <= 0) return fail(QPWC_E_SHAPE, "non-positive extent B=%d", B);
    for (int i = 0; i < n_levels; ++i) {
        if (h[i] <= 0 || w[i] <= 0) return fail(QPWC_E_SHAPE, "level %d: non-positive extent %dx%d", i, h[i], w[i]);
        if ((int64_t)B * h[i] * w[i] > INT32_MAX)
            return fail(QPWC_E_SHAPE, "level %d: B=%d %dx%d is more than 2^31 - 1 pixels", i, B, h[i], w[i]);
    }
    if (unsup_loss_total_tiles(B, h, w, n_levels) > INT32_MAX)
        return fail(QPWC_E_SHAPE, "B=%d: more than 2^31 - 1 tiles in all levels", B);
    return QPWC_OK;
}

// the parameter ranges the label-free losses share (a NaN fails both comparisons)
static int unsup_loss_check_range(std::initializer_list<float> positive, std::initializer_list<float> non_negative) {
    for (float v : positive)
        if (!(v > 0.0f)) return fail(QPWC_E_RANGE, "q, eps and smooth_eps must be > 0, got %g", (double)v);
    for (float v : non_negative)
        if (!(v >= 0.0f)) return fail(QPWC_E_RANGE, "edge and smooth_weight must be >= 0, got %g", (double)v);
    return QPWC_OK;
}

// the shape rules of the image loss, shared by qpwc_image_loss_workspace_floats / _fwd / _fwd_kernel / _bwd: the kernels
// index a level's elements and all levels' tiles in 32 bits
static int image_loss_check_shapes(int B, int C, const int* h, const int* w, int n_levels) {
    if (n_levels < 1 || n_levels > 8) return fail(QPWC_E_SHAPE, "n_levels %d outside [1,8]", n_levels);
    if (C < 1 || C > 4) return fail(QPWC_E_SHAPE, "images take 1..4 channels, got %d", C);
    if (B <= 0) return fail(QPWC_E_SHAPE, "non-positive extent B=%d", B);
    for (int i = 0; i < n_levels; ++i) {
        if (h[i] <= 0 || w[i] <= 0) return fail(QPWC_E_SHAPE, "level %d: non-positive extent %dx%d", i, h[i], w[i]);
        // factor by factor, so that no product leaves 64 bits: B * C < 2^33 and h * w < 2^62 here
        if ((int64_t)h[i] * w[i] > INT32_MAX || (int64_t)B * C * ((int64_t)h[i] * w[i]) > INT32_MAX)
            return fail(QPWC_E_SHAPE, "level %d: B=%d C=%d %dx%d is more than 2^31 - 1 elements", i, B, C, h[i], w[i]);
    }
    // every extent is now at most 2^31 - 1 and B * h * w at most 2^31 - 1 per level: the tile counts below fit 64 bits
    if (image_loss_total_tiles(B, h, w, n_levels) > INT32_MAX)
        return fail(QPWC_E_SHAPE, "B=%d: more than 2^31 - 1 tiles in all levels", B);
    return QPWC_OK;
}

// the parameter ranges of the image loss (a NaN fails every comparison); max_val: NULL in the backward, which has none
static int image_loss_check_range(float ssim_weight, float q, float eps, const float* max_val, float offset) {
    if (!(ssim_weight >= 0.0f && ssim_weight <= 1.0f))
        return fail(QPWC_E_RANGE, "ssim_weight %g outside [0,1]", (double)ssim_weight);
    if (!(q > 0.0f) || !(eps > 0.0f)) return fail(QPWC_E_RANGE, "q and eps must be > 0, got %g and %g", (double)q, (double)eps);
    if (max_val && !(*max_val > 0.0f && *max_val <= FLT_MAX))
        return fail(QPWC_E_RANGE, "max_val must be finite and > 0, got %g", (double)*max_val);
    if (!(offset >= -FLT_MAX && offset <= FLT_MAX)) return fail(QPWC_E_RANGE, "offset must be finite, got %g", (double)offset);
    return QPWC_OK;
}

// the shape rules of the input pipeline, shared by qpwc_augment_workspace_floats / _fwd / _fwd_kernel
static int augment_check_shapes(int B, int H, int W, int h, int w) {
    if (B <= 0 || H <= 0 || W <= 0 || h <= 0 || w <= 0)
        return fail(QPWC_E_SHAPE, "non-positive extent B=%d H=%d W=%d h=%d w=%d", B, H, W, h, w);
    if (!augment_shape_ok(B, H, W, h, w))
        return fail(QPWC_E_SHAPE, "B=%d %dx%d -> %dx%d: a pixel count or the launch grid overflows 32 bits", B, H, W, h, w);
    return QPWC_OK;
}

// the shape rules of the interpolator's input pipeline, shared by qpwc_augment_triplet_fwd / _fwd_kernel: its launch is
// augment_pixel_kernel's (one-dimensional over sample x 256-pixel chunk, 6 floats per pixel in the larger output)
static int triplet_check_shapes(int B, int H, int W, int h, int w) { return augment_check_shapes(B, H, W, h, w); }

// the shape rules of the flow panels, shared by qpwc_flow_to_image_workspace_floats / _fwd / _fwd_kernel; oh, ow may be
// NULL (the workspace depends on the flows' own sizes only)
static int vis_check_shapes(int n, int B, const int* h, const int* w, const int* oh, const int* ow) {
    if (n < 1 || n > 8) return fail(QPWC_E_SHAPE, "n %d outside [1,8]", n);
    if (B <= 0) return fail(QPWC_E_SHAPE, "non-positive extent B=%d", B);
    for (int l = 0; l < n; ++l) {
        if (h[l] <= 0 || w[l] <= 0) return fail(QPWC_E_SHAPE, "level %d: non-positive extent %dx%d", l, h[l], w[l]);
        if (oh && (oh[l] <= 0 || ow[l] <= 0))
            return fail(QPWC_E_SHAPE, "level %d: non-positive output extent %dx%d", l, oh[l], ow[l]);
    }
    if (!flow_to_image_shape_ok(n, B, h, w, oh, ow))
        return fail(QPWC_E_SHAPE, "B=%d: an element count or a launch grid overflows 32 bits", B);
    return QPWC_OK;
}

// the shape rules of the image quality, shared by qpwc_image_quality_workspace_floats / _fwd / _fwd_kernel
static int quality_check_shapes(int B, int H, int W, int C) {
    if (B < 1) return fail(QPWC_E_SHAPE, "non-positive extent B=%d", B);
    if (C < 1 || C > 4) return fail(QPWC_E_SHAPE, "C=%d outside 1..4", C);
    // tf.image.ssim refuses it the same way: the 11 x 11 window has no position
    if (H < 11 || W < 11) return fail(QPWC_E_SHAPE, "H=%d W=%d: both must be at least 11, the filter size", H, W);
    if (!image_quality_shape_ok(B, H, W, C))
        return fail(QPWC_E_SHAPE, "B=%d H=%d W=%d C=%d: the element count or a launch grid overflows 32 bits", B, H, W, C);
    return QPWC_OK;
}

// the shape rules of the flow metrics, shared by qpwc_flow_quality_workspace_floats / _fwd / _fwd_kernel
static int flow_quality_check_shapes(int B, int H, int W) {
    if (B < 1 || H < 1 || W < 1) return fail(QPWC_E_SHAPE, "non-positive extent B=%d H=%d W=%d", B, H, W);
    if (!flow_quality_shape_ok(B, H, W))
        return fail(QPWC_E_SHAPE, "B=%d H=%d W=%d: the pixel count or a launch grid overflows 32 bits", B, H, W);
    return QPWC_OK;
}

// the shape rules of the review panels, shared by qpwc_review_workspace_floats / qpwc_review_panels_fwd_kernel and both
// entry points; n_flows = 2: the pictures of test_infer.py (h x w is H x W), 1: those of pre_train_test.py
static int review_check_shapes(int n_flows, int B, int H, int W, int h, int w) {
    if (n_flows != 1 && n_flows != 2) return fail(QPWC_E_SHAPE, "n_flows %d outside [1,2]", n_flows);
    if (B <= 0 || H <= 0 || W <= 0 || h <= 0 || w <= 0)
        return fail(QPWC_E_SHAPE, "non-positive extent B=%d H=%d W=%d h=%d w=%d", B, H, W, h, w);
    const int s = H / h;
    if (s < 1 || H != s * h || (int64_t)W != (int64_t)s * w || (n_flows == 2 && s != 1))
        return fail(QPWC_E_SHAPE, "%dx%d is not one whole multiple of the flow's %dx%d", H, W, h, w);
    if (!review_shape_ok(n_flows, B, H, W, h, w))
        return fail(QPWC_E_SHAPE, "B=%d H=%d W=%d: an element count or a launch grid overflows 32 bits", B, H, W);
    return QPWC_OK;
}

// the first null pointer of a {pointer, name} list fails, by name
struct PtrName {
    const void* p;
    const char* name;
};
static int check_nonnull(std::initializer_list<PtrName> need) {
    for (const PtrName& a : need)
        if (!a.p) return fail(QPWC_E_NULL, "%s is null", a.name);
    return QPWC_OK;
}

// name, extent in bytes and required alignment of every buffer of an entry point: inputs first, then outputs
struct BufCheck {
    const void* p;
    size_t n, align;
    char name[16];
};
// a buffer whose name carries an index: src[1], grad_src[2]
static BufCheck indexed_buf(const void* p, size_t n, size_t align, const char* fmt, int i) {
    BufCheck b = {p, n, align, ""};
    snprintf(b.name, sizeof(b.name), fmt, i);
    return b;
}
// every buffer aligned; no output (index >= n_in) overlapping a buffer listed before it
static int check_bufs(const BufCheck* b, int n_in, int n_all) {
    for (int k = 0; k < n_all; ++k)
        if ((uintptr_t)b[k].p % b[k].align) return fail(QPWC_E_ALIGN, "%s must be %d-byte aligned", b[k].name, (int)b[k].align);
    for (int o = n_in; o < n_all; ++o)
        for (int k = 0; k < o; ++k)
            if (overlaps(b[o].p, b[o].n, b[k].p, b[k].n)) return fail(QPWC_E_ALIAS, "%s overlaps %s", b[o].name, b[k].name);
    return QPWC_OK;
}

// Every check of the review panels' two entry points after the null pointers, in the order include/qpwc_review.h
// states; imgs: the n_img images with their channel counts, flows: the n_flows flows of h x w, outs: n_out pictures of
// H x W but for outs[flow_pic] (-1: none), which has the flow's size.  The store form follows from the shape and decides
// the alignment the outputs must have: the kernel does not look at the pointers.
static int review_check(const void* const* imgs, const int* img_c, int n_img, int img_dtype, const void* const* flows,
                        int n_flows, int B, int H, int W, int h, int w, int in_layout, void* const* outs, int n_out,
                        int flow_pic, int out_dtype, int out_layout, int grid, const void* ws) {
    if (img_dtype != QPWC_F32 && img_dtype != QPWC_F16) return fail(QPWC_E_DTYPE, "images: unsupported dtype %d", img_dtype);
    if (out_dtype != QPWC_F32 && out_dtype != QPWC_U8) return fail(QPWC_E_DTYPE, "unsupported output dtype %d", out_dtype);
    if (in_layout != QPWC_NHWC && in_layout != QPWC_NCHW)
        return fail(QPWC_E_LAYOUT, "Unsupported data format : %d", in_layout);
    if (out_layout != QPWC_NHWC && out_layout != QPWC_NCHW)
        return fail(QPWC_E_LAYOUT, "Unsupported data format : %d", out_layout);
    int rc = review_check_shapes(n_flows, B, H, W, h, w);
    if (rc != QPWC_OK) return rc;
    if (grid < 0) return fail(QPWC_E_SHAPE, "grid %d is negative", grid);
    const bool u8 = out_dtype == QPWC_U8;
    const size_t oalign = review_panels_vec(n_flows, H, W, h, w) ? (u8 ? 4 : 16) : (u8 ? 1 : 4);
    BufCheck bufs[3 + 2 + 1 + 10];
    int k = 0;
    static const char* const img_names[2][3] = {{"img_pair", "img1", "pred"}, {"ims", "", ""}};
    static const char* const flow_names[2][2] = {{"flow", ""}, {"flo", "flo_pred"}};
    for (int i = 0; i < n_img; ++i)
        bufs[k++] = indexed_buf(imgs[i], (size_t)B * H * W * img_c[i] * esize(img_dtype), esize(img_dtype),
                                img_names[n_flows - 1][i], 0);
    for (int i = 0; i < n_flows; ++i)
        bufs[k++] = indexed_buf(flows[i], (size_t)B * h * w * 2 * 4, 4, flow_names[n_flows - 1][i], 0);
    const int n_in = k;
    bufs[k++] = indexed_buf(ws, (size_t)review_workspace_floats(n_flows, B, h, w) * 4, 4, "ws", 0);
    for (int i = 0; i < n_out; ++i) {
        const size_t px = i == flow_pic ? (size_t)h * w : (size_t)H * W;
        bufs[k++] = indexed_buf(outs[i], (size_t)B * px * 3 * (u8 ? 1 : 4), oalign, "outs[%d]", i);
    }
    return check_bufs(bufs, n_in, k);
}

static int flow_head_train_check_shape(int B, int H, int W) {
    if (B <= 0 || H <= 0 || W <= 0) return fail(QPWC_E_SHAPE, "non-positive extent B=%d H=%d W=%d", B, H, W);
    if ((int64_t)B * H * W > (1 << 24))
        return fail(QPWC_E_SHAPE, "B=%d H=%d W=%d: more than 2^24 pixels (the pixel counts are fp32)", B, H, W);
    return QPWC_OK;
}

static int image_head_check_m(int64_t M) {
    if (M <= 0 || M > ((int64_t)1 << 40)) return fail(QPWC_E_SHAPE, "M=%lld outside [1, 2^40] pixels", (long long)M);
    return QPWC_OK;
}

// the shape rules both directions of the image upsampling share
static int upsample2x_image_check_shape(int B, int h, int w, int C) {
    if (B <= 0 || h <= 0 || w <= 0) return fail(QPWC_E_SHAPE, "non-positive extent B=%d h=%d w=%d", B, h, w);
    if (C < 1 || C > 4) return fail(QPWC_E_SHAPE, "C=%d outside 1..4", C);
    if (h > (1 << 29) || w > (1 << 29)) return fail(QPWC_E_SHAPE, "h=%d w=%d: the doubled extents must fit an int", h, w);
    return QPWC_OK;
}

}  // namespace qpwc

using namespace qpwc;

extern "C" {

int qpwc_version(void) { return QPWC_VERSION; }

int qpwc_layout_transpose_fwd(const void* in, void* out, int B, int H, int W, int C, int to_layout, int dtype,
                              void* stream) {
    if (!in || !out) return fail(QPWC_E_NULL, "null pointer argument");
    const int rc = check_common(B, H, W, C, to_layout, dtype);
    if (rc) return rc;
    const size_t es = esize(dtype), n = (size_t)B * H * W * C * es;
    if ((uintptr_t)in % es || (uintptr_t)out % es) return fail(QPWC_E_ALIGN, "pointer not aligned to its element size");
    if (overlaps(out, n, in, n)) return fail(QPWC_E_ALIAS, "out overlaps in");
    return layout_transpose_launch(in, out, B, H, W, C, to_layout, dtype, (hipStream_t)stream);
}

int qpwc_copy_pixels_fwd(const void* src, void* dst, int B, int H, int W, int C, const int64_t* src_strides,
                         const int64_t* dst_strides, int dtype, void* stream) {
    if (!src || !dst || !src_strides || !dst_strides) return fail(QPWC_E_NULL, "null pointer argument");
    if (dtype != QPWC_F32 && dtype != QPWC_F16) return fail(QPWC_E_DTYPE, "unsupported dtype %d", dtype);
    if (B <= 0 || H <= 0 || W <= 0 || C <= 0) return fail(QPWC_E_SHAPE, "non-positive extent B=%d H=%d W=%d C=%d", B, H, W, C);
    const int64_t es = dtype == QPWC_F32 ? 4 : 2;
    if ((C * es) % 16) return fail(QPWC_E_SHAPE, "a pixel's %d channels must be whole 16-byte chunks", C);
    for (int i = 0; i < 3; ++i) {
        if (src_strides[i] < (i == 2 ? C : 0) || dst_strides[i] < (i == 2 ? C : 0))
            return fail(QPWC_E_STRIDE, "stride %d smaller than what it spans", i);
        if ((src_strides[i] * es) % 16 || (dst_strides[i] * es) % 16)
            return fail(QPWC_E_STRIDE, "strides must be multiples of 16 bytes");
    }
    if (((uintptr_t)src | (uintptr_t)dst) % 16) return fail(QPWC_E_ALIGN, "pointers must be 16-byte aligned");
    const size_t sext = (size_t)(((B - 1) * src_strides[0] + (H - 1) * src_strides[1] + (W - 1) * src_strides[2] + C) * es);
    const size_t dext = (size_t)(((B - 1) * dst_strides[0] + (H - 1) * dst_strides[1] + (W - 1) * dst_strides[2] + C) * es);
    if (overlaps(dst, dext, src, sext)) return fail(QPWC_E_ALIAS, "dst overlaps src");
    return copy_pixels_launch(src, dst, B, H, W, C * es, src_strides[0] * es, src_strides[1] * es, src_strides[2] * es,
                              dst_strides[0] * es, dst_strides[1] * es, dst_strides[2] * es, (hipStream_t)stream);
}

// One wave that stamps (shader-clock counter, 100 MHz real-time counter) pairs while it sleeps: the sustained clock of
// the chip under whatever runs beside it is delta(s_memtime) / delta(s_memrealtime) x 100 MHz
// (MI355X_MICROARCH.md, constants table).  Bounded: n_samples stamps, then the wave ends.
__global__ __launch_bounds__(64) void clock_probe_kernel(unsigned long long* __restrict__ out, int n_samples,
                                                         int sleeps_per_sample) {
    if (threadIdx.x != 0) return;
    for (int i = 0; i < n_samples; ++i) {
        const unsigned long long t = __builtin_amdgcn_s_memtime();
        const unsigned long long r = __builtin_amdgcn_s_memrealtime();
        out[2 * i] = t;
        out[2 * i + 1] = r;
        for (int k = 0; k < sleeps_per_sample; ++k) __builtin_amdgcn_s_sleep(127);
    }
}

int qpwc_clock_probe(void* out_pairs, int n_samples, int sleeps_per_sample, void* stream) {
    if (!out_pairs) return fail(QPWC_E_NULL, "null pointer argument");
    if (n_samples <= 0 || n_samples > (1 << 20) || sleeps_per_sample < 0 || sleeps_per_sample > 4096)
        return fail(QPWC_E_SHAPE, "clock probe: 1..2^20 samples of 0..4096 sleeps");
    if ((uintptr_t)out_pairs % 8) return fail(QPWC_E_ALIGN, "clock probe buffer must be 8-byte aligned");
    hipLaunchKernelGGL(clock_probe_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, (unsigned long long*)out_pairs,
                       n_samples, sleeps_per_sample);
    return check_launch("clock_probe_kernel");
}

int qpwc_device_copy(const void* src, void* dst, int64_t bytes, void* stream) {
    if (!src || !dst) return fail(QPWC_E_NULL, "null pointer argument");
    if (bytes <= 0 || bytes % 16) return fail(QPWC_E_SHAPE, "bytes must be a positive multiple of 16");
    if (((uintptr_t)src | (uintptr_t)dst) % 16) return fail(QPWC_E_ALIGN, "pointers must be 16-byte aligned");
    if (overlaps(dst, (size_t)bytes, src, (size_t)bytes)) return fail(QPWC_E_ALIAS, "dst overlaps src");
    const int64_t n16 = bytes / 16;
    const int64_t want = (n16 + 255) / 256;
    if (want > INT32_MAX) return fail(QPWC_E_SHAPE, "copy of %lld bytes needs too many workgroups", (long long)bytes);
    const unsigned grid = (unsigned)want;
    hipLaunchKernelGGL(device_copy_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream,
                       (const copy_u32x4*)src, (copy_u32x4*)dst, n16);
    return check_launch("device_copy_kernel");
}

const char* qpwc_last_error(void) { return g_err; }

const char* qpwc_strerror(int code) {
    switch (code) {
        case QPWC_OK: return "ok";
        case QPWC_E_NULL: return "null pointer";
        case QPWC_E_LAYOUT: return "unsupported data format";
        case QPWC_E_DTYPE: return "unsupported dtype";
        case QPWC_E_SHAPE: return "bad shape";
        case QPWC_E_RANGE: return "bad search range";
        case QPWC_E_MODE: return "unknown warp mode";
        case QPWC_E_ALIAS: return "output aliases an input";
        case QPWC_E_LAUNCH: return "kernel launch failed";
        case QPWC_E_ALIGN: return "misaligned pointer";
        case QPWC_E_STRIDE: return "bad output stride/offset";
        case QPWC_E_NODEVICE: return "no HIP device";
        default: return "unknown error";
    }
}

int qpwc_cost_volume_fwd(const void* prv, const void* nxt, void* out, int B, int H, int W, int C,
                         int search_range, int layout, int dtype, float lrelu_slope, void* stream) {
    return cost_volume_checked(prv, nxt, nullptr, out, B, H, W, C, search_range, layout, dtype,
                               lrelu_slope, 0, 0, false, false, stream);
}

int qpwc_cost_volume_fwd_strided(const void* prv, const void* nxt, void* out, int B, int H, int W,
                                 int C, int search_range, int dtype, float lrelu_slope,
                                 int64_t out_pixel_stride, int64_t out_channel_offset, void* stream) {
    return cost_volume_checked(prv, nxt, nullptr, out, B, H, W, C, search_range, QPWC_NHWC, dtype,
                               lrelu_slope, out_pixel_stride, out_channel_offset, true, false,
                               stream);
}

int qpwc_warp_cost_volume_fwd(const void* prv, const void* nxt, const void* flo, void* out, int B,
                              int H, int W, int C, int search_range, int dtype, float lrelu_slope,
                              int64_t out_pixel_stride, int64_t out_channel_offset, void* stream) {
    return cost_volume_checked(prv, nxt, flo, out, B, H, W, C, search_range, QPWC_NHWC, dtype,
                               lrelu_slope, out_pixel_stride, out_channel_offset, true, true, stream);
}

const char* qpwc_cost_volume_kernel(int B, int H, int W, int C, int search_range, int layout, int dtype,
                                    int64_t out_pixel_stride, int fused) {
    if (check_common(B, H, W, C, layout, dtype) != QPWC_OK || search_range < 0 || search_range > 16 ||
        (fused && (H < 2 || W < 2 || layout != QPWC_NHWC)))
        return "";
    const int DD = (2 * search_range + 1) * (2 * search_range + 1);
    if (out_pixel_stride <= 0) out_pixel_stride = DD;
    // the launchers only look at the alignment of their operands: a 4096-aligned placeholder stands for
    // "aligned as torch allocates"; nothing is dereferenced or enqueued while g_dry_run is set
    const void* p = reinterpret_cast<const void*>((uintptr_t)4096);
    g_dry_kernel = "";
    g_dry_run = true;
    const bool pad84 = layout == QPWC_NHWC && out_pixel_stride == 84 && DD == 81;
    const int rc = cost_volume_launch(p, p, fused ? p : nullptr, const_cast<void*>(p), B, H, W, C, search_range, layout,
                                      dtype, out_pixel_stride, 0.1f, fused != 0, pad84, nullptr);
    g_dry_run = false;
    return rc == QPWC_OK ? g_dry_kernel : "";
}

int qpwc_warp_fwd(const void* img, const void* flo, void* out, int B, int H, int W, int C,
                  int flo_bcast_mask, int layout, int dtype, int mode, void* stream) {
    if (!img || !flo || !out) return fail(QPWC_E_NULL, "null pointer argument");
    int rc = check_common(B, H, W, C, layout, dtype);
    if (rc != QPWC_OK) return rc;
    if (mode != QPWC_WARP_CLAMP && mode != QPWC_WARP_TFWARP)
        return fail(QPWC_E_MODE, "unknown warp mode %d", mode);
    if (mode == QPWC_WARP_CLAMP && (H < 2 || W < 2))
        return fail(QPWC_E_SHAPE, "Grid must be at least 2x2 (got %dx%d)", H, W);
    if (flo_bcast_mask & ~(QPWC_BCAST_B | QPWC_BCAST_H | QPWC_BCAST_W))
        return fail(QPWC_E_SHAPE, "bad flo_bcast_mask %d", flo_bcast_mask);
    const size_t es = esize(dtype);
    if ((uintptr_t)img % es || (uintptr_t)out % es || (uintptr_t)flo % 4)
        return fail(QPWC_E_ALIGN, "pointer not aligned to its element size");
    const size_t n = (size_t)B * H * W * C * es;
    const size_t nf = (size_t)((flo_bcast_mask & QPWC_BCAST_B) ? 1 : B) *
                      ((flo_bcast_mask & QPWC_BCAST_H) ? 1 : H) *
                      ((flo_bcast_mask & QPWC_BCAST_W) ? 1 : W) * 2 * 4;
    if (overlaps(out, n, img, n) || overlaps(out, n, flo, nf))
        return fail(QPWC_E_ALIAS, "out overlaps an input");
    return warp_launch(img, flo, out, B, H, W, C, flo_bcast_mask, layout, dtype, mode,
                       (hipStream_t)stream);
}

int qpwc_cost_volume_bwd(const void* prv, const void* nxt, const void* out, const void* grad_out, void* grad_prv,
                         void* grad_nxt, int B, int H, int W, int C, int search_range, int dtype, float lrelu_slope,
                         void* stream) {
    if (!prv || !nxt || !out || !grad_out || (!grad_prv && !grad_nxt)) return fail(QPWC_E_NULL, "null pointer argument");
    int rc = check_common(B, H, W, C, QPWC_NHWC, dtype);
    if (rc != QPWC_OK) return rc;
    if (search_range < 0 || search_range > 16) return fail(QPWC_E_RANGE, "search_range %d outside [0,16]", search_range);
    // the mask is read from the saved output as out > 0: the sign of the pre-activation only for slope >= 0
    if (!(lrelu_slope >= 0.0f)) return fail(QPWC_E_RANGE, "lrelu_slope %g: the backward needs slope >= 0", (double)lrelu_slope);
    const size_t es = esize(dtype);
    if ((uintptr_t)prv % es || (uintptr_t)nxt % es || (uintptr_t)out % es || (uintptr_t)grad_out % es ||
        (uintptr_t)grad_prv % es || (uintptr_t)grad_nxt % es)
        return fail(QPWC_E_ALIGN, "pointer not aligned to its element size");
    const int64_t DD = (int64_t)(2 * search_range + 1) * (2 * search_range + 1);
    const size_t n_in = (size_t)B * H * W * C * es, n_cv = (size_t)B * H * W * DD * es;
    const void* ins[4] = {prv, nxt, out, grad_out};
    const size_t ns[4] = {n_in, n_in, n_cv, n_cv};
    for (void* g : {grad_prv, grad_nxt}) {
        if (!g) continue;
        for (int i = 0; i < 4; ++i)
            if (overlaps(g, n_in, ins[i], ns[i])) return fail(QPWC_E_ALIAS, "a gradient buffer overlaps an input");
    }
    if (grad_prv && grad_nxt && overlaps(grad_prv, n_in, grad_nxt, n_in))
        return fail(QPWC_E_ALIAS, "grad_prv overlaps grad_nxt");
    return cost_volume_bwd_launch(prv, nxt, out, grad_out, grad_prv, grad_nxt, B, H, W, C, search_range, dtype,
                                  lrelu_slope, (hipStream_t)stream);
}

int64_t qpwc_warp_bwd_workspace_floats(int B, int H, int W, int C, int dtype) {
    if (dtype != QPWC_F32 && dtype != QPWC_F16) return fail(QPWC_E_DTYPE, "unsupported dtype %d", dtype);
    if (B <= 0 || H <= 0 || W <= 0 || C <= 0)
        return fail(QPWC_E_SHAPE, "non-positive extent B=%d H=%d W=%d C=%d", B, H, W, C);
    return dtype == QPWC_F32 ? 0 : (int64_t)B * H * W * C;
}

int qpwc_warp_bwd(const void* img, const void* flo, const void* grad_out, void* grad_img, void* grad_flo,
                  void* workspace, int B, int H, int W, int C, int dtype, int mode, void* stream) {
    if (!img || !flo || !grad_out || (!grad_img && !grad_flo)) return fail(QPWC_E_NULL, "null pointer argument");
    int rc = check_common(B, H, W, C, QPWC_NHWC, dtype);
    if (rc != QPWC_OK) return rc;
    if (mode != QPWC_WARP_CLAMP && mode != QPWC_WARP_TFWARP) return fail(QPWC_E_MODE, "unknown warp mode %d", mode);
    if (mode == QPWC_WARP_CLAMP && (H < 2 || W < 2))
        return fail(QPWC_E_SHAPE, "Grid must be at least 2x2 (got %dx%d)", H, W);
    const bool need_ws = grad_img && dtype == QPWC_F16;
    if (need_ws && !workspace) return fail(QPWC_E_NULL, "fp16 grad_img needs the fp32 workspace");
    const size_t es = esize(dtype);
    if ((uintptr_t)img % es || (uintptr_t)grad_out % es || (uintptr_t)grad_img % es || (uintptr_t)flo % 4 ||
        (uintptr_t)grad_flo % 4 || (need_ws && (uintptr_t)workspace % 4))
        return fail(QPWC_E_ALIGN, "pointer not aligned to its element size");
    const size_t n = (size_t)B * H * W * C * es, nf = (size_t)B * H * W * 2 * 4, nw = (size_t)B * H * W * C * 4;
    const void* ins[3] = {img, flo, grad_out};
    const size_t ns[3] = {n, nf, n};
    void* outs[3] = {grad_img, grad_flo, need_ws ? workspace : nullptr};
    const size_t no[3] = {n, nf, nw};
    for (int o = 0; o < 3; ++o) {
        if (!outs[o]) continue;
        for (int i = 0; i < 3; ++i)
            if (overlaps(outs[o], no[o], ins[i], ns[i])) return fail(QPWC_E_ALIAS, "a gradient buffer overlaps an input");
        for (int k = o + 1; k < 3; ++k)
            if (outs[k] && overlaps(outs[o], no[o], outs[k], no[k]))
                return fail(QPWC_E_ALIAS, "gradient / workspace buffers overlap each other");
    }
    return warp_bwd_launch(img, flo, grad_out, grad_img, grad_flo, need_ws ? workspace : nullptr, B, H, W, C, dtype,
                           mode, (hipStream_t)stream);
}

int64_t qpwc_loss_workspace_floats(int kind, int B, int H, int W, int C, const int* h, const int* w, int n_levels) {
    const int rc = loss_check_shapes(kind, B, H, W, C, h, w, n_levels);
    return rc != QPWC_OK ? rc : loss_workspace_floats(n_levels);
}

const char* qpwc_loss_fwd_kernel(int kind, const void* y_true, int B, int H, int W, int C, const int* h, const int* w,
                                 int n_levels) {
    if (loss_check_shapes(kind, B, H, W, C, h, w, n_levels) != QPWC_OK) return "";
    return loss_fwd_kernel(kind, H, W, h, w, n_levels, y_true);
}

int qpwc_loss_fwd(int kind, float p0, float p1, const void* y_true, int B, int H, int W, int C, int layout,
                  const void* const* y_pred, const int* h, const int* w, const int* pred_dtype, int n_levels,
                  void* out_losses, void* const* dpred, void* const* gt_out, void* workspace, void* stream) {
    if (!y_true || !y_pred || !pred_dtype || !out_losses || !workspace) return fail(QPWC_E_NULL, "null pointer argument");
    int rc = loss_check_shapes(kind, B, H, W, C, h, w, n_levels);
    if (rc != QPWC_OK) return rc;
    if (layout != QPWC_NHWC && layout != QPWC_NCHW) return fail(QPWC_E_LAYOUT, "Unsupported data format : %d", layout);
    if (kind == QPWC_LOSS_FLOW_MSE_V2 && !(p0 >= 0.0f)) return fail(QPWC_E_RANGE, "Huber delta %g < 0", (double)p0);
    if ((uintptr_t)y_true % 4 || (uintptr_t)out_losses % 4 || (uintptr_t)workspace % 4)
        return fail(QPWC_E_ALIGN, "pointer not aligned to its element size");
    // every input and output extent, for the alias checks
    const void* ins[1 + 8];
    size_t nin[1 + 8];
    void* outs[2 + 16];
    size_t nout[2 + 16];
    int ni = 0, no = 0;
    ins[ni] = y_true;
    nin[ni++] = (size_t)B * H * W * C * 4;
    outs[no] = out_losses;
    nout[no++] = (size_t)n_levels * 4;
    outs[no] = workspace;
    nout[no++] = (size_t)loss_workspace_floats(n_levels) * 4;
    for (int i = 0; i < n_levels; ++i) {
        if (pred_dtype[i] != QPWC_F32 && pred_dtype[i] != QPWC_F16)
            return fail(QPWC_E_DTYPE, "level %d: unsupported prediction dtype %d", i, pred_dtype[i]);
        const bool want_gt = gt_out && gt_out[i];
        if (!y_pred[i] && !want_gt) return fail(QPWC_E_NULL, "null prediction at level %d", i);
        if (dpred && !dpred[i]) return fail(QPWC_E_NULL, "null dpred buffer at level %d", i);
        const size_t es = esize(pred_dtype[i]), ne = (size_t)B * h[i] * w[i] * C;
        if ((uintptr_t)y_pred[i] % es || (dpred && (uintptr_t)dpred[i] % 4) || (want_gt && (uintptr_t)gt_out[i] % 4))
            return fail(QPWC_E_ALIGN, "level %d: pointer not aligned to its element size", i);
        if (y_pred[i]) {
            ins[ni] = y_pred[i];
            nin[ni++] = ne * es;
        }
        if (dpred) {
            outs[no] = dpred[i];
            nout[no++] = ne * 4;
        }
        if (want_gt) {
            outs[no] = gt_out[i];
            nout[no++] = ne * 4;
        }
    }
    for (int o = 0; o < no; ++o) {
        for (int i = 0; i < ni; ++i)
            if (overlaps(outs[o], nout[o], ins[i], nin[i])) return fail(QPWC_E_ALIAS, "an output overlaps an input");
        for (int k = o + 1; k < no; ++k)
            if (overlaps(outs[o], nout[o], outs[k], nout[k])) return fail(QPWC_E_ALIAS, "two outputs overlap");
    }
    return loss_fwd_launch(kind, p0, p1, (const float*)y_true, B, H, W, C, layout, y_pred, h, w, pred_dtype, n_levels,
                           (float*)out_losses, dpred, gt_out, (float*)workspace, (hipStream_t)stream);
}

int qpwc_loss_bwd(const void* const* dpred, const void* grad_losses, void* const* grad_pred, const int64_t* n_elems,
                  const int* pred_dtype, int n_levels, void* stream) {
    if (!dpred || !grad_losses || !grad_pred || !n_elems || !pred_dtype) return fail(QPWC_E_NULL, "null pointer argument");
    if (n_levels < 1 || n_levels > 8) return fail(QPWC_E_SHAPE, "n_levels %d outside [1,8]", n_levels);
    if ((uintptr_t)grad_losses % 4) return fail(QPWC_E_ALIGN, "grad_losses not 4-byte aligned");
    for (int i = 0; i < n_levels; ++i) {
        if (!dpred[i] || !grad_pred[i]) return fail(QPWC_E_NULL, "null buffer at level %d", i);
        if (pred_dtype[i] != QPWC_F32 && pred_dtype[i] != QPWC_F16)
            return fail(QPWC_E_DTYPE, "level %d: unsupported prediction dtype %d", i, pred_dtype[i]);
        if (n_elems[i] <= 0) return fail(QPWC_E_SHAPE, "level %d has no elements", i);
        if ((uintptr_t)dpred[i] % 4 || (uintptr_t)grad_pred[i] % esize(pred_dtype[i]))
            return fail(QPWC_E_ALIGN, "level %d: pointer not aligned to its element size", i);
    }
    for (int i = 0; i < n_levels; ++i) {
        const size_t ng = (size_t)n_elems[i] * esize(pred_dtype[i]);
        if (overlaps(grad_pred[i], ng, grad_losses, (size_t)n_levels * 4))
            return fail(QPWC_E_ALIAS, "grad_pred overlaps grad_losses");
        for (int k = 0; k < n_levels; ++k) {
            if (overlaps(grad_pred[i], ng, dpred[k], (size_t)n_elems[k] * 4))
                return fail(QPWC_E_ALIAS, "grad_pred overlaps a dpred buffer");
            if (k > i && overlaps(grad_pred[i], ng, grad_pred[k], (size_t)n_elems[k] * esize(pred_dtype[k])))
                return fail(QPWC_E_ALIAS, "two grad_pred buffers overlap");
        }
    }
    return loss_bwd_launch(dpred, (const float*)grad_losses, grad_pred, n_elems, pred_dtype, n_levels,
                           (hipStream_t)stream);
}

int64_t qpwc_augment_workspace_floats(int B, int h, int w) {
    const int rc = augment_check_shapes(B, 1, 1, h, w);
    return rc != QPWC_OK ? rc : augment_workspace_floats(B, h, w);
}

const char* qpwc_augment_fwd_kernel(int B, int h, int w, const void* out_ims, const void* out_flo) {
    if (!out_ims || !out_flo || augment_check_shapes(B, 1, 1, h, w) != QPWC_OK) return "";
    return augment_fwd_kernel(h, w, out_ims, out_flo);
}

int qpwc_augment_fwd(const void* ims, int ims_dtype, const void* flo, int B, int H, int W, const void* iparams,
                     const void* fparams, int h, int w, int flags, int layout, void* out_ims, void* out_flo,
                     void* workspace, void* stream) {
    if (flags & ~(QPWC_AUGMENT_COLOR | QPWC_AUGMENT_RAW)) return fail(QPWC_E_MODE, "unknown augment flags 0x%x", flags);
    const bool colour = flags & QPWC_AUGMENT_COLOR;
    if (!ims || !flo || !iparams || !fparams || !out_ims || !out_flo || (colour && !workspace))
        return fail(QPWC_E_NULL, "null pointer argument");
    if (ims_dtype != QPWC_F32 && ims_dtype != QPWC_U8) return fail(QPWC_E_DTYPE, "unsupported image dtype %d", ims_dtype);
    if (layout != QPWC_NHWC && layout != QPWC_NCHW) return fail(QPWC_E_LAYOUT, "Unsupported data format : %d", layout);
    int rc = augment_check_shapes(B, H, W, h, w);
    if (rc != QPWC_OK) return rc;
    const bool u8 = ims_dtype == QPWC_U8;
    const size_t src_px = (size_t)B * H * W, out_px = (size_t)B * h * w;
    // a uint8 pixel is read as three 2-byte pieces, an fp32 pixel and a flow vector as 8-byte pieces
    const BufCheck bufs[] = {
        {ims, src_px * 6 * (u8 ? 1 : 4), u8 ? (size_t)2 : (size_t)8, "ims"},
        {flo, src_px * 2 * 4, 8, "flo"},
        {iparams, (size_t)B * 6 * 4, 4, "iparams"},
        {fparams, (size_t)B * 6 * 4, 4, "fparams"},
        {out_ims, out_px * 6 * 4, 4, "out_ims"},
        {out_flo, out_px * 2 * 4, 4, "out_flo"},
        {workspace, (size_t)augment_workspace_floats(B, h, w) * 4, 4, "workspace"},
    };
    if ((rc = check_bufs(bufs, 4, colour ? 7 : 6)) != QPWC_OK) return rc;
    return augment_fwd_launch(ims, u8, (const float*)flo, B, H, W, (const int*)iparams, (const float*)fparams, h, w,
                              flags, layout, (float*)out_ims, (float*)out_flo, (float*)workspace,
                              (hipStream_t)stream);
}

const char* qpwc_augment_sparse_fwd_kernel(int B, int h, int w) {
    if (augment_check_shapes(B, 1, 1, h, w) != QPWC_OK) return "";
    return augment_sparse_fwd_kernel(h, w);
}

int qpwc_augment_sparse_fwd(const void* ims, int ims_dtype, const void* flo, const void* valid, int B, int H, int W,
                            const void* iparams, const void* fparams, int h, int w, int flags, int layout, void* out_ims,
                            void* out_flo, void* out_valid, void* workspace, void* stream) {
    if (flags & ~(QPWC_AUGMENT_COLOR | QPWC_AUGMENT_RAW)) return fail(QPWC_E_MODE, "unknown augment flags 0x%x", flags);
    const bool colour = flags & QPWC_AUGMENT_COLOR;
    if (!ims || !flo || !iparams || !fparams || !out_ims || !out_flo || !out_valid || (colour && !workspace))
        return fail(QPWC_E_NULL, "null pointer argument");
    if (ims_dtype != QPWC_F32 && ims_dtype != QPWC_U8) return fail(QPWC_E_DTYPE, "unsupported image dtype %d", ims_dtype);
    if (layout != QPWC_NHWC && layout != QPWC_NCHW) return fail(QPWC_E_LAYOUT, "Unsupported data format : %d", layout);
    int rc = augment_check_shapes(B, H, W, h, w);
    if (rc != QPWC_OK) return rc;
    const bool u8 = ims_dtype == QPWC_U8;
    const size_t src_px = (size_t)B * H * W, out_px = (size_t)B * h * w;
    // the sources as qpwc_augment_fwd reads them, the mask byte by byte; the form follows from the shape and decides the
    // grid the outputs must be on: the kernel does not look at the pointers
    const size_t oalign = augment_sparse_out_align(h, w);
    BufCheck bufs[9];
    int k = 0;
    bufs[k++] = indexed_buf(ims, src_px * 6 * (u8 ? 1 : 4), u8 ? 2 : 8, "ims", 0);
    bufs[k++] = indexed_buf(flo, src_px * 2 * 4, 8, "flo", 0);
    if (valid) bufs[k++] = indexed_buf(valid, src_px, 1, "valid", 0);
    bufs[k++] = indexed_buf(iparams, (size_t)B * 6 * 4, 4, "iparams", 0);
    bufs[k++] = indexed_buf(fparams, (size_t)B * 6 * 4, 4, "fparams", 0);
    const int n_in = k;
    bufs[k++] = indexed_buf(out_ims, out_px * 6 * 4, oalign, "out_ims", 0);
    bufs[k++] = indexed_buf(out_flo, out_px * 2 * 4, oalign, "out_flo", 0);
    bufs[k++] = indexed_buf(out_valid, out_px, oalign / 4, "out_valid", 0);
    if (colour) bufs[k++] = indexed_buf(workspace, (size_t)augment_workspace_floats(B, h, w) * 4, 4, "workspace", 0);
    if ((rc = check_bufs(bufs, n_in, k)) != QPWC_OK) return rc;
    return augment_sparse_fwd_launch(ims, u8, (const float*)flo, (const unsigned char*)valid, B, H, W,
                                     (const int*)iparams, (const float*)fparams, h, w, flags, layout, (float*)out_ims,
                                     (float*)out_flo, (unsigned char*)out_valid, (float*)workspace, (hipStream_t)stream);
}

int qpwc_epe_workspace_floats(void) { return epe_workspace_floats(); }

int qpwc_epe_fwd(const void* y_true, const void* y_pred, void* out_mean, void* workspace, int B,
                 int H, int W, int layout, void* stream) {
    if (!y_true || !y_pred || !out_mean || !workspace) return fail(QPWC_E_NULL, "null pointer argument");
    int rc = check_common(B, H, W, 2, layout, QPWC_F32);
    if (rc != QPWC_OK) return rc;
    if ((uintptr_t)y_true % 8 || (uintptr_t)y_pred % 8 || (uintptr_t)out_mean % 4 ||
        (uintptr_t)workspace % 4)
        return fail(QPWC_E_ALIGN, "flow pointers must be 8-byte aligned");
    return epe_launch((const float*)y_true, (const float*)y_pred, (float*)out_mean,
                      (float*)workspace, B, H, W, layout, (hipStream_t)stream);
}

int qpwc_dwconv3x3_fwd(const void* const* src, const int* src_channels,
                       const int64_t* src_pixel_stride, int n_src, int mish_on_load,
                       const void* weight, void* out, int B, int H, int W, int dtype, void* stream) {
    if (!src || !src_channels || !src_pixel_stride || !weight || !out)
        return fail(QPWC_E_NULL, "null pointer argument");
    if (dtype != QPWC_F32 && dtype != QPWC_F16) return fail(QPWC_E_DTYPE, "unsupported dtype %d", dtype);
    const size_t es = esize(dtype);
    if (n_src < 1 || n_src > 3) return fail(QPWC_E_SHAPE, "n_src %d outside [1,3]", n_src);
    if (B <= 0 || H <= 0 || W <= 0) return fail(QPWC_E_SHAPE, "non-positive extent B=%d H=%d W=%d", B, H, W);
    int64_t C = 0;
    for (int i = 0; i < n_src; ++i) {
        if (!src[i]) return fail(QPWC_E_NULL, "null source %d", i);
        if (src_channels[i] <= 0 || src_pixel_stride[i] < src_channels[i])
            return fail(QPWC_E_STRIDE, "source %d: %d channels at pixel stride %lld", i,
                        src_channels[i], (long long)src_pixel_stride[i]);
        if ((uintptr_t)src[i] % es) return fail(QPWC_E_ALIGN, "source %d not element aligned", i);
        C += src_channels[i];
    }
    if ((uintptr_t)out % es || (uintptr_t)weight % 4) return fail(QPWC_E_ALIGN, "pointer not element aligned");
    const size_t n_out = (size_t)B * H * W * C * es;
    for (int i = 0; i < n_src; ++i)
        if (overlaps(out, n_out, src[i], (((size_t)B * H * W - 1) * src_pixel_stride[i] + src_channels[i]) * es))
            return fail(QPWC_E_ALIAS, "out overlaps source %d", i);
    if ((int64_t)W * C > INT32_MAX) return fail(QPWC_E_SHAPE, "row too long");
    return dwconv3x3_launch(src, src_channels, src_pixel_stride, n_src, mish_on_load, weight, out, B,
                            H, W, dtype, (hipStream_t)stream);
}

// The fused SeparableConv2D forwards.  es: the element size of the sources and of out (4: fp32 and bf16x3, 2: fp16);
// pw_name: what the messages call the pointwise operand.  The order is part of the contract: null, stride, alignment
// and aliasing source by source, only then the alignment of out / pw / bias, and mish_flags last.
static int sepconv_fwd_check(const void* const* src, const int* src_channels, const int64_t* src_pixel_stride, int n_src,
                             int mish_flags, const void* dw, const void* pw, const void* bias, const void* out, int B,
                             int H, int W, int F, size_t es, const char* pw_name) {
    if (!src || !src_channels || !src_pixel_stride || !dw || !pw || !bias || !out)
        return fail(QPWC_E_NULL, "null pointer argument");
    if (n_src < 1 || n_src > 3) return fail(QPWC_E_SHAPE, "n_src %d outside [1,3]", n_src);
    if (B <= 0 || H <= 0 || W <= 0) return fail(QPWC_E_SHAPE, "non-positive extent B=%d H=%d W=%d", B, H, W);
    if (F != 16 && F != 32 && F != 64 && F != 128) return fail(QPWC_E_SHAPE, "F=%d not in {16,32,64,128}", F);
    for (int i = 0; i < n_src; ++i) {
        if (!src[i]) return fail(QPWC_E_NULL, "null source %d", i);
        if (src_channels[i] <= 0 || src_pixel_stride[i] < src_channels[i])
            return fail(QPWC_E_STRIDE, "source %d: %d channels at pixel stride %lld", i, src_channels[i],
                        (long long)src_pixel_stride[i]);
        if (es == 2) {
            // 8-byte loads of 4 channels: every source but a short (< 4 channel) last one
            const bool tail = i + 1 == n_src && src_channels[i] < 4;
            if (!tail && (src_channels[i] % 4 || src_pixel_stride[i] % 4 || (uintptr_t)src[i] % 8))
                return fail(QPWC_E_ALIGN, "source %d: %d channels at stride %lld must be multiples of 4, 8-byte aligned",
                            i, src_channels[i], (long long)src_pixel_stride[i]);
            if ((uintptr_t)src[i] % 2) return fail(QPWC_E_ALIGN, "source %d not element aligned", i);
        } else if ((uintptr_t)src[i] % 4) {
            return fail(QPWC_E_ALIGN, "source %d not 4-byte aligned", i);
        }
        if (overlaps(out, (size_t)B * H * W * F * es, src[i],
                     (((size_t)B * H * W - 1) * src_pixel_stride[i] + src_channels[i]) * es))
            return fail(QPWC_E_ALIAS, "out overlaps source %d", i);
        if (es == 2 && (int64_t)H * W * src_pixel_stride[i] > INT32_MAX) return fail(QPWC_E_SHAPE, "image too large");
    }
    if ((uintptr_t)out % 16 || (uintptr_t)pw % 16 || (uintptr_t)bias % 16 || (uintptr_t)dw % 4)
        return fail(QPWC_E_ALIGN, "out, %s, bias must be 16-byte aligned", pw_name);
    if (mish_flags < 0 || mish_flags > 3) return fail(QPWC_E_SHAPE, "mish_flags %d outside [0,3]", mish_flags);
    return QPWC_OK;
}

int qpwc_sepconv3x3_fwd(const void* const* src, const int* src_channels,
                        const int64_t* src_pixel_stride, int n_src, int mish_flags, const void* dw,
                        const void* pw, const void* bias, void* out, int B, int H, int W, int F,
                        void* stream) {
    const int rc = sepconv_fwd_check(src, src_channels, src_pixel_stride, n_src, mish_flags, dw, pw, bias, out, B, H, W,
                                     F, 4, "pw");
    return rc != QPWC_OK ? rc
                         : sepconv3x3_launch(src, src_channels, src_pixel_stride, n_src, mish_flags, dw, pw, bias, out,
                                             B, H, W, F, (hipStream_t)stream);
}

static int sepconv_bwd_check_shape(int B, int H, int W, int64_t C, int F) {
    if (B <= 0 || H <= 0 || W <= 0 || C <= 0)
        return fail(QPWC_E_SHAPE, "non-positive extent B=%d H=%d W=%d C=%lld", B, H, W, (long long)C);
    if (F != 16 && F != 32 && F != 64 && F != 128) return fail(QPWC_E_SHAPE, "F=%d not in {16,32,64,128}", F);
    if (C > (1 << 20) || !sepconv3x3_bwd_shape_ok(B, H, W, (int)C, F))
        return fail(QPWC_E_SHAPE, "B=%d H=%d W=%d C=%lld: too large for the backward's launch grids", B, H, W, (long long)C);
    return QPWC_OK;
}

int64_t qpwc_sepconv3x3_bwd_workspace_floats(int B, int H, int W, int C, int F) {
    const int rc = sepconv_bwd_check_shape(B, H, W, C, F);
    return rc != QPWC_OK ? rc : sepconv3x3_bwd_workspace_floats(B, H, W, C, F);
}

int qpwc_sepconv3x3_bwd(const void* const* src, const int* src_channels, const int64_t* src_pixel_stride, int n_src,
                        int mish_flags, const void* dw, const void* pw, const void* bias, const void* grad_out,
                        void* const* grad_src, void* grad_dw, void* grad_pw, void* grad_bias, void* workspace, int B,
                        int H, int W, int F, void* stream) {
    int rc = check_nonnull({{src, "src"}, {src_channels, "src_channels"}, {src_pixel_stride, "src_pixel_stride"},
                            {dw, "dw"}, {pw, "pw"}, {bias, "bias"}, {grad_out, "grad_out"}, {workspace, "workspace"}});
    if (rc != QPWC_OK) return rc;
    if (n_src < 1 || n_src > 3) return fail(QPWC_E_SHAPE, "n_src %d outside [1,3]", n_src);
    if (mish_flags < 0 || mish_flags > 3) return fail(QPWC_E_SHAPE, "mish_flags %d outside [0,3]", mish_flags);
    int64_t C = 0;
    bool any_out = grad_dw || grad_pw || grad_bias;
    for (int i = 0; i < n_src; ++i) {
        if (!src[i]) return fail(QPWC_E_NULL, "src[%d] is null", i);
        if (src_channels[i] <= 0 || src_pixel_stride[i] < src_channels[i])
            return fail(QPWC_E_SHAPE, "src[%d]: %d channels at pixel stride %lld", i, src_channels[i],
                        (long long)src_pixel_stride[i]);
        C += src_channels[i];
        any_out |= grad_src && grad_src[i];
    }
    if (!any_out) return fail(QPWC_E_NULL, "grad_src, grad_dw, grad_pw and grad_bias are all null");
    if ((rc = sepconv_bwd_check_shape(B, H, W, C, F)) != QPWC_OK) return rc;
    const size_t M = (size_t)B * H * W, cpad = (size_t)(C + 31) / 32 * 32;
    BufCheck bufs[14];
    int n_in = 0;
    for (int i = 0; i < n_src; ++i)
        bufs[n_in++] = indexed_buf(src[i], ((M - 1) * (size_t)src_pixel_stride[i] + src_channels[i]) * 4, 4, "src[%d]", i);
    bufs[n_in++] = {dw, (size_t)C * 9 * 4, 4, "dw"};
    bufs[n_in++] = {pw, (size_t)F * cpad * 4, 16, "pw"};
    bufs[n_in++] = {bias, (size_t)F * 4, 4, "bias"};
    bufs[n_in++] = {grad_out, M * F * 4, 16, "grad_out"};
    int n_all = n_in;
    for (int i = 0; i < n_src; ++i)
        if (grad_src && grad_src[i])
            bufs[n_all++] = indexed_buf(grad_src[i], M * src_channels[i] * 4, 4, "grad_src[%d]", i);
    if (grad_dw) bufs[n_all++] = {grad_dw, (size_t)C * 9 * 4, 4, "grad_dw"};
    if (grad_pw) bufs[n_all++] = {grad_pw, (size_t)F * cpad * 4, 16, "grad_pw"};
    if (grad_bias) bufs[n_all++] = {grad_bias, (size_t)F * 4, 4, "grad_bias"};
    bufs[n_all++] = {workspace, (size_t)sepconv3x3_bwd_workspace_floats(B, H, W, (int)C, F) * 4, 16, "workspace"};
    if ((rc = check_bufs(bufs, n_in, n_all)) != QPWC_OK) return rc;
    return sepconv3x3_bwd_launch(src, src_channels, src_pixel_stride, n_src, mish_flags, dw, pw, bias, grad_out, grad_src,
                                 grad_dw, grad_pw, grad_bias, workspace, B, H, W, F, (hipStream_t)stream);
}

int qpwc_sepconv3x3_x3_fwd(const void* const* src, const int* src_channels, const int64_t* src_pixel_stride,
                           int n_src, int mish_flags, const void* dw, const void* pw3, const void* bias, void* out,
                           int B, int H, int W, int F, void* stream) {
    const int rc = sepconv_fwd_check(src, src_channels, src_pixel_stride, n_src, mish_flags, dw, pw3, bias, out, B, H,
                                     W, F, 4, "pw3");
    return rc != QPWC_OK ? rc
                         : sepconv3x3_x3_launch(src, src_channels, src_pixel_stride, n_src, mish_flags, dw, pw3, bias,
                                                out, B, H, W, F, (hipStream_t)stream);
}

int qpwc_sepconv3x3_f16_fwd(const void* const* src, const int* src_channels, const int64_t* src_pixel_stride,
                            int n_src, int mish_flags, const void* dw, const void* pw, const void* bias,
                            void* out, int B, int H, int W, int F, void* stream) {
    const int rc = sepconv_fwd_check(src, src_channels, src_pixel_stride, n_src, mish_flags, dw, pw, bias, out, B, H, W,
                                     F, 2, "pw");
    return rc != QPWC_OK ? rc
                         : sepconv3x3_f16_launch(src, src_channels, src_pixel_stride, n_src, mish_flags, dw, pw, bias,
                                                 out, B, H, W, F, (hipStream_t)stream);
}

int qpwc_pointwise_bias_fwd(const void* y, const void* weight, const void* bias, void* out, int64_t M, int C, int F,
                            void* stream) {
    if (!y || !weight || !bias || !out) return fail(QPWC_E_NULL, "null pointer argument");
    if (M <= 0 || C <= 0) return fail(QPWC_E_SHAPE, "non-positive extent M=%lld C=%d", (long long)M, C);
    if (F != 16 && F != 32 && F != 64 && F != 128 && F != 256) return fail(QPWC_E_SHAPE, "F=%d not in {16,32,64,128,256}", F);
    if (M * (int64_t)(C > F ? C : F) >= INT32_MAX) return fail(QPWC_E_SHAPE, "M x max(C, F) must stay below 2^31");
    if ((uintptr_t)y % 16 || (uintptr_t)weight % 16 || (uintptr_t)bias % 16 || (uintptr_t)out % 16)
        return fail(QPWC_E_ALIGN, "y, weight, bias, out must be 16-byte aligned");
    const int cpad = (C + 31) / 32 * 32;
    if (overlaps(out, (size_t)M * F * 4, y, (size_t)M * C * 4)) return fail(QPWC_E_ALIAS, "out overlaps y");
    return pointwise_bias_launch(y, weight, bias, out, M, C, cpad, F, (hipStream_t)stream);
}

int qpwc_flow_head_param_floats(void) { return flow_head_param_floats(); }

int qpwc_flow_head_up_fwd(const void* z, const void* params, void* out, void* out_up, void* out_up_f32, int B, int H, int W,
                          float scale, float up_scale, int dtype, void* stream) {
    if (!z || !params || !out || !out_up) return fail(QPWC_E_NULL, "null pointer argument");
    if (dtype != QPWC_F32 && dtype != QPWC_F16) return fail(QPWC_E_DTYPE, "unsupported dtype %d", dtype);
    const size_t es = esize(dtype);
    if (B <= 0 || H <= 0 || W <= 0) return fail(QPWC_E_SHAPE, "non-positive extent B=%d H=%d W=%d", B, H, W);
    if ((int64_t)B * 4 * H * W * 2 >= INT32_MAX) return fail(QPWC_E_SHAPE, "upsampled flow too large for 32-bit pixel indices");
    if ((uintptr_t)z % (4 * es) || (uintptr_t)out % (2 * es) || (uintptr_t)out_up % (4 * es) || (uintptr_t)params % 4)
        return fail(QPWC_E_ALIGN, "z and out_up must be aligned to 4 elements, out to 2");
    const size_t nz = (size_t)B * H * W * 16 * es, no = (size_t)B * H * W * 2 * es, nu = 4 * no;
    if (overlaps(out, no, z, nz) || overlaps(out_up, nu, z, nz) || overlaps(out_up, nu, out, no))
        return fail(QPWC_E_ALIAS, "out / out_up overlap z or each other");
    if (out_up_f32) {
        if (dtype != QPWC_F16) return fail(QPWC_E_DTYPE, "out_up_f32 is the fp32 copy of an fp16 out_up: pass NULL for fp32 storage");
        if ((uintptr_t)out_up_f32 % 16) return fail(QPWC_E_ALIGN, "out_up_f32 must be 16-byte aligned");
        if (overlaps(out_up_f32, (size_t)B * 4 * H * W * 2 * 4, z, nz) || overlaps(out_up_f32, (size_t)B * 4 * H * W * 2 * 4, out, no) ||
            overlaps(out_up_f32, (size_t)B * 4 * H * W * 2 * 4, out_up, nu))
            return fail(QPWC_E_ALIAS, "out_up_f32 overlaps another operand");
    }
    return flow_head_up_launch(z, params, out, out_up, out_up_f32, B, H, W, scale, up_scale, dtype, (hipStream_t)stream);
}

int qpwc_flow_head_fwd(const void* z, const void* params, void* out, int B, int H, int W, float scale,
                       int dtype, int out_layout, void* stream) {
    if (!z || !params || !out) return fail(QPWC_E_NULL, "null pointer argument");
    if (out_layout != QPWC_NHWC && out_layout != QPWC_NCHW)
        return fail(QPWC_E_LAYOUT, "Unsupported data format : %d", out_layout);
    if (dtype != QPWC_F32 && dtype != QPWC_F16) return fail(QPWC_E_DTYPE, "unsupported dtype %d", dtype);
    const size_t es = esize(dtype);
    if (B <= 0 || H <= 0 || W <= 0) return fail(QPWC_E_SHAPE, "non-positive extent B=%d H=%d W=%d", B, H, W);
    if ((uintptr_t)z % (4 * es) || (uintptr_t)out % (2 * es) || (uintptr_t)params % 4)
        return fail(QPWC_E_ALIGN, "z must be aligned to 4 elements, out to 2");
    if (overlaps(out, (size_t)B * H * W * 2 * es, z, (size_t)B * H * W * 16 * es))
        return fail(QPWC_E_ALIAS, "out overlaps z");
    return flow_head_launch(z, params, out, B, H, W, scale, dtype, out_layout, (hipStream_t)stream);
}

int64_t qpwc_flow_head_stats_workspace_floats(int B, int H, int W) {
    const int rc = flow_head_train_check_shape(B, H, W);
    return rc != QPWC_OK ? rc : flow_head_stats_workspace_floats(B, H, W);
}

int qpwc_flow_head_stats_fwd(const void* z, const void* w1, const void* b1, const void* gamma, const void* beta,
                             const void* wf, void* moving_mean, void* moving_var, float momentum, float eps,
                             void* params, void* stats, void* workspace, int B, int H, int W, void* stream) {
    int rc = check_nonnull({{z, "z"}, {w1, "w1"}, {b1, "b1"}, {gamma, "gamma"}, {beta, "beta"}, {wf, "wf"},
                            {params, "params"}, {workspace, "workspace"}});
    if (rc != QPWC_OK) return rc;
    if (!moving_mean != !moving_var) return fail(QPWC_E_NULL, "moving_mean and moving_var: both or neither");
    if ((rc = flow_head_train_check_shape(B, H, W)) != QPWC_OK) return rc;
    if (!(eps > 0.0f)) return fail(QPWC_E_RANGE, "eps %g must be positive", (double)eps);
    if (!(momentum >= 0.0f && momentum <= 1.0f)) return fail(QPWC_E_RANGE, "momentum %g outside [0,1]", (double)momentum);
    const size_t M = (size_t)B * H * W;
    BufCheck bufs[11];
    int n_in = 0;
    bufs[n_in++] = {z, M * 64, 16, "z"};
    bufs[n_in++] = {w1, 1024, 16, "w1"};
    bufs[n_in++] = {b1, 64, 16, "b1"};
    bufs[n_in++] = {gamma, 64, 4, "gamma"};
    bufs[n_in++] = {beta, 64, 4, "beta"};
    bufs[n_in++] = {wf, 1152, 4, "wf"};
    int n_all = n_in;
    bufs[n_all++] = {params, 592 * 4, 16, "params"};
    if (stats) bufs[n_all++] = {stats, 192, 16, "stats"};
    if (moving_mean) {
        bufs[n_all++] = {moving_mean, 64, 4, "moving_mean"};
        bufs[n_all++] = {moving_var, 64, 4, "moving_var"};
    }
    bufs[n_all++] = {workspace, (size_t)flow_head_stats_workspace_floats(B, H, W) * 4, 16, "workspace"};
    if ((rc = check_bufs(bufs, n_in, n_all)) != QPWC_OK) return rc;
    return flow_head_stats_launch(z, w1, b1, gamma, beta, wf, moving_mean, moving_var, momentum, eps, params, stats,
                                  workspace, B, H, W, (hipStream_t)stream);
}

int64_t qpwc_flow_head_bwd_workspace_floats(int B, int H, int W) {
    const int rc = flow_head_train_check_shape(B, H, W);
    return rc != QPWC_OK ? rc : flow_head_bwd_workspace_floats(B, H, W);
}

int qpwc_flow_head_bwd(const void* z, const void* params, const void* stats, float eps, int training, float scale,
                       const void* grad_out, void* grad_z, void* grad_w1, void* grad_b1, void* grad_gamma,
                       void* grad_beta, void* grad_wf, void* workspace, int B, int H, int W, void* stream) {
    int rc = check_nonnull({{z, "z"}, {params, "params"}, {stats, "stats"}, {grad_out, "grad_out"},
                            {workspace, "workspace"}});
    if (rc != QPWC_OK) return rc;
    if (!grad_z && !grad_w1 && !grad_b1 && !grad_gamma && !grad_beta && !grad_wf)
        return fail(QPWC_E_NULL, "grad_z, grad_w1, grad_b1, grad_gamma, grad_beta and grad_wf are all null");
    if ((rc = flow_head_train_check_shape(B, H, W)) != QPWC_OK) return rc;
    if (!(eps > 0.0f)) return fail(QPWC_E_RANGE, "eps %g must be positive", (double)eps);
    const size_t M = (size_t)B * H * W;
    BufCheck bufs[11];
    int n_in = 0;
    bufs[n_in++] = {z, M * 64, 16, "z"};
    bufs[n_in++] = {params, 592 * 4, 16, "params"};
    bufs[n_in++] = {stats, 192, 16, "stats"};
    bufs[n_in++] = {grad_out, M * 8, 8, "grad_out"};
    int n_all = n_in;
    if (grad_z) bufs[n_all++] = {grad_z, M * 64, 16, "grad_z"};
    if (grad_w1) bufs[n_all++] = {grad_w1, 1024, 4, "grad_w1"};
    if (grad_b1) bufs[n_all++] = {grad_b1, 64, 4, "grad_b1"};
    if (grad_gamma) bufs[n_all++] = {grad_gamma, 64, 4, "grad_gamma"};
    if (grad_beta) bufs[n_all++] = {grad_beta, 64, 4, "grad_beta"};
    if (grad_wf) bufs[n_all++] = {grad_wf, 1152, 4, "grad_wf"};
    bufs[n_all++] = {workspace, (size_t)flow_head_bwd_workspace_floats(B, H, W) * 4, 16, "workspace"};
    if ((rc = check_bufs(bufs, n_in, n_all)) != QPWC_OK) return rc;
    return flow_head_bwd_launch(z, params, stats, eps, training, scale, grad_out, grad_z, grad_w1, grad_b1, grad_gamma,
                                grad_beta, grad_wf, workspace, B, H, W, (hipStream_t)stream);
}

int qpwc_upsample2x_flow_bwd(const void* grad_out, void* grad_in, int B, int h, int w, float scale, void* stream) {
    int rc = check_nonnull({{grad_out, "grad_out"}, {grad_in, "grad_in"}});
    if (rc != QPWC_OK) return rc;
    if (B <= 0 || h <= 0 || w <= 0) return fail(QPWC_E_SHAPE, "non-positive extent B=%d h=%d w=%d", B, h, w);
    if (h > (1 << 29) || w > (1 << 29)) return fail(QPWC_E_SHAPE, "h=%d w=%d: the doubled extents must fit an int", h, w);
    const size_t n = (size_t)B * h * w * 8;
    const BufCheck bufs[2] = {{grad_out, 4 * n, 8, "grad_out"}, {grad_in, n, 8, "grad_in"}};
    if ((rc = check_bufs(bufs, 1, 2)) != QPWC_OK) return rc;
    return upsample2x_flow_bwd_launch(grad_out, grad_in, B, h, w, scale, (hipStream_t)stream);
}

int qpwc_optflow_tail_fwd(const void* z2, const void* dw3, const void* pw3, const void* b3, const void* dw4,
                          const void* pw4, const void* b4, const void* head_params, void* out, int B, int H, int W,
                          float scale, int mish_on_load, int out_layout, void* stream) {
    if (!z2 || !dw3 || !pw3 || !b3 || !dw4 || !pw4 || !b4 || !head_params || !out)
        return fail(QPWC_E_NULL, "null pointer argument");
    if (out_layout != QPWC_NHWC && out_layout != QPWC_NCHW)
        return fail(QPWC_E_LAYOUT, "Unsupported data format : %d", out_layout);
    if (B <= 0 || H <= 0 || W <= 0) return fail(QPWC_E_SHAPE, "non-positive extent B=%d H=%d W=%d", B, H, W);
    if ((uintptr_t)z2 % 16 || (uintptr_t)pw3 % 16 || (uintptr_t)pw4 % 16 || (uintptr_t)b3 % 16 || (uintptr_t)b4 % 16 ||
        (uintptr_t)head_params % 16 || (uintptr_t)dw3 % 4 || (uintptr_t)dw4 % 4 || (uintptr_t)out % 8)
        return fail(QPWC_E_ALIGN, "z2, pw3, pw4, b3, b4, head_params must be 16-byte aligned, out 8-byte");
    if (overlaps(out, (size_t)B * H * W * 2 * 4, z2, (size_t)B * H * W * 64 * 4)) return fail(QPWC_E_ALIAS, "out overlaps z2");
    return optflow_tail_launch(z2, dw3, pw3, b3, dw4, pw4, b4, head_params, out, B, H, W, scale, mish_on_load,
                               out_layout, (hipStream_t)stream);
}

int qpwc_bias_mish_fwd(void* x, const void* bias, int64_t n_pixels, int C, int dtype, void* stream) {
    if (!x) return fail(QPWC_E_NULL, "null pointer argument");
    if (dtype != QPWC_F32 && dtype != QPWC_F16) return fail(QPWC_E_DTYPE, "unsupported dtype %d", dtype);
    if (n_pixels <= 0 || C <= 0 || C % 4) return fail(QPWC_E_SHAPE, "need n_pixels > 0 and C %% 4 == 0 (C=%d)", C);
    if ((uintptr_t)x % (4 * esize(dtype)) || (uintptr_t)bias % 16)
        return fail(QPWC_E_ALIGN, "x must be aligned to 4 elements, bias to 16 bytes");
    return bias_mish_launch(x, bias, n_pixels, C, dtype, (hipStream_t)stream);
}

int qpwc_bias_mish_pad_fwd(const void* src, const void* bias, void* dst, int B, int H, int W, int C,
                           int pad_h, int pad_w, int64_t dst_pixel_stride, int dtype, void* stream) {
    if (!src || !dst) return fail(QPWC_E_NULL, "null pointer argument");
    if (dtype != QPWC_F32 && dtype != QPWC_F16) return fail(QPWC_E_DTYPE, "unsupported dtype %d", dtype);
    if (B <= 0 || H <= 0 || W <= 0 || C <= 0 || C % 4 || pad_h < 0 || pad_w < 0)
        return fail(QPWC_E_SHAPE, "bad shape B=%d H=%d W=%d C=%d pad=%d,%d", B, H, W, C, pad_h, pad_w);
    if (dst_pixel_stride < C || dst_pixel_stride % 4)
        return fail(QPWC_E_STRIDE, "dst_pixel_stride %lld must be >= C and a multiple of 4",
                    (long long)dst_pixel_stride);
    const size_t es = esize(dtype);
    if ((uintptr_t)src % (4 * es) || (uintptr_t)dst % (4 * es) || (uintptr_t)bias % 16)
        return fail(QPWC_E_ALIGN, "src/dst must be aligned to 4 elements, bias to 16 bytes");
    if (overlaps(dst, (size_t)B * (H + pad_h) * (W + pad_w) * dst_pixel_stride * es, src,
                 (size_t)B * H * W * C * es))
        return fail(QPWC_E_ALIAS, "dst overlaps src");
    return bias_mish_pad_launch(src, bias, dst, B, H, W, C, pad_h, pad_w, dst_pixel_stride, dtype,
                                (hipStream_t)stream);
}

int qpwc_split_frames_pad_fwd(const void* in, void* out, int B, int H, int W, int pad_h, int pad_w,
                              int dtype, void* stream) {
    if (!in || !out) return fail(QPWC_E_NULL, "null pointer argument");
    if (dtype != QPWC_F32 && dtype != QPWC_F16) return fail(QPWC_E_DTYPE, "unsupported dtype %d", dtype);
    if (B <= 0 || H <= 0 || W <= 0 || pad_h < 0 || pad_w < 0)
        return fail(QPWC_E_SHAPE, "bad shape B=%d H=%d W=%d pad=%d,%d", B, H, W, pad_h, pad_w);
    const size_t es = esize(dtype);
    if ((uintptr_t)in % es || (uintptr_t)out % es) return fail(QPWC_E_ALIGN, "pointer not element aligned");
    if (overlaps(out, (size_t)2 * B * (H + pad_h) * (W + pad_w) * 3 * es, in, (size_t)B * H * W * 6 * es))
        return fail(QPWC_E_ALIAS, "out overlaps in");
    return split_frames_pad_launch(in, out, B, H, W, pad_h, pad_w, dtype, (hipStream_t)stream);
}

int qpwc_upsample2x_flow_fwd(const void* in, void* out, int B, int h, int w, float scale, int dtype,
                             int in_layout, int out_layout, void* stream) {
    if (!in || !out) return fail(QPWC_E_NULL, "null pointer argument");
    if ((in_layout != QPWC_NHWC && in_layout != QPWC_NCHW) || (out_layout != QPWC_NHWC && out_layout != QPWC_NCHW))
        return fail(QPWC_E_LAYOUT, "Unsupported data format : %d / %d", in_layout, out_layout);
    if (dtype != QPWC_F32 && dtype != QPWC_F16) return fail(QPWC_E_DTYPE, "unsupported dtype %d", dtype);
    const size_t es = esize(dtype);
    if (B <= 0 || h <= 0 || w <= 0) return fail(QPWC_E_SHAPE, "non-positive extent B=%d h=%d w=%d", B, h, w);
    if ((uintptr_t)in % es || (uintptr_t)out % es) return fail(QPWC_E_ALIGN, "flow pointers must be element aligned");
    if (overlaps(out, (size_t)B * 4 * h * w * 2 * es, in, (size_t)B * h * w * 2 * es))
        return fail(QPWC_E_ALIAS, "out overlaps in");
    return upsample2x_flow_launch(in, out, B, h, w, scale, dtype, in_layout, out_layout, (hipStream_t)stream);
}

int qpwc_epe_multi_workspace_floats(void) { return epe_multi_workspace_floats(); }

// pred_dtype: one storage dtype per prediction (mixed), or null for all fp32
static int epe_multi_checked(const void* const* y_true, const void* const* y_pred, const int64_t* n_pixels,
                             const int64_t* plane_pixels, const int* pred_dtype, bool mixed, int n_levels,
                             void* out_means, void* workspace, void* stream) {
    if (!y_true || !y_pred || !n_pixels || (mixed && !pred_dtype) || !out_means || !workspace)
        return fail(QPWC_E_NULL, "null pointer argument");
    if (n_levels < 1 || n_levels > 8) return fail(QPWC_E_SHAPE, "n_levels %d outside [1,8]", n_levels);
    for (int i = 0; i < n_levels; ++i) {
        if (!y_true[i] || !y_pred[i]) return fail(QPWC_E_NULL, "null flow pointer at level %d", i);
        if (mixed && pred_dtype[i] != QPWC_F32 && pred_dtype[i] != QPWC_F16)
            return fail(QPWC_E_DTYPE, "level %d: unsupported prediction dtype %d", i, pred_dtype[i]);
        if (n_pixels[i] <= 0) return fail(QPWC_E_SHAPE, "level %d has no pixels", i);
        const bool planar = plane_pixels && plane_pixels[i] > 0;
        if (planar && n_pixels[i] % plane_pixels[i])
            return fail(QPWC_E_SHAPE, "level %d: %lld pixels are not whole planes of %lld", i,
                        (long long)n_pixels[i], (long long)plane_pixels[i]);
        const int pes = mixed && pred_dtype[i] == QPWC_F16 ? 2 : 4;
        if ((uintptr_t)y_true[i] % (planar ? 4 : 8) || (uintptr_t)y_pred[i] % (planar ? pes : 2 * pes))
            return fail(QPWC_E_ALIGN, mixed ? "flow pointers must be aligned to a pixel (channels-last) / an element (planes)"
                                            : "flow pointers must be 8-byte (pixels) / 4-byte (planes) aligned");
    }
    return epe_multi_launch(y_true, y_pred, n_pixels, plane_pixels, pred_dtype, n_levels, (float*)out_means,
                            (float*)workspace, (hipStream_t)stream);
}

int qpwc_epe_multi_fwd(const void* const* y_true, const void* const* y_pred, const int64_t* n_pixels,
                       const int64_t* plane_pixels, int n_levels, void* out_means, void* workspace,
                       void* stream) {
    return epe_multi_checked(y_true, y_pred, n_pixels, plane_pixels, nullptr, false, n_levels, out_means, workspace, stream);
}

int qpwc_epe_multi_mixed_fwd(const void* const* y_true, const void* const* y_pred, const int64_t* n_pixels,
                             const int64_t* plane_pixels, const int* pred_dtype, int n_levels, void* out_means,
                             void* workspace, void* stream) {
    return epe_multi_checked(y_true, y_pred, n_pixels, plane_pixels, pred_dtype, true, n_levels, out_means, workspace,
                             stream);
}

int qpwc_cost_volume_to_flow_fwd(const void* cvol, void* flow, int B, int H, int W, int D,
                                 int64_t pixel_stride, int layout, int dtype, void* stream) {
    if (!cvol || !flow) return fail(QPWC_E_NULL, "null pointer argument");
    const int rc = check_common(B, H, W, D, layout, dtype);
    if (rc) return rc;
    if (layout == QPWC_NHWC ? pixel_stride < D : pixel_stride != D)
        return fail(QPWC_E_STRIDE, "pixel stride %lld for %d channels", (long long)pixel_stride, D);
    if ((uintptr_t)cvol % esize(dtype) || (uintptr_t)flow % 8)
        return fail(QPWC_E_ALIGN, "cvol must be element aligned, flow 8-byte aligned");
    if (overlaps(flow, (size_t)B * H * W * 8, cvol, (size_t)B * H * W * pixel_stride * esize(dtype)))
        return fail(QPWC_E_ALIAS, "flow overlaps cvol");
    return cost_volume_to_flow_launch(cvol, (float*)flow, B, H, W, D, pixel_stride, layout, dtype,
                                      (hipStream_t)stream);
}

static int check_flow_args(const void* flow, const void* out, int B, int H, int W, int layout, int dtype,
                           size_t out_bytes) {
    if (!flow || !out) return fail(QPWC_E_NULL, "null pointer argument");
    const int rc = check_common(B, H, W, 2, layout, dtype);
    if (rc) return rc;
    const size_t es = esize(dtype);
    if ((uintptr_t)flow % es || (uintptr_t)out % es)
        return fail(QPWC_E_ALIGN, "pointer not element aligned");
    if ((int64_t)B * H * W * 2 >= ((int64_t)1 << 40)) return fail(QPWC_E_SHAPE, "flow too large");
    if (overlaps(out, out_bytes, flow, (size_t)B * H * W * 2 * es)) return fail(QPWC_E_ALIAS, "out overlaps flow");
    return QPWC_OK;
}

int qpwc_invert_flow_fwd(const void* flow, void* out, int B, int H, int W, int layout, int dtype,
                         void* stream) {
    const int rc = check_flow_args(flow, out, B, H, W, layout, dtype,
                                   (size_t)(B > 0 ? B : 0) * (H > 0 ? H : 0) * (W > 0 ? W : 0) * 2 * esize(dtype));
    if (rc) return rc;
    return invert_flow_launch(flow, out, B, H, W, layout, dtype, (hipStream_t)stream);
}

int qpwc_occlusion_fwd(const void* flow, void* out, int B, int H, int W, int layout, int dtype,
                       void* stream) {
    const int rc = check_flow_args(flow, out, B, H, W, layout, dtype,
                                   (size_t)(B > 0 ? B : 0) * (H > 0 ? H : 0) * (W > 0 ? W : 0) * 4);
    if (rc) return rc;
    if ((uintptr_t)out % 4) return fail(QPWC_E_ALIGN, "out must be 4-byte aligned");
    return occlusion_launch(flow, out, B, H, W, layout, dtype, (hipStream_t)stream);
}

// ---- The encoder and decoder forwards: one checker per layer, an export per arithmetic (fp32, bf16x3, fp16).
// es: the element size of x and out (4: fp32 and bf16x3, 2: fp16); w_name: what the messages call the weight operand.

static int conv3x3_mish_check(const void* x, const void* weight, const void* bias, const void* out, int B, int H, int W,
                              int C, int pad_h, int pad_w, size_t es, const char* w_name) {
    if (!x || !weight || !bias || !out) return fail(QPWC_E_NULL, "null pointer argument");
    if (C != 16 && C != 32 && C != 64 && C != 128 && C != 256)
        return fail(QPWC_E_SHAPE, "C=%d not in {16,32,64,128,256}", C);
    if (B <= 0 || H <= 0 || W <= 0 || pad_h < 0 || pad_w < 0 || pad_h > 8 || pad_w > 8)
        return fail(QPWC_E_SHAPE, "bad shape B=%d H=%d W=%d pad=%d,%d", B, H, W, pad_h, pad_w);
    if ((uintptr_t)x % 16 || (uintptr_t)weight % 16 || (uintptr_t)bias % 16 || (uintptr_t)out % 16)
        return fail(QPWC_E_ALIGN, "x, %s, bias, out must be 16-byte aligned", w_name);
    if (overlaps(out, (size_t)B * (H + pad_h) * (W + pad_w) * C * es, x, (size_t)B * H * W * C * es))
        return fail(QPWC_E_ALIAS, "out overlaps x");
    return QPWC_OK;
}

int qpwc_conv3x3_mish_fwd(const void* x, const void* weight, const void* bias, void* out, int B, int H,
                          int W, int C, int pad_h, int pad_w, void* stream) {
    const int rc = conv3x3_mish_check(x, weight, bias, out, B, H, W, C, pad_h, pad_w, 4, "weight");
    return rc != QPWC_OK ? rc : conv3x3_mish_launch(x, weight, bias, out, B, H, W, C, pad_h, pad_w, (hipStream_t)stream);
}

int qpwc_conv3x3_mish_x3_fwd(const void* x, const void* weight3, const void* bias, void* out, int B, int H,
                             int W, int C, int pad_h, int pad_w, void* stream) {
    const int rc = conv3x3_mish_check(x, weight3, bias, out, B, H, W, C, pad_h, pad_w, 4, "weight3");
    return rc != QPWC_OK ? rc
                         : conv3x3_mish_x3_launch(x, weight3, bias, out, B, H, W, C, pad_h, pad_w, (hipStream_t)stream);
}

int qpwc_conv3x3_mish_f16_fwd(const void* x, const void* weight, const void* bias, void* out, int B, int H,
                              int W, int C, int pad_h, int pad_w, void* stream) {
    const int rc = conv3x3_mish_check(x, weight, bias, out, B, H, W, C, pad_h, pad_w, 2, "weight");
    return rc != QPWC_OK ? rc
                         : conv3x3_mish_f16_launch(x, weight, bias, out, B, H, W, C, pad_h, pad_w, (hipStream_t)stream);
}

static int conv_same_check_shape(int B, int H, int W, int C_in, int C_out, int stride) {
    if (B <= 0 || H <= 0 || W <= 0) return fail(QPWC_E_SHAPE, "non-positive extent B=%d H=%d W=%d", B, H, W);
    if (C_in != 3 && C_in != 16 && C_in != 32 && C_in != 64 && C_in != 128 && C_in != 256)
        return fail(QPWC_E_SHAPE, "C_in=%d not in {3,16,32,64,128,256}", C_in);
    if (C_out != 16 && C_out != 32 && C_out != 64 && C_out != 128 && C_out != 256)
        return fail(QPWC_E_SHAPE, "C_out=%d not in {16,32,64,128,256}", C_out);
    if (stride != 1 && stride != 2) return fail(QPWC_E_SHAPE, "stride=%d not in {1,2}", stride);
    if (!conv3x3_same_shape_ok(B, H, W, C_in, C_out, stride))
        return fail(QPWC_E_SHAPE, "B=%d H=%d W=%d: too large for the launch grids", B, H, W);
    return QPWC_OK;
}

int qpwc_conv3x3_same_fwd(const void* x, const void* weight, const void* bias, void* out, int B, int H, int W,
                          int C_in, int C_out, int stride, int mish, void* stream) {
    int rc = check_nonnull({{x, "x"}, {weight, "weight"}, {bias, "bias"}, {out, "out"}});
    if (rc != QPWC_OK) return rc;
    if ((rc = conv_same_check_shape(B, H, W, C_in, C_out, stride)) != QPWC_OK) return rc;
    if (mish != 0 && mish != 1) return fail(QPWC_E_SHAPE, "mish=%d not in {0,1}", mish);
    const size_t Ho = (size_t)(H + stride - 1) / stride, Wo = (size_t)(W + stride - 1) / stride;
    const size_t cp = (size_t)(C_in + 3) / 4 * 4;
    BufCheck bufs[4];
    int n_in = 0;
    bufs[n_in++] = {x, (size_t)B * H * W * C_in * 4, (size_t)(C_in % 4 ? 4 : 16), "x"};
    bufs[n_in++] = {weight, 9 * (size_t)C_out * cp * 4, 16, "weight"};
    bufs[n_in++] = {bias, (size_t)C_out * 4, 4, "bias"};
    int n_all = n_in;
    bufs[n_all++] = {out, (size_t)B * Ho * Wo * C_out * 4, 16, "out"};
    if ((rc = check_bufs(bufs, n_in, n_all)) != QPWC_OK) return rc;
    return conv3x3_same_fwd_launch(x, weight, bias, out, B, H, W, C_in, C_out, stride, mish, (hipStream_t)stream);
}

int64_t qpwc_conv3x3_same_bwd_workspace_floats(int B, int H, int W, int C_in, int C_out, int stride) {
    const int rc = conv_same_check_shape(B, H, W, C_in, C_out, stride);
    return rc != QPWC_OK ? rc : conv3x3_same_bwd_workspace_floats(B, H, W, C_in, C_out, stride);
}

int qpwc_conv3x3_same_bwd(const void* x, const void* weight, const void* bias, const void* grad_out, void* grad_x,
                          void* grad_w, void* grad_b, void* workspace, int B, int H, int W, int C_in, int C_out,
                          int stride, int mish, void* stream) {
    int rc = check_nonnull({{x, "x"}, {weight, "weight"}, {bias, "bias"}, {grad_out, "grad_out"},
                            {workspace, "workspace"}});
    if (rc != QPWC_OK) return rc;
    if (!grad_x && !grad_w && !grad_b) return fail(QPWC_E_NULL, "grad_x, grad_w and grad_b are all null");
    if ((rc = conv_same_check_shape(B, H, W, C_in, C_out, stride)) != QPWC_OK) return rc;
    if (mish != 0 && mish != 1) return fail(QPWC_E_SHAPE, "mish=%d not in {0,1}", mish);
    const size_t Ho = (size_t)(H + stride - 1) / stride, Wo = (size_t)(W + stride - 1) / stride;
    const size_t cp = (size_t)(C_in + 3) / 4 * 4, xa = C_in % 4 ? 4 : 16;
    BufCheck bufs[8];
    int n_in = 0;
    bufs[n_in++] = {x, (size_t)B * H * W * C_in * 4, xa, "x"};
    bufs[n_in++] = {weight, 9 * (size_t)C_out * cp * 4, 16, "weight"};
    bufs[n_in++] = {bias, (size_t)C_out * 4, 4, "bias"};
    bufs[n_in++] = {grad_out, (size_t)B * Ho * Wo * C_out * 4, 16, "grad_out"};
    int n_all = n_in;
    if (grad_x) bufs[n_all++] = {grad_x, (size_t)B * H * W * C_in * 4, xa, "grad_x"};
    if (grad_w) bufs[n_all++] = {grad_w, 9 * (size_t)C_out * cp * 4, 16, "grad_w"};
    if (grad_b) bufs[n_all++] = {grad_b, (size_t)C_out * 4, 4, "grad_b"};
    bufs[n_all++] = {workspace, (size_t)conv3x3_same_bwd_workspace_floats(B, H, W, C_in, C_out, stride) * 4, 16,
                     "workspace"};
    if ((rc = check_bufs(bufs, n_in, n_all)) != QPWC_OK) return rc;
    return conv3x3_same_bwd_launch(x, weight, bias, grad_out, grad_x, grad_w, grad_b, workspace, B, H, W, C_in, C_out,
                                   stride, mish, (hipStream_t)stream);
}

static int upconv_bwd_check_shape(int B, int H, int W, int C, int F) {
    if (B <= 0 || H <= 0 || W <= 0) return fail(QPWC_E_SHAPE, "non-positive extent B=%d H=%d W=%d", B, H, W);
    if (C != 64 && C != 128 && C != 256) return fail(QPWC_E_SHAPE, "C=%d not in {64,128,256}", C);
    if (F != 16 && F != 32 && F != 64 && F != 128) return fail(QPWC_E_SHAPE, "F=%d not in {16,32,64,128}", F);
    if (!upconv4x4s2_bwd_shape_ok(B, H, W, C, F))
        return fail(QPWC_E_SHAPE, "B=%d H=%d W=%d: too large for the launch grids", B, H, W);
    return QPWC_OK;
}

int64_t qpwc_upconv4x4s2_bwd_workspace_floats(int B, int H, int W, int C, int F) {
    const int rc = upconv_bwd_check_shape(B, H, W, C, F);
    return rc != QPWC_OK ? rc : upconv4x4s2_bwd_workspace_floats(B, H, W, C, F);
}

int qpwc_upconv4x4s2_bwd(const void* x, const void* weight, const void* bias, const void* grad_out,
                         int64_t grad_out_pixel_stride, void* grad_x, void* grad_w, void* grad_b, void* workspace,
                         int B, int H, int W, int C, int F, int mish, void* stream) {
    int rc = check_nonnull({{x, "x"}, {weight, "weight"}, {bias, "bias"}, {grad_out, "grad_out"},
                            {workspace, "workspace"}});
    if (rc != QPWC_OK) return rc;
    if (!grad_x && !grad_w && !grad_b) return fail(QPWC_E_NULL, "grad_x, grad_w and grad_b are all null");
    if ((rc = upconv_bwd_check_shape(B, H, W, C, F)) != QPWC_OK) return rc;
    if (mish != 0 && mish != 1) return fail(QPWC_E_SHAPE, "mish=%d not in {0,1}", mish);
    if (grad_out_pixel_stride < F || grad_out_pixel_stride % 4 || grad_out_pixel_stride > ((int64_t)1 << 24))
        return fail(QPWC_E_SHAPE, "grad_out_pixel_stride=%lld must be a multiple of 4 in [F=%d, 2^24]", (long long)grad_out_pixel_stride,
                    F);
    const size_t px = (size_t)B * H * W;
    BufCheck bufs[8];
    int n_in = 0;
    bufs[n_in++] = {x, px * C * 4, 16, "x"};
    bufs[n_in++] = {weight, 16 * (size_t)F * C * 4, 16, "weight"};
    bufs[n_in++] = {bias, (size_t)F * 4, 4, "bias"};
    bufs[n_in++] = {grad_out, ((4 * px - 1) * (size_t)grad_out_pixel_stride + F) * 4, 16, "grad_out"};
    int n_all = n_in;
    if (grad_x) bufs[n_all++] = {grad_x, px * C * 4, 16, "grad_x"};
    if (grad_w) bufs[n_all++] = {grad_w, 16 * (size_t)F * C * 4, 16, "grad_w"};
    if (grad_b) bufs[n_all++] = {grad_b, (size_t)F * 4, 4, "grad_b"};
    bufs[n_all++] = {workspace, (size_t)upconv4x4s2_bwd_workspace_floats(B, H, W, C, F) * 4, 16, "workspace"};
    if ((rc = check_bufs(bufs, n_in, n_all)) != QPWC_OK) return rc;
    return upconv4x4s2_bwd_launch(x, weight, bias, grad_out, grad_out_pixel_stride, grad_x, grad_w, grad_b, workspace, B,
                                  H, W, C, F, mish, (hipStream_t)stream);
}

int qpwc_split_bf16x3_fwd(const void* src, void* out, long long n, void* stream) {
    if (!src || !out) return fail(QPWC_E_NULL, "null pointer argument");
    if (n <= 0 || n > ((long long)1 << 40)) return fail(QPWC_E_SHAPE, "n=%lld out of range", n);
    if ((uintptr_t)src % 4 || (uintptr_t)out % 2) return fail(QPWC_E_ALIGN, "src must be 4-byte, out 2-byte aligned");
    if (overlaps(out, (size_t)n * 6, src, (size_t)n * 4)) return fail(QPWC_E_ALIAS, "out overlaps src");
    return split_bf16x3_launch(src, out, (int64_t)n, (hipStream_t)stream);
}

// pairs are read two elements, out is written four elements at a time
static int first_conv_mish_checked(const void* pairs, const void* weight, const void* bias, void* out, int B, int H,
                                   int W, int layout, int dtype, void* stream) {
    if (!pairs || !weight || !bias || !out) return fail(QPWC_E_NULL, "null pointer argument");
    if (layout != QPWC_NHWC && layout != QPWC_NCHW) return fail(QPWC_E_LAYOUT, "Unsupported data format : %d", layout);
    if (B <= 0 || H < 2 || W < 2 || (H & 1) || (W & 1))
        return fail(QPWC_E_SHAPE, "B=%d H=%d W=%d: H and W must be even and >= 2", B, H, W);
    const size_t es = esize(dtype);
    if ((uintptr_t)pairs % (2 * es) || (uintptr_t)weight % 4 || (uintptr_t)bias % 16 || (uintptr_t)out % (4 * es))
        return fail(QPWC_E_ALIGN, dtype == QPWC_F32 ? "pairs must be 8-byte, bias and out 16-byte aligned"
                                                    : "pairs must be 4-byte, bias 16-byte and out 8-byte aligned");
    if (overlaps(out, (size_t)2 * B * (H / 2) * (W / 2) * 16 * es, pairs, (size_t)B * H * W * 6 * es))
        return fail(QPWC_E_ALIAS, "out overlaps pairs");
    return first_conv_mish_launch(pairs, weight, bias, out, B, H, W, layout, dtype, (hipStream_t)stream);
}

int qpwc_first_conv_mish_fwd(const void* pairs, const void* weight, const void* bias, void* out, int B,
                             int H, int W, int layout, void* stream) {
    return first_conv_mish_checked(pairs, weight, bias, out, B, H, W, layout, QPWC_F32, stream);
}

int qpwc_first_conv_mish_f16_fwd(const void* pairs, const void* weight, const void* bias, void* out, int B,
                                 int H, int W, int layout, void* stream) {
    return first_conv_mish_checked(pairs, weight, bias, out, B, H, W, layout, QPWC_F16, stream);
}

// C_in a power of two in [c_min, 128]: c_min 16, or 32 for the bf16x3 form
static int conv3x3s2_mish_check(const void* x_padded, const void* weight, const void* bias, const void* out, int B,
                                int H, int W, int C_in, int c_min, size_t es, const char* w_name) {
    if (!x_padded || !weight || !bias || !out) return fail(QPWC_E_NULL, "null pointer argument");
    if ((C_in != 16 && C_in != 32 && C_in != 64 && C_in != 128) || C_in < c_min)
        return fail(QPWC_E_SHAPE, "C_in=%d not in {%s32,64,128}", C_in, c_min == 16 ? "16," : "");
    if (B <= 0 || H < 2 || W < 2 || (H & 1) || (W & 1))
        return fail(QPWC_E_SHAPE, "B=%d H=%d W=%d: H and W must be even and >= 2", B, H, W);
    if ((uintptr_t)x_padded % 16 || (uintptr_t)weight % 16 || (uintptr_t)bias % 16 || (uintptr_t)out % 16)
        return fail(QPWC_E_ALIGN, "x, %s, bias, out must be 16-byte aligned", w_name);
    if (overlaps(out, (size_t)B * (H / 2) * (W / 2) * 2 * C_in * es, x_padded,
                 (size_t)B * (H + 1) * (W + 1) * C_in * es))
        return fail(QPWC_E_ALIAS, "out overlaps x");
    return QPWC_OK;
}

int qpwc_conv3x3s2_mish_fwd(const void* x_padded, const void* weight, const void* bias, void* out, int B,
                            int H, int W, void* stream) {
    const int rc = conv3x3s2_mish_check(x_padded, weight, bias, out, B, H, W, 16, 16, 4, "weight");
    return rc != QPWC_OK ? rc : conv3x3s2_mish_launch(x_padded, weight, bias, out, B, H, W, (hipStream_t)stream);
}

int qpwc_conv3x3s2_mish_c_fwd(const void* x_padded, const void* weight, const void* bias, void* out, int B,
                              int H, int W, int C_in, void* stream) {
    const int rc = conv3x3s2_mish_check(x_padded, weight, bias, out, B, H, W, C_in, 16, 4, "weight");
    return rc != QPWC_OK ? rc
                         : conv3x3s2_mish_any_launch(x_padded, weight, bias, out, B, H, W, C_in, (hipStream_t)stream);
}

int qpwc_conv3x3s2_mish_x3_fwd(const void* x_padded, const void* weight3, const void* bias, void* out, int B,
                               int H, int W, int C_in, void* stream) {
    const int rc = conv3x3s2_mish_check(x_padded, weight3, bias, out, B, H, W, C_in, 32, 4, "weight3");
    return rc != QPWC_OK ? rc
                         : conv3x3s2_mish_x3_launch(x_padded, weight3, bias, out, B, H, W, C_in, (hipStream_t)stream);
}

int qpwc_conv3x3s2_mish_f16_fwd(const void* x_padded, const void* weight, const void* bias, void* out, int B,
                                int H, int W, int C_in, void* stream) {
    const int rc = conv3x3s2_mish_check(x_padded, weight, bias, out, B, H, W, C_in, 16, 2, "weight");
    return rc != QPWC_OK ? rc
                         : conv3x3s2_mish_f16_launch(x_padded, weight, bias, out, B, H, W, C_in, (hipStream_t)stream);
}

// UpConv, alone (skip == nullptr, cat == false) or with the skip half of concat([up, skip]) in the same launch
// (include/qpwc.h): with a skip the pixel holds 2 F channels, and skip is checked like out
static int upconv_check(const void* x, const void* weight, const void* bias, const void* skip, bool cat, int64_t skip_bs,
                        int64_t skip_rs, int64_t skip_ps, const void* out, int B, int H, int W, int C, int F,
                        int64_t out_pixel_stride, size_t es, const char* w_name) {
    if (!x || !weight || !bias || !out || (cat && !skip)) return fail(QPWC_E_NULL, "null pointer argument");
    if (C != 64 && C != 128 && C != 256) return fail(QPWC_E_SHAPE, "C=%d not in {64,128,256}", C);
    if (F <= 0 || F % 16) return fail(QPWC_E_SHAPE, "F=%d must be a positive multiple of 16", F);
    if (B <= 0 || H <= 0 || W <= 0) return fail(QPWC_E_SHAPE, "non-positive extent B=%d H=%d W=%d", B, H, W);
    if (out_pixel_stride < (cat ? 2 : 1) * (int64_t)F || out_pixel_stride % 4 || out_pixel_stride > (1 << 20))
        return fail(QPWC_E_STRIDE, "out_pixel_stride %lld must be >= %s and a multiple of 4", (long long)out_pixel_stride,
                    cat ? "2 F" : "F");
    if (cat && (skip_ps < F || skip_ps % 4 || skip_rs % 4 || skip_bs % 4 || skip_rs < 2 * (int64_t)W * skip_ps ||
                skip_bs < 2 * (int64_t)H * skip_rs))
        return fail(QPWC_E_STRIDE, "skip strides (%lld, %lld, %lld) must describe (B, 2H, 2W, >= F) in multiples of 4 elements",
                    (long long)skip_bs, (long long)skip_rs, (long long)skip_ps);
    const int oa = es == 4 ? 16 : 8;
    if ((uintptr_t)x % 16 || (uintptr_t)weight % 16 || (uintptr_t)bias % 16 || (uintptr_t)out % oa ||
        (cat && (uintptr_t)skip % oa)) {
        if (cat) return fail(QPWC_E_ALIGN, "x, weight, bias must be 16-byte aligned, out and skip %d-byte", oa);
        if (es == 2) return fail(QPWC_E_ALIGN, "x, weight, bias must be 16-byte aligned, out 8-byte");
        return fail(QPWC_E_ALIGN, "x, %s, bias, out must be 16-byte aligned", w_name);
    }
    const size_t out_bytes = (size_t)B * 4 * H * W * out_pixel_stride * es;
    if (overlaps(out, out_bytes, x, (size_t)B * H * W * C * es)) return fail(QPWC_E_ALIAS, "out overlaps x");
    if (cat && overlaps(out, out_bytes, skip, (size_t)B * skip_bs * es)) return fail(QPWC_E_ALIAS, "out overlaps skip");
    return QPWC_OK;
}

int qpwc_upconv4x4s2_mish_fwd(const void* x, const void* weight, const void* bias, void* out, int B, int H, int W,
                              int C, int F, int64_t out_pixel_stride, void* stream) {
    const int rc = upconv_check(x, weight, bias, nullptr, false, 0, 0, 0, out, B, H, W, C, F, out_pixel_stride, 4, "weight");
    return rc != QPWC_OK ? rc
                         : upconv4x4s2_mish_launch(x, weight, bias, out, B, H, W, C, F, (int)out_pixel_stride,
                                                   (hipStream_t)stream);
}

int qpwc_upconv4x4s2_mish_x3_fwd(const void* x, const void* weight3, const void* bias, void* out, int B, int H, int W,
                                 int C, int F, int64_t out_pixel_stride, void* stream) {
    const int rc = upconv_check(x, weight3, bias, nullptr, false, 0, 0, 0, out, B, H, W, C, F, out_pixel_stride, 4, "weight3");
    return rc != QPWC_OK ? rc
                         : upconv4x4s2_mish_x3_launch(x, weight3, bias, out, B, H, W, C, F, (int)out_pixel_stride,
                                                      (hipStream_t)stream);
}

int qpwc_upconv4x4s2_mish_f16_fwd(const void* x, const void* weight, const void* bias, void* out, int B, int H, int W,
                                  int C, int F, int64_t out_pixel_stride, void* stream) {
    const int rc = upconv_check(x, weight, bias, nullptr, false, 0, 0, 0, out, B, H, W, C, F, out_pixel_stride, 2, "weight");
    return rc != QPWC_OK ? rc
                         : upconv4x4s2_mish_f16_launch(x, weight, bias, out, B, H, W, C, F, (int)out_pixel_stride,
                                                       (hipStream_t)stream);
}

int qpwc_upconv4x4s2_mish_cat_fwd(const void* x, const void* weight, const void* bias, const void* skip,
                                  int64_t skip_batch_stride, int64_t skip_row_stride, int64_t skip_pixel_stride, void* out,
                                  int B, int H, int W, int C, int F, int64_t out_pixel_stride, void* stream) {
    const int rc = upconv_check(x, weight, bias, skip, true, skip_batch_stride, skip_row_stride, skip_pixel_stride, out, B,
                                H, W, C, F, out_pixel_stride, 4, "weight");
    return rc != QPWC_OK ? rc
                         : upconv4x4s2_mish_launch(x, weight, bias, out, B, H, W, C, F, (int)out_pixel_stride,
                                                   (hipStream_t)stream, skip, skip_batch_stride, skip_row_stride,
                                                   skip_pixel_stride);
}

int qpwc_upconv4x4s2_mish_cat_f16_fwd(const void* x, const void* weight, const void* bias, const void* skip,
                                      int64_t skip_batch_stride, int64_t skip_row_stride, int64_t skip_pixel_stride, void* out,
                                      int B, int H, int W, int C, int F, int64_t out_pixel_stride, void* stream) {
    const int rc = upconv_check(x, weight, bias, skip, true, skip_batch_stride, skip_row_stride, skip_pixel_stride, out, B,
                                H, W, C, F, out_pixel_stride, 2, "weight");
    return rc != QPWC_OK ? rc
                         : upconv4x4s2_mish_f16_launch(x, weight, bias, out, B, H, W, C, F, (int)out_pixel_stride,
                                                       (hipStream_t)stream, skip, skip_batch_stride, skip_row_stride,
                                                       skip_pixel_stride);
}

int qpwc_image_head_fwd(const void* z, const void* w2, const void* b2, void* out, int64_t M, void* stream) {
    int rc = check_nonnull({{z, "z"}, {w2, "w2"}, {b2, "b2"}, {out, "out"}});
    if (rc != QPWC_OK) return rc;
    if ((rc = image_head_check_m(M)) != QPWC_OK) return rc;
    const BufCheck bufs[4] = {{z, (size_t)M * 256, 16, "z"}, {w2, 768, 16, "w2"}, {b2, 12, 4, "b2"},
                              {out, (size_t)M * 12, 4, "out"}};
    if ((rc = check_bufs(bufs, 3, 4)) != QPWC_OK) return rc;
    return image_head_fwd_launch(z, w2, b2, out, M, (hipStream_t)stream);
}

int64_t qpwc_image_head_bwd_workspace_floats(int64_t M) {
    const int rc = image_head_check_m(M);
    return rc != QPWC_OK ? rc : image_head_bwd_workspace_floats(M);
}

int qpwc_image_head_bwd(const void* z, const void* w2, const void* grad_out, void* grad_z, void* grad_w2,
                        void* grad_b2, void* workspace, int64_t M, void* stream) {
    int rc = check_nonnull({{z, "z"}, {w2, "w2"}, {grad_out, "grad_out"}, {workspace, "workspace"}});
    if (rc != QPWC_OK) return rc;
    if (!grad_z && !grad_w2 && !grad_b2) return fail(QPWC_E_NULL, "grad_z, grad_w2 and grad_b2 are all null");
    if ((rc = image_head_check_m(M)) != QPWC_OK) return rc;
    BufCheck bufs[7];
    int n_in = 0;
    bufs[n_in++] = {z, (size_t)M * 256, 16, "z"};
    bufs[n_in++] = {w2, 768, 16, "w2"};
    bufs[n_in++] = {grad_out, (size_t)M * 12, 4, "grad_out"};
    int n_all = n_in;
    if (grad_z) bufs[n_all++] = {grad_z, (size_t)M * 256, 16, "grad_z"};
    if (grad_w2) bufs[n_all++] = {grad_w2, 768, 4, "grad_w2"};
    if (grad_b2) bufs[n_all++] = {grad_b2, 12, 4, "grad_b2"};
    bufs[n_all++] = {workspace, (size_t)image_head_bwd_workspace_floats(M) * 4, 16, "workspace"};
    if ((rc = check_bufs(bufs, n_in, n_all)) != QPWC_OK) return rc;
    return image_head_bwd_launch(z, w2, grad_out, grad_z, grad_w2, grad_b2, workspace, M, (hipStream_t)stream);
}

int qpwc_upsample2x_image_fwd(const void* in, void* out, int B, int h, int w, int C, float scale, void* stream) {
    int rc = check_nonnull({{in, "in"}, {out, "out"}});
    if (rc != QPWC_OK) return rc;
    if ((rc = upsample2x_image_check_shape(B, h, w, C)) != QPWC_OK) return rc;
    const size_t n = (size_t)B * h * w * C * 4;
    const BufCheck bufs[2] = {{in, n, 4, "in"}, {out, 4 * n, (size_t)(C == 4 ? 16 : C == 2 ? 8 : 4), "out"}};
    if ((rc = check_bufs(bufs, 1, 2)) != QPWC_OK) return rc;
    return upsample2x_image_launch(in, out, B, h, w, C, scale, (hipStream_t)stream);
}

int qpwc_upsample2x_image_bwd(const void* grad_out, void* grad_in, int B, int h, int w, int C, float scale,
                              void* stream) {
    int rc = check_nonnull({{grad_out, "grad_out"}, {grad_in, "grad_in"}});
    if (rc != QPWC_OK) return rc;
    if ((rc = upsample2x_image_check_shape(B, h, w, C)) != QPWC_OK) return rc;
    const size_t n = (size_t)B * h * w * C * 4;
    const BufCheck bufs[2] = {{grad_out, 4 * n, 4, "grad_out"}, {grad_in, n, 4, "grad_in"}};
    if ((rc = check_bufs(bufs, 1, 2)) != QPWC_OK) return rc;
    return upsample2x_image_bwd_launch(grad_out, grad_in, B, h, w, C, scale, (hipStream_t)stream);
}

int qpwc_avgpool_pyramid_fwd(const void* x, void* out, int B, int H, int W, int C, int levels, void* stream) {
    int rc = check_nonnull({{x, "x"}, {out, "out"}});
    if (rc != QPWC_OK) return rc;
    if (B <= 0 || H <= 0 || W <= 0) return fail(QPWC_E_SHAPE, "non-positive extent B=%d H=%d W=%d", B, H, W);
    if (C < 1 || C > 4) return fail(QPWC_E_SHAPE, "C=%d outside 1..4", C);
    if (levels < 1 || levels > avgpool_pyramid_max_levels())
        return fail(QPWC_E_SHAPE, "levels=%d outside 1..%d", levels, avgpool_pyramid_max_levels());
    const int S = 1 << levels;
    if (H % S || W % S) return fail(QPWC_E_SHAPE, "H=%d W=%d are not multiples of 2^levels = %d", H, W, S);
    if (avgpool_pyramid_tiles(B, H, W, levels, nullptr) > INT32_MAX)
        return fail(QPWC_E_SHAPE, "B=%d H=%d W=%d levels=%d: the launch grid overflows 32 bits", B, H, W, levels);
    const size_t n = (size_t)B * H * W * C * 4;
    const BufCheck bufs[2] = {{x, n, 8, "x"}, {out, n >> (2 * levels), 4, "out"}};
    if ((rc = check_bufs(bufs, 1, 2)) != QPWC_OK) return rc;
    return avgpool_pyramid_launch(x, out, B, H, W, C, levels, (hipStream_t)stream);
}

const char* qpwc_agc_adam_step_kernel(int64_t n_units) {
    if (n_units < 1 || n_units > agc_adam_max_units()) return "";
    return agc_adam_step_kernel(n_units);
}

int qpwc_agc_adam_step(const void* tensors, int n_tensors, const void* units, int64_t n_units, float alpha, float beta1,
                       float beta2, float epsilon, float clip_factor, float agc_eps, void* stream) {
    int rc = check_nonnull({{tensors, "tensors"}, {units, "units"}});
    if (rc != QPWC_OK) return rc;
    if (n_tensors < 1) return fail(QPWC_E_SHAPE, "n_tensors=%d < 1", n_tensors);
    if (n_units < 1 || n_units > agc_adam_max_units())
        return fail(QPWC_E_SHAPE, "n_units=%lld outside [1, %lld]", (long long)n_units, (long long)agc_adam_max_units());
    // written so that a NaN fails each test
    if (!(beta1 >= 0.0f && beta1 < 1.0f)) return fail(QPWC_E_RANGE, "beta1=%g outside [0, 1)", beta1);
    if (!(beta2 >= 0.0f && beta2 < 1.0f)) return fail(QPWC_E_RANGE, "beta2=%g outside [0, 1)", beta2);
    if (!(epsilon > 0.0f)) return fail(QPWC_E_RANGE, "epsilon=%g must be > 0", epsilon);
    if (!(agc_eps > 0.0f)) return fail(QPWC_E_RANGE, "agc_eps=%g must be > 0", agc_eps);
    if (!(alpha - alpha == 0.0f)) return fail(QPWC_E_RANGE, "alpha=%g is not finite", alpha);
    // both tables are inputs, but one written through the other's pointers would be a caller's bug: no overlap
    const BufCheck bufs[2] = {{tensors, (size_t)n_tensors * 32, 8, "tensors"}, {units, (size_t)n_units * 24, 8, "units"}};
    if ((rc = check_bufs(bufs, 1, 2)) != QPWC_OK) return rc;
    return agc_adam_step_launch(tensors, n_tensors, units, n_units, alpha, beta1, beta2, epsilon, clip_factor, agc_eps,
                                (hipStream_t)stream);
}

const char* qpwc_augment_triplet_fwd_kernel(int B, int h, int w, const void* out_pair, const void* out_mid) {
    if (!out_pair || !out_mid || triplet_check_shapes(B, 1, 1, h, w) != QPWC_OK) return "";
    return augment_triplet_fwd_kernel(h, w, out_pair, out_mid);
}

int qpwc_augment_triplet_fwd(const void* a, const void* b, const void* c, int dtype, int B, int H, int W,
                             const void* iparams, const void* fparams, int h, int w, int flags, int layout,
                             void* out_pair, void* out_mid, void* stream) {
    if (flags & ~QPWC_TRIPLET_RAW) return fail(QPWC_E_MODE, "unknown triplet flags 0x%x", flags);
    int rc = check_nonnull({{a, "a"}, {b, "b"}, {c, "c"}, {iparams, "iparams"}, {fparams, "fparams"},
                            {out_pair, "out_pair"}, {out_mid, "out_mid"}});
    if (rc != QPWC_OK) return rc;
    if (dtype != QPWC_F32 && dtype != QPWC_U8) return fail(QPWC_E_DTYPE, "unsupported frame dtype %d", dtype);
    if (layout != QPWC_NHWC && layout != QPWC_NCHW) return fail(QPWC_E_LAYOUT, "Unsupported data format : %d", layout);
    if ((rc = triplet_check_shapes(B, H, W, h, w)) != QPWC_OK) return rc;
    const bool u8 = dtype == QPWC_U8;
    // a uint8 pixel is read byte by byte, an fp32 pixel dword by dword; the three frames may be one buffer
    const size_t src_n = (size_t)B * H * W * 3 * (u8 ? 1 : 4), src_al = u8 ? 1 : 4, out_px = (size_t)B * h * w;
    const BufCheck bufs[] = {
        {a, src_n, src_al, "a"},
        {b, src_n, src_al, "b"},
        {c, src_n, src_al, "c"},
        {iparams, (size_t)B * 4 * 4, 4, "iparams"},
        {fparams, (size_t)B * 16 * 4, 4, "fparams"},
        {out_pair, out_px * 6 * 4, 4, "out_pair"},
        {out_mid, out_px * 3 * 4, 4, "out_mid"},
    };
    if ((rc = check_bufs(bufs, 5, 7)) != QPWC_OK) return rc;
    return augment_triplet_fwd_launch(a, b, c, u8, B, H, W, (const int*)iparams, (const float*)fparams, h, w, flags,
                                      layout, (float*)out_pair, (float*)out_mid, (hipStream_t)stream);
}

int64_t qpwc_flow_to_image_workspace_floats(int n, int B, const int* h, const int* w) {
    if (!h || !w) return fail(QPWC_E_NULL, "null pointer argument");
    const int rc = vis_check_shapes(n, B, h, w, nullptr, nullptr);
    if (rc != QPWC_OK) return rc;
    return flow_to_image_workspace_floats(n, B, h, w);
}

const char* qpwc_flow_to_image_fwd_kernel(int n, int B, const int* oh, const int* ow, int out_dtype, int out_layout,
                                          const void* const* outs) {
    if (!oh || !ow || !outs || n < 1 || n > 8) return "";
    if (out_dtype != QPWC_F32 && out_dtype != QPWC_U8) return "";
    if (out_layout != QPWC_NHWC && out_layout != QPWC_NCHW) return "";
    for (int l = 0; l < n; ++l)
        if (!outs[l]) return "";
    // the picture's size stands in for the flow's own: only the outputs decide the store form
    if (vis_check_shapes(n, B, oh, ow, oh, ow) != QPWC_OK) return "";
    return flow_to_image_fwd_kernel(n, oh, ow, outs);
}

int qpwc_flow_to_image_fwd(const void* const* flows, const int* flow_dtype, const int* h, const int* w, int n, int B,
                           int in_layout, void* const* outs, const int* oh, const int* ow, int out_dtype,
                           int out_layout, void* ws, void* stream) {
    int rc = check_nonnull({{flows, "flows"}, {flow_dtype, "flow_dtype"}, {h, "h"}, {w, "w"}, {outs, "outs"},
                            {oh, "oh"}, {ow, "ow"}, {ws, "ws"}});
    if (rc != QPWC_OK) return rc;
    // the arrays hold n entries: read them only for an n the entry point takes (n itself fails below, as a shape)
    const int nn = n < 1 || n > 8 ? 0 : n;
    for (int l = 0; l < nn; ++l) {
        if (!flows[l]) return fail(QPWC_E_NULL, "flows[%d] is null", l);
        if (!outs[l]) return fail(QPWC_E_NULL, "outs[%d] is null", l);
    }
    for (int l = 0; l < nn; ++l)
        if (flow_dtype[l] != QPWC_F32 && flow_dtype[l] != QPWC_F16)
            return fail(QPWC_E_DTYPE, "flows[%d]: unsupported dtype %d", l, flow_dtype[l]);
    if (out_dtype != QPWC_F32 && out_dtype != QPWC_U8) return fail(QPWC_E_DTYPE, "unsupported output dtype %d", out_dtype);
    if (in_layout != QPWC_NHWC && in_layout != QPWC_NCHW)
        return fail(QPWC_E_LAYOUT, "Unsupported data format : %d", in_layout);
    if (out_layout != QPWC_NHWC && out_layout != QPWC_NCHW)
        return fail(QPWC_E_LAYOUT, "Unsupported data format : %d", out_layout);
    if ((rc = vis_check_shapes(n, B, h, w, oh, ow)) != QPWC_OK) return rc;
    const bool u8 = out_dtype == QPWC_U8;
    // the flows are only read and may be one buffer; the workspace and the outputs are written
    BufCheck bufs[2 * 8 + 1];
    int f16[8];
    for (int l = 0; l < n; ++l) {
        f16[l] = flow_dtype[l] == QPWC_F16;
        const size_t es = f16[l] ? 2 : 4;
        bufs[l] = indexed_buf(flows[l], (size_t)B * h[l] * w[l] * 2 * es, es, "flows[%d]", l);
        bufs[n + 1 + l] = indexed_buf(outs[l], (size_t)B * oh[l] * ow[l] * 3 * (u8 ? 1 : 4), u8 ? 1 : 4, "outs[%d]", l);
    }
    bufs[n] = indexed_buf(ws, (size_t)flow_to_image_workspace_floats(n, B, h, w) * 4, 4, "ws", 0);
    if ((rc = check_bufs(bufs, n, 2 * n + 1)) != QPWC_OK) return rc;
    return flow_to_image_fwd_launch(flows, f16, h, w, n, B, in_layout, outs, oh, ow, u8, out_layout, (float*)ws,
                                    (hipStream_t)stream);
}

int64_t qpwc_image_quality_workspace_floats(int B, int H, int W, int C) {
    const int rc = quality_check_shapes(B, H, W, C);
    if (rc != QPWC_OK) return rc;
    return image_quality_workspace_floats(B, H, W, C);
}

const char* qpwc_image_quality_fwd_kernel(int B, int H, int W, int C) {
    if (quality_check_shapes(B, H, W, C) != QPWC_OK) return "";
    return image_quality_fwd_kernel();
}

int qpwc_image_quality_fwd(const void* truth, int truth_dtype, const void* pred, int pred_dtype, int B, int H, int W,
                           int C, int layout, float offset_truth, float offset_pred, int flags, float max_val,
                           void* out, void* state, void* ws, void* stream) {
    int rc = check_nonnull({{truth, "truth"}, {pred, "pred"}, {out, "out"}, {ws, "ws"}});
    if (rc != QPWC_OK) return rc;
    if (truth_dtype != QPWC_F32 && truth_dtype != QPWC_F16) return fail(QPWC_E_DTYPE, "truth: unsupported dtype %d", truth_dtype);
    if (pred_dtype != QPWC_F32 && pred_dtype != QPWC_F16) return fail(QPWC_E_DTYPE, "pred: unsupported dtype %d", pred_dtype);
    if (layout != QPWC_NHWC && layout != QPWC_NCHW) return fail(QPWC_E_LAYOUT, "Unsupported data format : %d", layout);
    if ((rc = quality_check_shapes(B, H, W, C)) != QPWC_OK) return rc;
    // written so that a NaN fails each test
    if (!(max_val > 0.0f && max_val - max_val == 0.0f)) return fail(QPWC_E_RANGE, "max_val=%g must be finite and > 0", max_val);
    if (!(offset_truth - offset_truth == 0.0f)) return fail(QPWC_E_RANGE, "offset_truth=%g is not finite", offset_truth);
    if (!(offset_pred - offset_pred == 0.0f)) return fail(QPWC_E_RANGE, "offset_pred=%g is not finite", offset_pred);
    if ((flags == QPWC_QUALITY_U8 || flags == (QPWC_QUALITY_U8 | QPWC_QUALITY_CLIP)) && max_val != 255.0f)
        return fail(QPWC_E_RANGE, "QPWC_QUALITY_U8 takes max_val 255, got %g", max_val);
    if (flags < 0 || flags > 3) return fail(QPWC_E_MODE, "unknown quality flags 0x%x", flags);
    // the images are only read and may be one buffer; out, the workspace and the state are written
    const size_t n = (size_t)B * H * W * C;
    const BufCheck bufs[5] = {
        {truth, n * esize(truth_dtype), esize(truth_dtype), "truth"},
        {pred, n * esize(pred_dtype), esize(pred_dtype), "pred"},
        {out, (size_t)B * 3 * 4, 4, "out"},
        {ws, (size_t)image_quality_workspace_floats(B, H, W, C) * 4, 4, "ws"},
        {state, 4 * 8, 8, "state"},
    };
    if ((rc = check_bufs(bufs, 2, state ? 5 : 4)) != QPWC_OK) return rc;
    return image_quality_fwd_launch(truth, truth_dtype == QPWC_F16, pred, pred_dtype == QPWC_F16, B, H, W, C, layout,
                                    offset_truth, offset_pred, flags, max_val, (float*)out, (double*)state, (float*)ws,
                                    (hipStream_t)stream);
}

int64_t qpwc_flow_quality_workspace_floats(int B, int H, int W) {
    const int rc = flow_quality_check_shapes(B, H, W);
    if (rc != QPWC_OK) return rc;
    return flow_quality_workspace_floats(B, H, W);
}

const char* qpwc_flow_quality_fwd_kernel(int B, int H, int W) {
    if (flow_quality_check_shapes(B, H, W) != QPWC_OK) return "";
    return flow_quality_fwd_kernel();
}

int qpwc_flow_quality_fwd(const void* truth, const void* pred, int pred_dtype, const void* valid, const void* occluded,
                          int B, int H, int W, int layout, float out_abs, float out_rel, float t0, float t1, float t2,
                          float s0, float s1, void* out, void* state, void* ws, void* stream) {
    int rc = check_nonnull({{truth, "truth"}, {pred, "pred"}, {out, "out"}, {ws, "ws"}});
    if (rc != QPWC_OK) return rc;
    if (pred_dtype != QPWC_F32 && pred_dtype != QPWC_F16) return fail(QPWC_E_DTYPE, "pred: unsupported dtype %d", pred_dtype);
    if (layout != QPWC_NHWC && layout != QPWC_NCHW) return fail(QPWC_E_LAYOUT, "Unsupported data format : %d", layout);
    if ((rc = flow_quality_check_shapes(B, H, W)) != QPWC_OK) return rc;
    // written so that a NaN fails each test
    const struct {
        float v;
        const char* name;
    } params[7] = {{out_abs, "out_abs"}, {out_rel, "out_rel"}, {t0, "t0"}, {t1, "t1"}, {t2, "t2"}, {s0, "s0"}, {s1, "s1"}};
    for (const auto& a : params)
        if (!(a.v - a.v == 0.0f)) return fail(QPWC_E_RANGE, "%s=%g is not finite", a.name, a.v);
    if (!(out_abs > 0.0f)) return fail(QPWC_E_RANGE, "out_abs=%g must be > 0", out_abs);
    if (!(out_rel >= 0.0f)) return fail(QPWC_E_RANGE, "out_rel=%g must be >= 0", out_rel);
    if (!(t0 > 0.0f && t0 < t1 && t1 < t2)) return fail(QPWC_E_RANGE, "t0=%g t1=%g t2=%g must be 0 < t0 < t1 < t2", t0, t1, t2);
    if (!(s0 > 0.0f && s0 < s1)) return fail(QPWC_E_RANGE, "s0=%g s1=%g must be 0 < s0 < s1", s0, s1);
    // the flows and the masks are only read and may be one buffer; out, the workspace and the state are written.  A
    // (B,H,W,2) pixel is one load of both components; a (B,2,H,W) plane is read element by element.
    const size_t px = (size_t)B * H * W, es = esize(pred_dtype), pixel = layout == QPWC_NHWC ? 2 : 1;
    BufCheck bufs[7];
    int k = 0;
    bufs[k++] = indexed_buf(truth, px * 2 * 4, pixel * 4, "truth", 0);
    bufs[k++] = indexed_buf(pred, px * 2 * es, pixel * es, "pred", 0);
    if (valid) bufs[k++] = indexed_buf(valid, px, 1, "valid", 0);
    if (occluded) bufs[k++] = indexed_buf(occluded, px, 1, "occluded", 0);
    const int n_in = k;
    bufs[k++] = indexed_buf(out, (size_t)B * 12 * 4, 4, "out", 0);
    bufs[k++] = indexed_buf(ws, (size_t)flow_quality_workspace_floats(B, H, W) * 4, 4, "ws", 0);
    if (state) bufs[k++] = indexed_buf(state, 17 * 8, 8, "state", 0);
    if ((rc = check_bufs(bufs, n_in, k)) != QPWC_OK) return rc;
    return flow_quality_fwd_launch((const float*)truth, pred, pred_dtype == QPWC_F16, (const unsigned char*)valid,
                                   (const unsigned char*)occluded, B, H, W, layout, out_abs, out_rel, t0, t1, t2, s0, s1,
                                   (float*)out, (double*)state, (float*)ws, (hipStream_t)stream);
}

int64_t qpwc_masked_loss_workspace_floats(int kind, int B, int H, int W, int C, const int* h, const int* w, int n_levels) {
    const int rc = masked_loss_check_shapes(kind, B, H, W, C, h, w, n_levels);
    return rc != QPWC_OK ? rc : masked_loss_workspace_floats(n_levels);
}

const char* qpwc_masked_loss_fwd_kernel(int kind, int B, int H, int W, int C, const int* h, const int* w, int n_levels) {
    if (masked_loss_check_shapes(kind, B, H, W, C, h, w, n_levels) != QPWC_OK) return "";
    return masked_loss_fwd_kernel(kind, H, W, h, w, n_levels);
}

int qpwc_masked_loss_fwd(int kind, float p0, float p1, const void* y_true, const void* valid, int B, int H, int W, int C,
                         int layout, const void* const* y_pred, const int* h, const int* w, const int* pred_dtype,
                         int n_levels, void* out_losses, void* out_counts, void* const* dpred, void* const* gt_out,
                         void* const* valid_out, void* workspace, void* stream) {
    int rc = check_nonnull({{y_true, "y_true"}, {y_pred, "y_pred"}, {pred_dtype, "pred_dtype"}, {out_losses, "out_losses"},
                            {out_counts, "out_counts"}, {workspace, "workspace"}, {h, "h"}, {w, "w"}});
    if (rc != QPWC_OK) return rc;
    if ((rc = masked_loss_check_shapes(kind, B, H, W, C, h, w, n_levels)) != QPWC_OK) return rc;
    if (layout != QPWC_NHWC && layout != QPWC_NCHW) return fail(QPWC_E_LAYOUT, "Unsupported data format : %d", layout);
    if (kind == QPWC_LOSS_FLOW_MSE_V2 && !(p0 >= 0.0f)) return fail(QPWC_E_RANGE, "Huber delta %g < 0", (double)p0);
    for (int i = 0; i < n_levels; ++i)
        if (pred_dtype[i] != QPWC_F32 && pred_dtype[i] != QPWC_F16)
            return fail(QPWC_E_DTYPE, "level %d: unsupported prediction dtype %d", i, pred_dtype[i]);
    // y_true and the mask are read in 16-byte and 4-byte pieces and there is no element-wise form behind them: the
    // inputs first, then everything that is written
    const size_t px = (size_t)B * H * W;
    BufCheck bufs[2 + 8 + 3 + 24];
    int k = 0;
    bufs[k++] = indexed_buf(y_true, px * 2 * 4, 16, "y_true", 0);
    if (valid) bufs[k++] = indexed_buf(valid, px, 4, "valid", 0);
    for (int i = 0; i < n_levels; ++i) {
        const bool other = (gt_out && gt_out[i]) || (valid_out && valid_out[i]);
        if (!y_pred[i] && !other) return fail(QPWC_E_NULL, "null prediction at level %d", i);
        if (dpred && !dpred[i]) return fail(QPWC_E_NULL, "null dpred buffer at level %d", i);
        const size_t es = esize(pred_dtype[i]);
        if (y_pred[i]) bufs[k++] = indexed_buf(y_pred[i], (size_t)B * h[i] * w[i] * 2 * es, es, "y_pred[%d]", i);
    }
    const int n_in = k;
    bufs[k++] = indexed_buf(out_losses, (size_t)n_levels * 4, 4, "out_losses", 0);
    bufs[k++] = indexed_buf(out_counts, (size_t)n_levels * 8, 8, "out_counts", 0);
    bufs[k++] = indexed_buf(workspace, (size_t)masked_loss_workspace_floats(n_levels) * 4, 4, "workspace", 0);
    for (int i = 0; i < n_levels; ++i) {
        const size_t lp = (size_t)B * h[i] * w[i];
        if (dpred) bufs[k++] = indexed_buf(dpred[i], lp * 2 * 4, 4, "dpred[%d]", i);
        if (gt_out && gt_out[i]) bufs[k++] = indexed_buf(gt_out[i], lp * 2 * 4, 4, "gt_out[%d]", i);
        if (valid_out && valid_out[i]) bufs[k++] = indexed_buf(valid_out[i], lp, 1, "valid_out[%d]", i);
    }
    if ((rc = check_bufs(bufs, n_in, k)) != QPWC_OK) return rc;
    return masked_loss_fwd_launch(kind, p0, p1, (const float*)y_true, (const unsigned char*)valid, B, H, W, layout, y_pred,
                                  h, w, pred_dtype, n_levels, (float*)out_losses, (int64_t*)out_counts, dpred, gt_out,
                                  valid_out, (float*)workspace, (hipStream_t)stream);
}

int qpwc_masked_loss_bwd(int kind, const void* const* dpred, const void* counts, const void* grad_losses,
                         void* const* grad_pred, const int64_t* n_elems, const int* pred_dtype, int n_levels,
                         void* stream) {
    int rc = check_nonnull({{dpred, "dpred"}, {counts, "counts"}, {grad_losses, "grad_losses"}, {grad_pred, "grad_pred"},
                            {n_elems, "n_elems"}, {pred_dtype, "pred_dtype"}});
    if (rc != QPWC_OK) return rc;
    if (kind < QPWC_LOSS_FLOW_MSE_V2 || kind > QPWC_LOSS_FLOW_FINETUNE)
        return fail(QPWC_E_MODE, "loss kind %d is not one of the three flow losses", kind);
    if (n_levels < 1 || n_levels > 8) return fail(QPWC_E_SHAPE, "n_levels %d outside [1,8]", n_levels);
    BufCheck bufs[2 + 16];
    int k = 0;
    bufs[k++] = indexed_buf(counts, (size_t)n_levels * 8, 8, "counts", 0);
    bufs[k++] = indexed_buf(grad_losses, (size_t)n_levels * 4, 4, "grad_losses", 0);
    for (int i = 0; i < n_levels; ++i) {
        if (!dpred[i] || !grad_pred[i]) return fail(QPWC_E_NULL, "null buffer at level %d", i);
        if (pred_dtype[i] != QPWC_F32 && pred_dtype[i] != QPWC_F16)
            return fail(QPWC_E_DTYPE, "level %d: unsupported prediction dtype %d", i, pred_dtype[i]);
        if (n_elems[i] <= 0) return fail(QPWC_E_SHAPE, "level %d has no elements", i);
        bufs[k++] = indexed_buf(dpred[i], (size_t)n_elems[i] * 4, 16, "dpred[%d]", i);
    }
    const int n_in = k;
    for (int i = 0; i < n_levels; ++i) {
        const size_t es = esize(pred_dtype[i]);
        bufs[k++] = indexed_buf(grad_pred[i], (size_t)n_elems[i] * es, 4 * es, "grad_pred[%d]", i);
    }
    if ((rc = check_bufs(bufs, n_in, k)) != QPWC_OK) return rc;
    return masked_loss_bwd_launch(kind, dpred, (const int64_t*)counts, (const float*)grad_losses, grad_pred, n_elems,
                                  pred_dtype, n_levels, (hipStream_t)stream);
}

int64_t qpwc_unsup_loss_workspace_floats(int kind, int B, const int* h, const int* w, int n_levels) {
    if (!h || !w) return fail(QPWC_E_NULL, "null pointer argument");
    const int rc = unsup_loss_check_shapes(kind, B, h, w, n_levels);
    return rc != QPWC_OK ? rc : unsup_loss_workspace_floats(B, h, w, n_levels);
}

const char* qpwc_unsup_loss_fwd_kernel(int kind, int B, const int* h, const int* w, int n_levels) {
    if (!h || !w || unsup_loss_check_shapes(kind, B, h, w, n_levels) != QPWC_OK) return "";
    return unsup_loss_fwd_kernel(kind);
}

int qpwc_unsup_loss_fwd(int kind, float q, float eps, float smooth_weight, float edge, float smooth_eps,
                        const void* const* prv, const void* const* nxt, const void* const* flow,
                        const void* const* occluded, int B, const int* h, const int* w, const int* flow_dtype, int layout,
                        int n_levels, void* out_losses, void* out_photo, void* out_smooth, void* out_counts,
                        void* workspace, void* stream) {
    int rc = check_nonnull({{prv, "prv"}, {nxt, "nxt"}, {flow, "flow"}, {h, "h"}, {w, "w"}, {flow_dtype, "flow_dtype"},
                            {out_losses, "out_losses"}, {out_photo, "out_photo"}, {out_smooth, "out_smooth"},
                            {out_counts, "out_counts"}, {workspace, "workspace"}});
    if (rc != QPWC_OK) return rc;
    if ((rc = unsup_loss_check_shapes(kind, B, h, w, n_levels)) != QPWC_OK) return rc;
    if (layout != QPWC_NHWC && layout != QPWC_NCHW) return fail(QPWC_E_LAYOUT, "Unsupported data format : %d", layout);
    if ((rc = unsup_loss_check_range({q, eps, smooth_eps}, {edge, smooth_weight})) != QPWC_OK) return rc;
    for (int i = 0; i < n_levels; ++i)
        if (flow_dtype[i] != QPWC_F32 && flow_dtype[i] != QPWC_F16)
            return fail(QPWC_E_DTYPE, "level %d: unsupported flow dtype %d", i, flow_dtype[i]);
    BufCheck bufs[4 * 8 + 5];
    int k = 0;
    for (int i = 0; i < n_levels; ++i) {
        if (!prv[i] || !nxt[i] || !flow[i]) return fail(QPWC_E_NULL, "null frame or flow at level %d", i);
        const size_t px = (size_t)B * h[i] * w[i], es = esize(flow_dtype[i]);
        bufs[k++] = indexed_buf(prv[i], px * 3 * 4, 4, "prv[%d]", i);
        bufs[k++] = indexed_buf(nxt[i], px * 3 * 4, 4, "nxt[%d]", i);
        bufs[k++] = indexed_buf(flow[i], px * 2 * es, es, "flow[%d]", i);
        if (occluded && occluded[i]) bufs[k++] = indexed_buf(occluded[i], px, 1, "occluded[%d]", i);
    }
    const int n_in = k;
    bufs[k++] = indexed_buf(out_losses, (size_t)n_levels * 4, 4, "out_losses", 0);
    bufs[k++] = indexed_buf(out_photo, (size_t)n_levels * 4, 4, "out_photo", 0);
    bufs[k++] = indexed_buf(out_smooth, (size_t)n_levels * 4, 4, "out_smooth", 0);
    bufs[k++] = indexed_buf(out_counts, (size_t)n_levels * 8, 8, "out_counts", 0);
    bufs[k++] = indexed_buf(workspace, (size_t)unsup_loss_workspace_floats(B, h, w, n_levels) * 4, 4, "workspace", 0);
    if ((rc = check_bufs(bufs, n_in, k)) != QPWC_OK) return rc;
    return unsup_loss_fwd_launch(kind, q, eps, smooth_weight, edge, smooth_eps, prv, nxt, flow, occluded, B, h, w,
                                 flow_dtype, layout, n_levels, (float*)out_losses, (float*)out_photo, (float*)out_smooth,
                                 (int64_t*)out_counts, (float*)workspace, (hipStream_t)stream);
}

int qpwc_unsup_loss_bwd(int kind, float smooth_weight, float smooth_eps, const void* const* flow, const void* workspace,
                        const void* counts, const void* grad_losses, void* const* grad_flow, int B, const int* h,
                        const int* w, const int* flow_dtype, int layout, int n_levels, void* stream) {
    int rc = check_nonnull({{flow, "flow"}, {workspace, "workspace"}, {counts, "counts"}, {grad_losses, "grad_losses"},
                            {grad_flow, "grad_flow"}, {h, "h"}, {w, "w"}, {flow_dtype, "flow_dtype"}});
    if (rc != QPWC_OK) return rc;
    if ((rc = unsup_loss_check_shapes(kind, B, h, w, n_levels)) != QPWC_OK) return rc;
    if (layout != QPWC_NHWC && layout != QPWC_NCHW) return fail(QPWC_E_LAYOUT, "Unsupported data format : %d", layout);
    if ((rc = unsup_loss_check_range({smooth_eps}, {smooth_weight})) != QPWC_OK) return rc;
    for (int i = 0; i < n_levels; ++i)
        if (flow_dtype[i] != QPWC_F32 && flow_dtype[i] != QPWC_F16)
            return fail(QPWC_E_DTYPE, "level %d: unsupported flow dtype %d", i, flow_dtype[i]);
    BufCheck bufs[3 + 2 * 8];
    int k = 0;
    bufs[k++] = indexed_buf(workspace, (size_t)unsup_loss_workspace_floats(B, h, w, n_levels) * 4, 4, "workspace", 0);
    bufs[k++] = indexed_buf(counts, (size_t)n_levels * 8, 8, "counts", 0);
    bufs[k++] = indexed_buf(grad_losses, (size_t)n_levels * 4, 4, "grad_losses", 0);
    for (int i = 0; i < n_levels; ++i) {
        if (!flow[i] || !grad_flow[i]) return fail(QPWC_E_NULL, "null buffer at level %d", i);
        const size_t es = esize(flow_dtype[i]);
        bufs[k++] = indexed_buf(flow[i], (size_t)B * h[i] * w[i] * 2 * es, es, "flow[%d]", i);
    }
    const int n_in = k;
    for (int i = 0; i < n_levels; ++i) {
        const size_t es = esize(flow_dtype[i]);
        bufs[k++] = indexed_buf(grad_flow[i], (size_t)B * h[i] * w[i] * 2 * es, es, "grad_flow[%d]", i);
    }
    if ((rc = check_bufs(bufs, n_in, k)) != QPWC_OK) return rc;
    return unsup_loss_bwd_launch(kind, smooth_weight, smooth_eps, flow, (const float*)workspace, (const int64_t*)counts,
                                 (const float*)grad_losses, grad_flow, B, h, w, flow_dtype, layout, n_levels,
                                 (hipStream_t)stream);
}

int64_t qpwc_image_loss_workspace_floats(int B, int C, const int* h, const int* w, int n_levels) {
    if (!h || !w) return fail(QPWC_E_NULL, "null pointer argument");
    const int rc = image_loss_check_shapes(B, C, h, w, n_levels);
    return rc != QPWC_OK ? rc : image_loss_workspace_floats(B, C, h, w, n_levels);
}

const char* qpwc_image_loss_fwd_kernel(int B, int C, const int* h, const int* w, int n_levels) {
    if (!h || !w || image_loss_check_shapes(B, C, h, w, n_levels) != QPWC_OK) return "";
    return image_loss_fwd_kernel();
}

int qpwc_image_loss_fwd(float ssim_weight, float q, float eps, float max_val, float offset, const void* const* truth,
                        const void* const* pred, int B, int C, const int* h, const int* w, const int* pred_dtype,
                        int layout, int n_levels, void* out_losses, void* out_dssim, void* out_charb, void* workspace,
                        void* stream) {
    int rc = check_nonnull({{truth, "truth"}, {pred, "pred"}, {h, "h"}, {w, "w"}, {pred_dtype, "pred_dtype"},
                            {out_losses, "out_losses"}, {out_dssim, "out_dssim"}, {out_charb, "out_charb"},
                            {workspace, "workspace"}});
    if (rc != QPWC_OK) return rc;
    if ((rc = image_loss_check_shapes(B, C, h, w, n_levels)) != QPWC_OK) return rc;
    if (layout != QPWC_NHWC && layout != QPWC_NCHW) return fail(QPWC_E_LAYOUT, "Unsupported data format : %d", layout);
    if ((rc = image_loss_check_range(ssim_weight, q, eps, &max_val, offset)) != QPWC_OK) return rc;
    for (int i = 0; i < n_levels; ++i)
        if (pred_dtype[i] != QPWC_F32 && pred_dtype[i] != QPWC_F16)
            return fail(QPWC_E_DTYPE, "level %d: unsupported prediction dtype %d", i, pred_dtype[i]);
    BufCheck bufs[2 * 8 + 4];
    int k = 0;
    for (int i = 0; i < n_levels; ++i) {
        if (!truth[i] || !pred[i]) return fail(QPWC_E_NULL, "null target or prediction at level %d", i);
        const size_t ne = (size_t)B * C * h[i] * w[i], es = esize(pred_dtype[i]);
        bufs[k++] = indexed_buf(truth[i], ne * 4, 4, "truth[%d]", i);
        bufs[k++] = indexed_buf(pred[i], ne * es, es, "pred[%d]", i);
    }
    const int n_in = k;
    bufs[k++] = indexed_buf(out_losses, (size_t)n_levels * 4, 4, "out_losses", 0);
    bufs[k++] = indexed_buf(out_dssim, (size_t)n_levels * 4, 4, "out_dssim", 0);
    bufs[k++] = indexed_buf(out_charb, (size_t)n_levels * 4, 4, "out_charb", 0);
    bufs[k++] = indexed_buf(workspace, (size_t)image_loss_workspace_floats(B, C, h, w, n_levels) * 4, 4, "workspace", 0);
    if ((rc = check_bufs(bufs, n_in, k)) != QPWC_OK) return rc;
    return image_loss_fwd_launch(ssim_weight, q, eps, max_val, offset, truth, pred, B, C, h, w, pred_dtype, layout,
                                 n_levels, (float*)out_losses, (float*)out_dssim, (float*)out_charb, (float*)workspace,
                                 (hipStream_t)stream);
}

int qpwc_image_loss_bwd(float ssim_weight, float q, float eps, float offset, const void* const* truth,
                        const void* const* pred, const void* workspace, const void* grad_losses, void* const* grad_pred,
                        int B, int C, const int* h, const int* w, const int* pred_dtype, int layout, int n_levels,
                        void* stream) {
    int rc = check_nonnull({{truth, "truth"}, {pred, "pred"}, {workspace, "workspace"}, {grad_losses, "grad_losses"},
                            {grad_pred, "grad_pred"}, {h, "h"}, {w, "w"}, {pred_dtype, "pred_dtype"}});
    if (rc != QPWC_OK) return rc;
    if ((rc = image_loss_check_shapes(B, C, h, w, n_levels)) != QPWC_OK) return rc;
    if (layout != QPWC_NHWC && layout != QPWC_NCHW) return fail(QPWC_E_LAYOUT, "Unsupported data format : %d", layout);
    if ((rc = image_loss_check_range(ssim_weight, q, eps, nullptr, offset)) != QPWC_OK) return rc;
    for (int i = 0; i < n_levels; ++i)
        if (pred_dtype[i] != QPWC_F32 && pred_dtype[i] != QPWC_F16)
            return fail(QPWC_E_DTYPE, "level %d: unsupported prediction dtype %d", i, pred_dtype[i]);
    BufCheck bufs[2 + 3 * 8];
    int k = 0;
    bufs[k++] = indexed_buf(workspace, (size_t)image_loss_workspace_floats(B, C, h, w, n_levels) * 4, 4, "workspace", 0);
    bufs[k++] = indexed_buf(grad_losses, (size_t)n_levels * 4, 4, "grad_losses", 0);
    for (int i = 0; i < n_levels; ++i) {
        if (!truth[i] || !pred[i] || !grad_pred[i]) return fail(QPWC_E_NULL, "null buffer at level %d", i);
        const size_t ne = (size_t)B * C * h[i] * w[i], es = esize(pred_dtype[i]);
        bufs[k++] = indexed_buf(truth[i], ne * 4, 4, "truth[%d]", i);
        bufs[k++] = indexed_buf(pred[i], ne * es, es, "pred[%d]", i);
    }
    const int n_in = k;
    for (int i = 0; i < n_levels; ++i) {
        const size_t es = esize(pred_dtype[i]);
        bufs[k++] = indexed_buf(grad_pred[i], (size_t)B * C * h[i] * w[i] * es, es, "grad_pred[%d]", i);
    }
    if ((rc = check_bufs(bufs, n_in, k)) != QPWC_OK) return rc;
    return image_loss_bwd_launch(ssim_weight, q, eps, offset, truth, pred, (const float*)workspace,
                                 (const float*)grad_losses, grad_pred, B, C, h, w, pred_dtype, layout, n_levels,
                                 (hipStream_t)stream);
}

int64_t qpwc_review_workspace_floats(int n_flows, int B, int h, int w) {
    const int rc = review_check_shapes(n_flows, B, h, w, h, w);
    if (rc != QPWC_OK) return rc;
    return review_workspace_floats(n_flows, B, h, w);
}

const char* qpwc_review_panels_fwd_kernel(int n_flows, int B, int H, int W, int h, int w, int out_dtype, int out_layout) {
    if (out_dtype != QPWC_F32 && out_dtype != QPWC_U8) return "";
    if (out_layout != QPWC_NHWC && out_layout != QPWC_NCHW) return "";
    if (review_check_shapes(n_flows, B, H, W, h, w) != QPWC_OK) return "";
    return review_panels_fwd_kernel(n_flows, H, W, h, w);
}

int qpwc_inference_panels_fwd(const void* ims, int ims_dtype, const void* flo, const void* flo_pred, int B, int H, int W,
                              int in_layout, void* const* outs, int out_dtype, int out_layout, int grid, void* ws,
                              void* stream) {
    int rc = check_nonnull({{ims, "ims"}, {flo, "flo"}, {flo_pred, "flo_pred"}, {outs, "outs"}, {ws, "ws"}});
    if (rc != QPWC_OK) return rc;
    for (int i = 0; i < 10; ++i)
        if (!outs[i]) return fail(QPWC_E_NULL, "outs[%d] is null", i);
    const void* const imgs[1] = {ims};
    const int img_c[1] = {6};
    const void* const flows[2] = {flo, flo_pred};
    if ((rc = review_check(imgs, img_c, 1, ims_dtype, flows, 2, B, H, W, H, W, in_layout, outs, 10, -1, out_dtype,
                           out_layout, grid, ws)) != QPWC_OK)
        return rc;
    return inference_panels_launch(ims, ims_dtype == QPWC_F16, (const float*)flo, (const float*)flo_pred, B, H, W,
                                   in_layout, outs, out_dtype == QPWC_U8, out_layout, grid, (float*)ws,
                                   (hipStream_t)stream);
}

int qpwc_interpolation_panels_fwd(const void* img_pair, const void* img1, const void* pred, int img_dtype,
                                  const void* flow, int B, int H, int W, int h, int w, int in_layout, void* const* outs,
                                  int out_dtype, int out_layout, int grid, void* ws, void* stream) {
    int rc = check_nonnull({{img_pair, "img_pair"}, {img1, "img1"}, {pred, "pred"}, {flow, "flow"}, {outs, "outs"},
                            {ws, "ws"}});
    if (rc != QPWC_OK) return rc;
    for (int i = 0; i < 7; ++i)
        if (!outs[i]) return fail(QPWC_E_NULL, "outs[%d] is null", i);
    const void* const imgs[3] = {img_pair, img1, pred};
    const int img_c[3] = {6, 3, 3};
    const void* const flows[1] = {flow};
    if ((rc = review_check(imgs, img_c, 3, img_dtype, flows, 1, B, H, W, h, w, in_layout, outs, 7, 5, out_dtype,
                           out_layout, grid, ws)) != QPWC_OK)
        return rc;
    return interpolation_panels_launch(img_pair, img1, pred, img_dtype == QPWC_F16, (const float*)flow, B, H, W, h, w,
                                       in_layout, outs, out_dtype == QPWC_U8, out_layout, grid, (float*)ws,
                                       (hipStream_t)stream);
}

}  // extern "C"

// Flow evaluation metrics (include/qpwc_flow_quality.h): per-image end-point error with its matched / unmatched and
// speed splits, Fl-all, accuracy at three thresholds and the average angular error, over the valid pixels, in two launches:
//   flow_quality_tile_kernel   one workgroup per (image, chunk of kFlowQualChunk consecutive pixels): every lane walks
//                              the chunk with a stride of the workgroup, keeps the 15 sums of its pixels in registers,
//                              then wave reductions and one LDS step give the chunk's 15 partial sums.
//   flow_quality_fold_kernel   one workgroup, a wave per image: sums the image's partials in chunk order in double, writes
//                              out and adds the images' sums to the running state in image order.
// No atomics and nothing kept between calls except the state: two runs are bit-identical, and a captured graph replays
// both launches unchanged.  The kernel is a stream: 12 or 16 bytes of flow and 0..2 bytes of mask per pixel, read once;
// a (B,H,W,2) pixel is one 8-byte (fp32) or 4-byte (fp16) load, a (B,2,H,W) pixel two coalesced plane loads.  Which lane
// sums which pixel does not depend on the layout.
#include <math.h>

#include "../../include/qpwc_flow_quality.h"
#include "common.h"
#include "launch.h"

// every product and sum of include/qpwc_flow_quality.h is rounded separately
#pragma clang fp contract(off)

namespace qpwc {

constexpr int kFlowQualThreads = 256;
constexpr int kFlowQualFoldThreads = 1024;         // the fold launch: one workgroup, a wave per image
constexpr int kFlowQualChunk = 4096;               // pixels per workgroup (_hip.FLOW_QUALITY_CHUNK)
constexpr int kFlowQualSums = 15;                  // partial sums per (image, chunk)
constexpr int kFlowQualOuts = 12;                  // values per image

static_assert(kFlowQualChunk <= (1 << 24), "a chunk's counts must be exact in fp32");
static_assert(kFlowQualChunk % kFlowQualThreads == 0, "every lane walks the same number of pixels of a whole chunk");

struct FlowQualParams {
    float out_abs, out_rel, t0, t1, t2, s0, s1;
};

namespace {

__device__ __forceinline__ float fq_wave_sum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

__device__ __forceinline__ double fq_wave_sum(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

}  // namespace

// blockIdx.x = image * chunks + chunk; ws[blockIdx.x * 15 + q]: the chunk's sum of quantity q.  hw = H * W fits 32 bits,
// the offsets into the batch do not have to.
template <int LAYOUT, bool F16>
__global__ __launch_bounds__(kFlowQualThreads) void flow_quality_tile_kernel(const float* __restrict__ truth,
                                                                             const void* __restrict__ pred,
                                                                             const unsigned char* __restrict__ valid,
                                                                             const unsigned char* __restrict__ occluded,
                                                                             int hw, int chunks, FlowQualParams q,
                                                                             float* __restrict__ ws) {
    __shared__ float red[kFlowQualThreads / 64][kFlowQualSums];
    const int tid = threadIdx.x;
    const int n = blockIdx.x / chunks, chunk = blockIdx.x - n * chunks;
    const int p0 = chunk * kFlowQualChunk;                       // < hw
    const int len = hw - p0 < kFlowQualChunk ? hw - p0 : kFlowQualChunk;    // the last chunk may be partial
    const int64_t img = (int64_t)n * hw;                         // the image's first pixel in the batch

    float acc[kFlowQualSums];
#pragma unroll
    for (int i = 0; i < kFlowQualSums; ++i) acc[i] = 0.0f;

#pragma unroll 4
    for (int i = tid; i < len; i += kFlowQualThreads) {
        const int p = p0 + i;                                    // < hw
        float u, v, up, vp;
        if (LAYOUT == QPWC_NHWC) {
            const float2 t = reinterpret_cast<const float2*>(truth)[img + p];
            u = t.x;
            v = t.y;
            if (F16) {
                const float2 w = __half22float2(reinterpret_cast<const __half2*>(pred)[img + p]);
                up = w.x;
                vp = w.y;
            } else {
                const float2 w = reinterpret_cast<const float2*>(pred)[img + p];
                up = w.x;
                vp = w.y;
            }
        } else {
            const int64_t o = 2 * img + p;
            u = truth[o];
            v = truth[o + hw];
            if (F16) {
                up = __half2float(reinterpret_cast<const __half*>(pred)[o]);
                vp = __half2float(reinterpret_cast<const __half*>(pred)[o + hw]);
            } else {
                up = reinterpret_cast<const float*>(pred)[o];
                vp = reinterpret_cast<const float*>(pred)[o + hw];
            }
        }
        // NaN and +-inf fail both comparisons
        bool ok = fabsf(u) <= 1e9f && fabsf(v) <= 1e9f;
        if (valid != nullptr) ok = ok && valid[img + p] != 0;
        const bool occ = occluded != nullptr && occluded[img + p] != 0;

        const float du = u - up, dv = v - vp;
        const float sq = du * du + dv * dv;
        const float e = sqrtf(sq);
        const float m = sqrtf(u * u + v * v);
        const float c = u * vp - v * up;
        const float ang = atan2f(sqrtf(sq + c * c), (u * up + v * vp) + 1.0f) * 57.29577951308232f;

        const float one = ok ? 1.0f : 0.0f;
        const float ev = ok ? e : 0.0f;
        const bool b0 = m < q.s0, b2 = m >= q.s1;
        const bool b1 = !b0 && !b2;                              // ok pixels only: m is finite there
        acc[0] += one;
        acc[1] += ev;
        acc[2] += ok ? ang : 0.0f;
        acc[3] += (ok && e > q.out_abs && e > q.out_rel * m) ? 1.0f : 0.0f;
        acc[4] += (ok && e < q.t0) ? 1.0f : 0.0f;
        acc[5] += (ok && e < q.t1) ? 1.0f : 0.0f;
        acc[6] += (ok && e < q.t2) ? 1.0f : 0.0f;
        acc[7] += (ok && occ) ? 1.0f : 0.0f;
        acc[8] += occ ? ev : 0.0f;
        acc[9] += (ok && b0) ? 1.0f : 0.0f;
        acc[10] += b0 ? ev : 0.0f;
        acc[11] += (ok && b1) ? 1.0f : 0.0f;
        acc[12] += b1 ? ev : 0.0f;
        acc[13] += (ok && b2) ? 1.0f : 0.0f;
        acc[14] += b2 ? ev : 0.0f;
    }

    // the chunk's 15 sums: wave reductions, then the four waves in order
    const int wave = tid >> 6;
#pragma unroll
    for (int i = 0; i < kFlowQualSums; ++i) {
        const float s = fq_wave_sum(acc[i]);
        if ((tid & 63) == 0) red[wave][i] = s;
    }
    __syncthreads();
    if (tid < kFlowQualSums)
        ws[(int64_t)blockIdx.x * kFlowQualSums + tid] = ((red[0][tid] + red[1][tid]) + red[2][tid]) + red[3][tid];
}

// One workgroup; wave w of its 16 takes images w, w + 16, ...: lane l sums chunks l, l + 64, ... in double, a wave
// reduction, and lanes 0..11 write the image's values.  After every sixteen images threads 0..14 add them, one quantity
// each, to the running sums in image order.
__global__ __launch_bounds__(kFlowQualFoldThreads) void flow_quality_fold_kernel(const float* __restrict__ ws, int B,
                                                                                 int chunks, double pixels,
                                                                                 float* __restrict__ out,
                                                                                 double* __restrict__ state) {
    __shared__ double res[kFlowQualFoldThreads / 64][kFlowQualSums];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    double run = 0.0;
    if (state != nullptr && tid < kFlowQualSums) run = state[tid];
    for (int n0 = 0; n0 < B; n0 += kFlowQualFoldThreads / 64) {
        const int n = n0 + wave;
        if (n < B) {
            const float* p = ws + (int64_t)n * chunks * kFlowQualSums;
            double s[kFlowQualSums];
#pragma unroll
            for (int i = 0; i < kFlowQualSums; ++i) s[i] = 0.0;
            for (int t = lane; t < chunks; t += 64) {
                const float* pt = p + (int64_t)t * kFlowQualSums;
#pragma unroll
                for (int i = 0; i < kFlowQualSums; ++i) s[i] += (double)pt[i];
            }
#pragma unroll
            for (int i = 0; i < kFlowQualSums; ++i) s[i] = fq_wave_sum(s[i]);
            if (lane == 0) {
#pragma unroll
                for (int i = 0; i < kFlowQualSums; ++i) res[wave][i] = s[i];
            }
            // every lane holds the 15 sums: lane k forms value k
            double num = 0.0, den = 0.0;
            switch (lane) {
                case 0: num = s[1], den = s[0]; break;
                case 1: num = s[2], den = s[0]; break;
                case 2: num = s[3], den = s[0]; break;
                case 3: num = s[4], den = s[0]; break;
                case 4: num = s[5], den = s[0]; break;
                case 5: num = s[6], den = s[0]; break;
                case 6: num = s[1] - s[8], den = s[0] - s[7]; break;
                case 7: num = s[8], den = s[7]; break;
                case 8: num = s[10], den = s[9]; break;
                case 9: num = s[12], den = s[11]; break;
                case 10: num = s[14], den = s[13]; break;
                default: num = s[0], den = pixels; break;
            }
            if (lane < kFlowQualOuts) out[(int64_t)lane * B + n] = (float)(num / den);      // 0 / 0: NaN
        }
        __syncthreads();
        if (state != nullptr && tid < kFlowQualSums) {
            for (int w = 0; w < kFlowQualFoldThreads / 64 && n0 + w < B; ++w) run += res[w][tid];
        }
        __syncthreads();
    }
    if (state != nullptr) {
        if (tid < kFlowQualSums) state[tid] = run;
        if (tid == kFlowQualSums) state[15] += (double)B;
        if (tid == kFlowQualSums + 1) state[16] += (double)B * pixels;
    }
}

// ---- host side ------------------------------------------------------------------------------------------------------

static int64_t flow_qual_chunks(int H, int W) { return ((int64_t)H * W + kFlowQualChunk - 1) / kFlowQualChunk; }

// every count the launches index with fits 32 bits: B * H * W and the workgroups of the tile launch (the fold launch is
// one workgroup); for B, H, W >= 1
bool flow_quality_shape_ok(int B, int H, int W) {
    return (int64_t)B * H * W <= INT32_MAX && B * flow_qual_chunks(H, W) <= INT32_MAX;
}

int64_t flow_quality_workspace_floats(int B, int H, int W) { return B * flow_qual_chunks(H, W) * kFlowQualSums; }

const char* flow_quality_fwd_kernel() { return "flow_quality_tile_kernel"; }

int flow_quality_fwd_launch(const float* truth, const void* pred, bool f16, const unsigned char* valid,
                            const unsigned char* occluded, int B, int H, int W, int layout, float out_abs,
                            float out_rel, float t0, float t1, float t2, float s0, float s1, float* out, double* state,
                            float* ws, hipStream_t s) {
    const FlowQualParams q = {out_abs, out_rel, t0, t1, t2, s0, s1};
    const int hw = H * W, chunks = (int)flow_qual_chunks(H, W);
    const dim3 grid((unsigned)(B * chunks)), block(kFlowQualThreads);
#define QPWC_FLOW_QUAL(LAYOUT, F16)                                                                                   \
    hipLaunchKernelGGL((flow_quality_tile_kernel<LAYOUT, F16>), grid, block, 0, s, truth, pred, valid, occluded, hw,  \
                       chunks, q, ws)
    if (layout == QPWC_NHWC) {
        if (f16)
            QPWC_FLOW_QUAL(QPWC_NHWC, true);
        else
            QPWC_FLOW_QUAL(QPWC_NHWC, false);
    } else {
        if (f16)
            QPWC_FLOW_QUAL(QPWC_NCHW, true);
        else
            QPWC_FLOW_QUAL(QPWC_NCHW, false);
    }
#undef QPWC_FLOW_QUAL
    const int rc = check_launch("flow_quality_tile_kernel");
    if (rc != QPWC_OK) return rc;
    hipLaunchKernelGGL(flow_quality_fold_kernel, dim3(1), dim3(kFlowQualFoldThreads), 0, s, (const float*)ws, B, chunks,
                       (double)H * W, out, state);
    return check_launch("flow_quality_fold_kernel");
}

}  // namespace qpwc

// Trainer update step (qpwcnet/core/agc.py:39-49 adaptive_clip_grad, then tf.keras.optimizers.Adam's dense update;
// app/optical_flow/train.py:294-296), for every parameter tensor of a model in ONE launch.
//   A unit is the run of elements that shares one AGC norm (include/qpwc_optim.h): contiguous in the torch layouts.
//   One wave per unit, four waves per workgroup, a grid-stride loop over the unit table.
//   pass 1: sum p^2 and sum g^2 over the unit: per-lane partial sums in index order, then a 6-step xor butterfly, which
//           leaves the same bits in every lane.  No atomics: two runs are bit-identical.
//   pass 2: re-reads p and g (the unit was just read: at most a few KB, still in cache), scales g by the unit's clip
//           factor and applies m += (g - m)(1 - b1), v += (g^2 - v)(1 - b2), p -= alpha m / (sqrt(v) + epsilon).
// A unit whose four addresses share one 16-byte phase goes as (<= 3 scalar) + float4 + (<= 3 scalar) elements per
// array -- the 115-float pointwise rows and the 1035-float depthwise kernels have no aligned start or length -- any
// other unit as scalars.  Both tables are read from device memory; an entry that points outside the tensor table, a
// non-positive length or a null pointer skips the unit.
#include "common.h"
#include "launch.h"

// the update is rounded operation by operation, as the reference's TF kernels round it
#pragma clang fp contract(off)

namespace qpwc {

constexpr int kOptThreads = 256;
constexpr int kOptWaves = kOptThreads / 64;
constexpr int kOptMaxBlocks = 1024;      // 4 workgroups on each of the 256 CUs; more units than waves: the loop strides

struct OptTensor {                       // include/qpwc_optim.h: 4 pointers per tensor
    float* p;
    const float* g;
    float* m;
    float* v;
};
struct OptUnit {                         // include/qpwc_optim.h: 3 int64 per unit
    int64_t tensor, offset, length;
};
static_assert(sizeof(OptTensor) == 32 && sizeof(OptUnit) == 24, "table layouts of include/qpwc_optim.h");

namespace {

__device__ __forceinline__ float opt_wave_allsum(float v) {
#pragma unroll
    for (int m = 32; m > 0; m >>= 1) v += __shfl_xor(v, m, 64);
    return v;
}

struct OptStep {
    float alpha, omb1, omb2, epsilon, scale;
    __device__ __forceinline__ void operator()(float& p, float g, float& m, float& v) const {
        const float gc = g * scale;      // scale == 1 keeps g's bits
        m = m + (gc - m) * omb1;
        v = v + (gc * gc - v) * omb2;
        p = p - (m * alpha) / (sqrtf(v) + epsilon);
    }
};

}  // namespace

__global__ __launch_bounds__(kOptThreads) void agc_adam_kernel(const OptTensor* __restrict__ tensors, int n_tensors,
                                                               const OptUnit* __restrict__ units, int64_t n_units,
                                                               float alpha, float omb1, float omb2, float epsilon,
                                                               float clip_factor, float agc_eps) {
    const int lane = threadIdx.x & 63;
    const int64_t stride = (int64_t)gridDim.x * kOptWaves;
    for (int64_t u = (int64_t)blockIdx.x * kOptWaves + (threadIdx.x >> 6); u < n_units; u += stride) {
        const OptUnit un = units[u];
        if (un.tensor < 0 || un.tensor >= n_tensors || un.offset < 0 || un.length <= 0) continue;
        const OptTensor t = tensors[un.tensor];
        if (!t.g || !t.p || !t.m || !t.v) continue;          // grad is None: p, m, v keep their bits
        float* const p = t.p + un.offset;
        const float* const g = t.g + un.offset;
        float* const m = t.m + un.offset;
        float* const v = t.v + un.offset;
        const int64_t len = un.length;
        const unsigned phase = (unsigned)((uintptr_t)p & 15);
        const bool vec = (phase & 3) == 0 && ((uintptr_t)g & 15) == phase && ((uintptr_t)m & 15) == phase &&
                         ((uintptr_t)v & 15) == phase;
        // elements [0, head) and [tail, len) go as scalars, [head, tail) as n4 float4
        int64_t head = vec ? ((16 - phase) & 15) >> 2 : len;
        if (head > len) head = len;
        const int64_t n4 = (len - head) >> 2;
        const int64_t tail = head + 4 * n4;
        const float4* const g4 = reinterpret_cast<const float4*>(g + head);
        float4* const p4 = reinterpret_cast<float4*>(p + head);

        OptStep step = {alpha, omb1, omb2, epsilon, 1.0f};
        if (clip_factor > 0.0f) {
            float sp = 0.0f, sg = 0.0f;
            for (int64_t i = lane; i < head; i += 64) {
                const float a = p[i], b = g[i];
                sp += a * a;
                sg += b * b;
            }
            for (int64_t i = lane; i < n4; i += 64) {
                const float4 a = p4[i], b = g4[i];
                sp += a.x * a.x; sp += a.y * a.y; sp += a.z * a.z; sp += a.w * a.w;
                sg += b.x * b.x; sg += b.y * b.y; sg += b.z * b.z; sg += b.w * b.w;
            }
            for (int64_t i = tail + lane; i < len; i += 64) {
                const float a = p[i], b = g[i];
                sp += a * a;
                sg += b * b;
            }
            const float pn = sqrtf(opt_wave_allsum(sp)), gn = sqrtf(opt_wave_allsum(sg));
            const float mx = fmaxf(pn, agc_eps) * clip_factor;
            // tf.maximum propagates NaN and a NaN comparison selects the clipped branch: a NaN norm makes the whole
            // unit's gradient NaN (fmaxf would drop it)
            if (pn != pn || gn != gn) step.scale = __builtin_nanf("");
            else if (!(gn < mx)) step.scale = mx / fmaxf(gn, 1e-6f);
        }

        float4* const m4 = reinterpret_cast<float4*>(m + head);
        float4* const v4 = reinterpret_cast<float4*>(v + head);
        for (int64_t i = lane; i < head; i += 64) step(p[i], g[i], m[i], v[i]);
        for (int64_t i = lane; i < n4; i += 64) {
            float4 a = p4[i], c = m4[i], d = v4[i];
            const float4 b = g4[i];
            step(a.x, b.x, c.x, d.x);
            step(a.y, b.y, c.y, d.y);
            step(a.z, b.z, c.z, d.z);
            step(a.w, b.w, c.w, d.w);
            p4[i] = a;
            m4[i] = c;
            v4[i] = d;
        }
        for (int64_t i = tail + lane; i < len; i += 64) step(p[i], g[i], m[i], v[i]);
    }
}

// ---- host side ------------------------------------------------------------------------------------------------------

static int64_t opt_blocks(int64_t n_units) { return (n_units + kOptWaves - 1) / kOptWaves; }

int64_t agc_adam_max_units() { return 0x7fffffff; }

const char* agc_adam_step_kernel(int64_t n_units) {
    return opt_blocks(n_units) <= kOptMaxBlocks ? "agc_adam_kernel<one unit per wave>" : "agc_adam_kernel<grid-stride>";
}

int agc_adam_step_launch(const void* tensors, int n_tensors, const void* units, int64_t n_units, float alpha,
                         float beta1, float beta2, float epsilon, float clip_factor, float agc_eps, hipStream_t s) {
    const int64_t nblk = opt_blocks(n_units);
    const dim3 grid((unsigned)(nblk < kOptMaxBlocks ? nblk : kOptMaxBlocks)), block(kOptThreads);
    // 1 - beta in double from the fp32 betas, rounded once: what `1 - beta_t` of an fp32 variable gives in Keras
    const float omb1 = (float)(1.0 - (double)beta1), omb2 = (float)(1.0 - (double)beta2);
    hipLaunchKernelGGL(agc_adam_kernel, grid, block, 0, s, (const OptTensor*)tensors, n_tensors, (const OptUnit*)units,
                       n_units, alpha, omb1, omb2, epsilon, clip_factor, agc_eps);
    return check_launch("agc_adam_kernel");
}

}  // namespace qpwc

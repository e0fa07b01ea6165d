// Device-resident step controls (include/hesic_train_ctl.h): the global L2 norm of a flat gradient buffer with the clip coefficient and
// the non-finite guard derived from it on the device, and the Adam update that reads its learning rate, that coefficient and the
// apply / skip flag from the control block.  A training step recorded into a HIP graph runs no Python between its launches: what a host loop
// decides there (clip_grad_norm_, "is the loss finite", this epoch's rate) is decided here by kernels that read a few floats of device memory.
//
// Determinism is part of the contract: every rank of a data-parallel run computes the norm of the same all-reduced buffer and must reach
// the same coefficient and the same skip decision, and a graph replay must repeat the eager step.  So no atomics and no "last block done"
// counter: each block leaves ONE fp64 partial in a slot of its own, a second one-block launch adds the slots in a fixed order.
#include "common.h"
#include "../../include/hesic_train_ctl.h"

namespace {

constexpr int NORM_THREADS = 256, NORM_EPB = 4096;          // the grid is a function of numel alone: ceil(numel / NORM_EPB), capped

__device__ __forceinline__ double sq4(const f32x4 v) {
    const double a = (double)v[0], b = (double)v[1], c = (double)v[2], d = (double)v[3];
    return (a * a + b * b) + (c * c + d * d);
}

// Stage 1.  `head` scalar elements bring the address to a 16-byte boundary, `nvec` 16-byte loads follow, `tail` scalar elements finish.
// The products are fp64 from the start: 1e-30^2 does not vanish and 1e30^2 is not infinity, so the only way to a non-finite sum is a
// non-finite element.  HBM-bound: 4 bytes in per element against 1 conversion + 1 fp64 FMA.
__global__ __launch_bounds__(NORM_THREADS) void grad_sumsq_partials_kernel(const float* __restrict__ g, int64_t numel, int head, int64_t nvec,
                                                                           double* __restrict__ partials) {
    __shared__ double red[NORM_THREADS / 64];
    const int tid = threadIdx.x;
    const int64_t stride = (int64_t)gridDim.x * NORM_THREADS;
    const f32x4* __restrict__ gv = (const f32x4*)(g + head);
    double acc = 0.0;
    int64_t i = (int64_t)blockIdx.x * NORM_THREADS + tid;
    for (; i + 3 * stride < nvec; i += 4 * stride) {            // four independent 16-byte loads in flight per thread
        const f32x4 a = gv[i], b = gv[i + stride], c = gv[i + 2 * stride], d = gv[i + 3 * stride];
        acc += (sq4(a) + sq4(b)) + (sq4(c) + sq4(d));
    }
    for (; i < nvec; i += stride) acc += sq4(gv[i]);
    if (blockIdx.x == 0) {                                       // the unaligned ends: at most 3 + 3 elements
        const int64_t tail0 = head + 4 * nvec;
        if (tid < head) { const double x = (double)g[tid]; acc += x * x; }
        if (tail0 + tid < numel && tid < 4) { const double x = (double)g[tail0 + tid]; acc += x * x; }
    }
    acc = wave_sum_d(acc);                                       // xor butterfly: every lane ends with the same bits, the order is fixed
    if ((tid & 63) == 0) red[tid >> 6] = acc;
    __syncthreads();
    if (tid == 0) partials[blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
}

// Stage 2: one block; thread t adds partials t, t + 256, ... in that order, then the same fixed tree as above.
__global__ __launch_bounds__(NORM_THREADS) void grad_norm_decide_kernel(const double* __restrict__ partials, int n_partials, float* __restrict__ ctl,
                                                                        const float* __restrict__ also_require) {
    __shared__ double red[NORM_THREADS / 64];
    const int tid = threadIdx.x;
    double acc = 0.0;
    for (int i = tid; i < n_partials; i += NORM_THREADS) acc += partials[i];
    acc = wave_sum_d(acc);
    if ((tid & 63) == 0) red[tid >> 6] = acc;
    __syncthreads();
    if (tid != 0) return;
    const double sumsq = (red[0] + red[1]) + (red[2] + red[3]);
    const float norm = (float)sqrt(sumsq);                       // correctly rounded fp64 root, rounded once to fp32
    const float max_norm = ctl[HESIC_TRAIN_CTL_MAX_NORM];
    float coef = 1.f;
    if (max_norm > 0.f) {
        // torch.nn.utils.clip_grad_norm_: clamp(max_norm / (total_norm + 1e-6), max=1.0) in fp32 (a NaN norm stays a NaN coefficient)
        const float c = __fdiv_rn(max_norm, __fadd_rn(norm, 1e-6f));
        coef = c > 1.f ? 1.f : c;
    }
    // judged on the fp64 sum: a finite buffer whose norm exceeds the fp32 range is still a finite gradient
    const bool finite = sumsq == sumsq && sumsq <= 1.7976931348623157e308;
    bool applied = !(ctl[HESIC_TRAIN_CTL_SKIP_NONFINITE] != 0.f && !finite);
    if (also_require) applied = applied && also_require[HESIC_TRAIN_CTL_APPLIED] != 0.f;
    ctl[HESIC_TRAIN_CTL_GRAD_NORM] = norm;
    ctl[HESIC_TRAIN_CTL_CLIP_COEF] = coef;
    ctl[HESIC_TRAIN_CTL_APPLIED] = applied ? 1.f : 0.f;
    ctl[HESIC_TRAIN_CTL_SKIPPED] += applied ? 0.f : 1.f;
}

// g * coef as ONE rounded fp32 product that never fuses into the operations that consume it (this toolchain's __fmul_rn is a plain `x * y`,
// open to contraction under the default -ffp-contract=fast-honor-pragmas; the pragma is what keeps it a product of its own): the update then
// equals hesic_adam_step fed the same products from memory.
__device__ __forceinline__ float mul_rn_unfused(float a, float b) {
#pragma clang fp contract(off)
    const float r = a * b;
    return r;
}

__global__ void adam_bump_steps_ctl_kernel(const hesic_adam_chunk c, const float* __restrict__ ctl) {
    const int i = threadIdx.x;
    if (ctl[HESIC_TRAIN_CTL_APPLIED] != 0.f && i < c.n) *c.step[i] += 1.f;
}

// adam_update_kernel (glue.hip) term for term; the differences: lr and the gradient's coefficient come from the control block, and a
// cleared `applied` flag ends every block before it touches anything.
constexpr int ADAM_EPB = 4096;
__global__ __launch_bounds__(256) void adam_update_ctl_kernel(const hesic_adam_chunk c, const float* __restrict__ ctl) {
    if (ctl[HESIC_TRAIN_CTL_APPLIED] == 0.f) return;             // uniform over the grid
    const int bid = blockIdx.x;
    int t = 0;
    while (t + 1 < c.n && c.block0[t + 1] <= bid) ++t;
    __shared__ float sc[2];
    if (threadIdx.x == 0) {
        const double st = (double)*c.step[t];
        const double bc1 = 1.0 - pow((double)c.beta1, st), bc2 = 1.0 - pow((double)c.beta2, st);
        sc[0] = (float)((double)ctl[HESIC_TRAIN_CTL_LR] / bc1);
        sc[1] = (float)(1.0 / sqrt(bc2));
    }
    __syncthreads();
    const float step_size = sc[0], rbc2s = sc[1];
    const float coef = ctl[HESIC_TRAIN_CTL_CLIP_COEF];
    float* __restrict__ p = c.p[t];
    const float* __restrict__ g = c.g[t];
    float* __restrict__ m = c.m[t];
    float* __restrict__ v = c.v[t];
    const int64_t n = c.numel[t];
    const int64_t base = (int64_t)(bid - c.block0[t]) * ADAM_EPB;
    const float omb1 = 1.f - c.beta1, omb2 = 1.f - c.beta2;
    const bool vec = ((((uintptr_t)p | (uintptr_t)g | (uintptr_t)m | (uintptr_t)v) & 15) == 0) && base + ADAM_EPB <= n;
    if (vec) {
#pragma unroll
        for (int u = 0; u < ADAM_EPB / 1024; ++u) {
            const int64_t i = base + u * 1024 + threadIdx.x * 4;
            f32x4 gv = *(const f32x4*)(g + i);
            f32x4 mv = *(const f32x4*)(m + i), vv = *(const f32x4*)(v + i), pv = *(const f32x4*)(p + i);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                gv[e] = mul_rn_unfused(gv[e], coef);
                mv[e] = mv[e] + omb1 * (gv[e] - mv[e]);
                vv[e] = vv[e] * c.beta2 + omb2 * gv[e] * gv[e];
                pv[e] -= step_size * (mv[e] / (sqrtf(vv[e]) * rbc2s + c.eps));
            }
            *(f32x4*)(m + i) = mv; *(f32x4*)(v + i) = vv; *(f32x4*)(p + i) = pv;
        }
    } else {
        for (int64_t i = base + threadIdx.x; i < base + ADAM_EPB && i < n; i += 256) {
            const float gv = mul_rn_unfused(g[i], coef);
            const float mv = m[i] + omb1 * (gv - m[i]);
            const float vv = v[i] * c.beta2 + omb2 * gv * gv;
            m[i] = mv; v[i] = vv;
            p[i] -= step_size * (mv / (sqrtf(vv) * rbc2s + c.eps));
        }
    }
}

}  // namespace

extern "C" int hesic_grad_norm_ctl(const float* g, int64_t numel, double* partials, float* ctl, const float* also_require, void* stream) {
    HESIC_CHECK_ARG(g && partials && ctl && numel > 0, "grad_norm_ctl: null pointer or numel <= 0");
    HESIC_CHECK_ARG(((uintptr_t)g & 3) == 0 && ((uintptr_t)partials & 7) == 0 && ((uintptr_t)ctl & 3) == 0, "grad_norm_ctl: misaligned pointer");
    int head = (int)(((16 - ((uintptr_t)g & 15)) & 15) / 4);     // scalar elements up to the first 16-byte boundary
    if (head > numel) head = (int)numel;
    const int64_t nvec = (numel - head) / 4;
    int64_t blocks = cdiv64(numel, NORM_EPB);
    if (blocks > HESIC_GRAD_NORM_MAX_BLOCKS) blocks = HESIC_GRAD_NORM_MAX_BLOCKS;
    hipLaunchKernelGGL(grad_sumsq_partials_kernel, dim3((unsigned)blocks), dim3(NORM_THREADS), 0, (hipStream_t)stream, g, numel, head, nvec, partials);
    hipLaunchKernelGGL(grad_norm_decide_kernel, dim3(1), dim3(NORM_THREADS), 0, (hipStream_t)stream, (const double*)partials, (int)blocks, ctl,
                       also_require);
    HESIC_LAUNCH_RETURN("grad_norm_ctl");
}

extern "C" int hesic_adam_step_ctl(const hesic_adam_chunk* chunk_host, const float* ctl, void* stream) {
    HESIC_CHECK_ARG(chunk_host && ctl, "adam_step_ctl: null pointer");
    HESIC_CHECK_ARG(chunk_host->n > 0 && chunk_host->n <= HESIC_ADAM_MAX_TENSORS, "adam_step_ctl: bad chunk");
    hesic_adam_chunk c = *chunk_host;
    int blk = 0;
    for (int i = 0; i < c.n; ++i) {
        HESIC_CHECK_ARG(c.p[i] && c.g[i] && c.m[i] && c.v[i] && c.step[i] && c.numel[i] > 0, "adam_step_ctl: null tensor or numel <= 0");
        c.block0[i] = blk;
        blk += (int)((c.numel[i] + ADAM_EPB - 1) / ADAM_EPB);
    }
    c.block0[c.n] = blk;
    hipLaunchKernelGGL(adam_bump_steps_ctl_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, c, ctl);
    hipLaunchKernelGGL(adam_update_ctl_kernel, dim3((unsigned)blk), dim3(256), 0, (hipStream_t)stream, c, ctl);
    HESIC_LAUNCH_RETURN("adam_step_ctl");
}

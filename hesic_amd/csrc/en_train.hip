// The stage-2 training step's own kernels (include/hesic_en_train.h): the criterion lambda * 255^2 * (MSE(a1, b1) + MSE(a2, b2)) of both views in
// two launches, its gradient as the 32-channel NHWC map the output layer's backward reads, and the data-gradient weights of all convs of a flat
// parameter buffer in one launch.  All three move bytes and do next to no arithmetic.
//
// The sums follow pair_metrics.hip's scheme: a block writes its fp64 partial to a workspace, a second, tiny launch adds the partials in index
// order -- no atomics, no zero-fill, the same bits every time.  The images are dense planar fp32, so an image of a view is one span of 3 * H * W
// floats, read with 16-byte loads where the span starts on a 16-byte boundary in both operands and with 4-byte loads by the same lanes in the same
// order otherwise.
#include "common.h"
#include "../../include/hesic_en_train.h"

namespace {

constexpr int EN_THREADS = 256;
// 4096 elements a block (256 lanes x one 16-byte load x 4 trips), at most 64 blocks an image: the finishing wave fetches 64 partials per trip.
// 512^2: 64 blocks of 12 trips; B = 8 gives 2 x 8 x 64 = 1024 blocks, four per CU.  A choice from the guides' grid rule, measured only as a whole
// (profiles/stage2_train_bench.json).
constexpr int EN_ELEMS = 4096, EN_MAX_BLOCKS = 64;

static inline int en_blocks(int64_t per) { return grid_for(per, EN_ELEMS, EN_MAX_BLOCKS); }

__device__ __forceinline__ double sq_d(float a, float b) {
    const double d = (double)(a - b);
    return d * d;
}
__device__ __forceinline__ double sq4_d(f32x4 a, f32x4 b) { return sq_d(a.x, b.x) + sq_d(a.y, b.y) + sq_d(a.z, b.z) + sq_d(a.w, b.w); }

struct EnLoss {
    const float* a[2]; const float* b[2];
    int B, nb;                     // images, blocks per (view, image)
    int64_t per;                   // 3 * H * W
    double* ws;                    // (2, B, nb)
    double n, lambda_255sq;
};

__global__ __launch_bounds__(EN_THREADS) void en_loss_partial_kernel(const EnLoss m) {
    __shared__ double red[4];
    const int r = (int)blockIdx.x, per_view = m.B * m.nb;
    const int v = r >= per_view ? 1 : 0, q = r - v * per_view;
    const int img = q / m.nb, bid = q - img * m.nb;
    const float* __restrict__ a = m.a[v] + (int64_t)img * m.per;
    const float* __restrict__ b = m.b[v] + (int64_t)img * m.per;
    const int64_t n = m.per, n4 = n >> 2;
    const int64_t gt = bid * (int64_t)EN_THREADS + threadIdx.x, stride = (int64_t)m.nb * EN_THREADS;
    double acc = 0.0;
    if ((((uintptr_t)a | (uintptr_t)b) & 15) == 0) {
        for (int64_t i = gt; i < n4; i += stride) acc += sq4_d(((const f32x4*)a)[i], ((const f32x4*)b)[i]);
    } else {
        for (int64_t i = gt; i < n4; i += stride)
            acc += sq4_d(f32x4{a[4 * i], a[4 * i + 1], a[4 * i + 2], a[4 * i + 3]}, f32x4{b[4 * i], b[4 * i + 1], b[4 * i + 2], b[4 * i + 3]});
    }
    for (int64_t i = n4 * 4 + gt; i < n; i += stride) acc += sq_d(a[i], b[i]);
    acc = wave_sum_d(acc);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) m.ws[r] = red[0] + red[1] + red[2] + red[3];
}

// wave v adds view v's B * nb partials in index order: 64 loads in flight per trip, then a chain of additions through readlanes, starting FROM the
// first partial (not from +0)
__global__ __launch_bounds__(128) void en_loss_finish_kernel(const EnLoss m, double* __restrict__ out) {
    __shared__ double sse[2];
    const int v = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int cnt = m.B * m.nb;
    const double* p = m.ws + (int64_t)v * cnt;
    double s = 0.0;
    for (int base = 0; base < cnt; base += 64) {
        const int k = cnt - base < 64 ? cnt - base : 64;
        const double x = lane < k ? p[base + lane] : 0.0;
        int j = 0;
        if (base == 0) { s = __shfl(x, 0, 64); j = 1; }
        for (; j < k; ++j) s += __shfl(x, j, 64);
    }
    if (lane == 0) sse[v] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        const double mse = sse[0] / m.n + sse[1] / m.n;
        out[0] = sse[0]; out[1] = sse[1]; out[2] = mse; out[3] = m.lambda_255sq * mse;
    }
}

// One lane a pixel: six 4-byte loads (coalesced plane by plane), four 16-byte stores that fill the pixel's 64 bytes -- pack_images_c32's store shape.
struct EnGrad {
    const float* a[2]; const float* b[2];
    uint32_t* g[2];
    const float* seed;
    float s;
    int B;
    int64_t HW;
};

__global__ __launch_bounds__(EN_THREADS) void en_loss_grad_kernel(const EnGrad m) {
    const float s = m.seed ? m.s * m.seed[0] : m.s;
    const int64_t per_view = (int64_t)m.B * m.HW, total = 2 * per_view, HW = m.HW;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int v = i >= per_view ? 1 : 0;
        const int64_t p = i - v * per_view, img = p / HW, q = p - img * HW;
        const float* __restrict__ pa = m.a[v] + img * 3 * HW + q;
        const float* __restrict__ pb = m.b[v] + img * 3 * HW + q;
        const float g0 = s * (pa[0] - pb[0]), g1 = s * (pa[HW] - pb[HW]), g2 = s * (pa[2 * HW] - pb[2 * HW]);
        const u32x4 v0 = {pack_h2_raw(g0, g1), pack_h2_raw(g2, 0.f), 0u, 0u};
        const u32x4 z = {0u, 0u, 0u, 0u};
        u32x4* o = (u32x4*)(m.g[v] + p * 16);
        o[0] = v0; o[1] = z; o[2] = z; o[3] = z;
    }
}

constexpr int MIRROR_BLOCKS_X = 4;      // 32 x 32 x 9 = 9216 floats a layer at most: 9 trips of 4 x 256 lanes
__global__ __launch_bounds__(EN_THREADS) void c32_mirror_weights_kernel(const float* __restrict__ src, int64_t src_numel, float* __restrict__ dst,
                                                                        int64_t dst_numel, const hesic_mirror_entry* __restrict__ table) {
    const hesic_mirror_entry e = table[blockIdx.y];
    if (e.cout < 1 || e.cout > 32 || e.cin < 1 || e.cin > 32 || e.cout_pad < e.cout || e.cout_pad > 32) return;      // block-uniform
    const int n_src = e.cout * e.cin * 9, n_dst = e.cin * e.cout_pad * 9;
    if (e.src < 0 || e.dst < 0 || e.src > src_numel - n_src || e.dst > dst_numel - n_dst) return;
    const float* __restrict__ w = src + e.src;
    float* __restrict__ o = dst + e.dst;
    for (int i = blockIdx.x * EN_THREADS + threadIdx.x; i < n_dst; i += MIRROR_BLOCKS_X * EN_THREADS) {
        const int t = i % 9, r = i / 9, co = r % e.cout_pad, ci = r / e.cout_pad;
        o[i] = co < e.cout ? w[(co * e.cin + ci) * 9 + 8 - t] : 0.f;          // tap (2 - ky, 2 - kx) = 8 - (3 ky + kx)
    }
}

int en_check_dims(const char* who, int B, int H, int W) {
    HESIC_CHECK_ARG(B >= 1 && H >= 1 && W >= 1, "%s: non-positive dims B=%d H=%d W=%d", who, B, H, W);
    HESIC_CHECK_ARG(B <= (1 << 20), "%s: B = %d pairs, more than 2^20", who, B);
    HESIC_CHECK_ARG((int64_t)H * W < (1ll << 31), "%s: H * W = %lld pixels an image, 2^31 or more", who, (long long)((int64_t)H * W));
    return 0;
}

}  // namespace

extern "C" int64_t hesic_en_loss_ws_bytes(int B, int H, int W) {
    if (en_check_dims("en_loss_ws_bytes", B, H, W) != 0) return -1;
    return 2 * (int64_t)B * en_blocks(3 * (int64_t)H * W) * (int64_t)sizeof(double);
}

extern "C" int hesic_en_loss(const float* a1, const float* b1, const float* a2, const float* b2, int B, int H, int W, double lambda_255sq,
                             double* out, void* ws, int64_t ws_bytes, void* stream) {
    HESIC_CHECK_ARG(a1 && b1 && a2 && b2 && out && ws, "en_loss: null pointer");
    if (en_check_dims("en_loss", B, H, W) != 0) return HESIC_EINVAL;
    HESIC_CHECK_ARG((((uintptr_t)a1 | (uintptr_t)b1 | (uintptr_t)a2 | (uintptr_t)b2) & 3) == 0, "en_loss: an operand is not 4-byte aligned");
    HESIC_CHECK_ARG(((uintptr_t)ws & 7) == 0 && ((uintptr_t)out & 7) == 0, "en_loss: out / workspace not 8-byte aligned");
    EnLoss m;
    m.a[0] = a1; m.b[0] = b1; m.a[1] = a2; m.b[1] = b2;
    m.B = B; m.per = 3 * (int64_t)H * W; m.nb = en_blocks(m.per);
    const int64_t need = 2 * (int64_t)B * m.nb * (int64_t)sizeof(double);
    HESIC_CHECK_ARG(ws_bytes >= need, "en_loss: workspace too small (%lld bytes, %lld needed)", (long long)ws_bytes, (long long)need);
    m.ws = (double*)ws; m.n = (double)B * 3.0 * (double)H * (double)W; m.lambda_255sq = lambda_255sq;
    hipLaunchKernelGGL(en_loss_partial_kernel, dim3((unsigned)(2 * B * m.nb)), dim3(EN_THREADS), 0, (hipStream_t)stream, m);
    hipLaunchKernelGGL(en_loss_finish_kernel, dim3(1), dim3(128), 0, (hipStream_t)stream, m, out);
    HESIC_LAUNCH_RETURN("en_loss");
}

extern "C" int hesic_en_loss_grad(const float* a1, const float* b1, const float* a2, const float* b2, int B, int H, int W, double lambda_255sq,
                                  const float* seed, void* g1, void* g2, void* stream) {
    HESIC_CHECK_ARG(a1 && b1 && a2 && b2 && g1 && g2, "en_loss_grad: null pointer");
    if (en_check_dims("en_loss_grad", B, H, W) != 0) return HESIC_EINVAL;
    HESIC_CHECK_ARG((((uintptr_t)a1 | (uintptr_t)b1 | (uintptr_t)a2 | (uintptr_t)b2 | (uintptr_t)seed) & 3) == 0,
                    "en_loss_grad: an operand is not 4-byte aligned");
    HESIC_CHECK_ARG((((uintptr_t)g1 | (uintptr_t)g2) & 15) == 0, "en_loss_grad: a gradient map is not 16-byte aligned");
    EnGrad m;
    m.a[0] = a1; m.b[0] = b1; m.a[1] = a2; m.b[1] = b2; m.g[0] = (uint32_t*)g1; m.g[1] = (uint32_t*)g2;
    m.seed = seed; m.B = B; m.HW = (int64_t)H * W;
    m.s = (float)(2.0 * lambda_255sq / ((double)B * 3.0 * (double)H * (double)W));
    hipLaunchKernelGGL(en_loss_grad_kernel, dim3(grid_for(2 * (int64_t)B * m.HW, EN_THREADS)), dim3(EN_THREADS), 0, (hipStream_t)stream, m);
    HESIC_LAUNCH_RETURN("en_loss_grad");
}

extern "C" int hesic_c32_mirror_weights(const float* src, int64_t src_numel, float* dst, int64_t dst_numel, const hesic_mirror_entry* table,
                                        int n_layers, int capacity, void* stream) {
    HESIC_CHECK_ARG(src && dst && table, "c32_mirror_weights: null pointer");
    HESIC_CHECK_ARG(src_numel >= 1 && dst_numel >= 1, "c32_mirror_weights: non-positive buffer sizes %lld, %lld", (long long)src_numel,
                    (long long)dst_numel);
    HESIC_CHECK_ARG(n_layers >= 1 && n_layers <= 65535, "c32_mirror_weights: n_layers = %d outside 1..65535", n_layers);
    HESIC_CHECK_ARG(n_layers <= capacity, "c32_mirror_weights: %d layers, more than the table's capacity of %d", n_layers, capacity);
    HESIC_CHECK_ARG((((uintptr_t)src | (uintptr_t)dst) & 3) == 0 && ((uintptr_t)table & 7) == 0, "c32_mirror_weights: misaligned pointer");
    hipLaunchKernelGGL(c32_mirror_weights_kernel, dim3(MIRROR_BLOCKS_X, (unsigned)n_layers), dim3(EN_THREADS), 0, (hipStream_t)stream, src, src_numel,
                       dst, dst_numel, table);
    HESIC_LAUNCH_RETURN("c32_mirror_weights");
}

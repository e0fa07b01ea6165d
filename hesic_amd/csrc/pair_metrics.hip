// The rate-distortion sums of a batch per pair (include/hesic_pair_metrics.h): bits per likelihood map, squared error per view and the
// squared error of the 8-bit images a decoder writes, as one row of a (B, n_lik + 4) fp64 table per pair.  hesic_rd_sums (glue.hip) adds a
// whole batch into one scalar per quantity with one same-address fp64 atomic per block; here a block writes its partial to a workspace and
// a second, tiny launch adds each (image, column)'s partials in index order: no atomics, no zero-fill, the same bits every time.
//
// Per term the arithmetic is that of sum_log2_body / sum_sq_diff_body in glue.hip: log2f in fp32 widened to fp64; per pixel an fp32 fmaf
// chain over the channels (restarted every 8), widened to fp64.  The 8-bit sum comes from the same loads: q(v) = rintf(clamp(v, 0, 1) * 255)
// are integers <= 255, eight squared differences stay below 2^24, so the fp32 chain and every fp64 sum of them are exact.
//
// A job is one (likelihood map | image pair) of ONE image; its block count and the work of each of its lanes depend only on that image's
// element / pixel count, so a pair's row does not depend on the batch it is evaluated in or on its position there.  A likelihood slice that
// does not start on a 16-byte boundary (per-image count % 4 != 0, images 1, 2, ...) is read with 4-byte loads by the same lanes in the same
// order as the 16-byte form reads it.
#include "common.h"
#include "../../include/hesic_pair_metrics.h"

namespace {

constexpr int PM_THREADS = 256;
// Block counts per job -- a choice, not a measured optimum (the issue that asked for this kernel left them open):
//   likelihood map: 4096 elements a block (256 lanes x one 16-byte load x 4 trips), at most 32 blocks.  The y maps of a 512^2 image
//     (192 x 32 x 32) get 32 blocks of 6 trips; a z map (128 x 8 x 8) gets 2.
//   image pair: 1024 pixels a block (the 4-pixel unrolled trip of sum_sq_diff_body), at most 64 blocks: 512^2 gives 64 blocks of 4 trips.
// At B = 8, 512^2 that is 8 x (2 x 32 + 2 x 2 + 2 x 64) = 1568 blocks, six per CU, and every finishing wave adds at most 64 partials, one per
// lane.  At B = 1 the 196 blocks still cover most of the 256 CUs.  The caps bound the finishing wave's serial chain, not the first launch.
constexpr int PM_LIK_ELEMS = 4096, PM_LIK_MAX_BLOCKS = 32;
constexpr int PM_SQ_PIXELS = 1024, PM_SQ_MAX_BLOCKS = 64;

struct PmSq {
    const void* a; const void* b; int a_dt, b_dt; int64_t as[4], bs[4];
};
struct PmBatch {
    int B, n_lik, C, H, W;
    int start[11];                 // first block of job j (8 likelihood maps + 2 image pairs + the end marker); job j has B * nb[j] blocks
    int nb[10];                    // blocks per image of job j
    int ws_off[10];                // first fp64 partial of job j: lik (B, nb), image pair (B, nb, 2)
    const float* lik[8]; int64_t per[8];
    PmSq sq[2];
    double* ws;
};

static inline int lik_blocks(int64_t per) { return grid_for(per, PM_LIK_ELEMS, PM_LIK_MAX_BLOCKS); }
static inline int sq_blocks(int64_t npix) { return grid_for(npix, PM_SQ_PIXELS, PM_SQ_MAX_BLOCKS); }

__device__ __forceinline__ double block_sum(double acc, double* red) {
    acc = wave_sum_d(acc);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
    __syncthreads();
    return red[0] + red[1] + red[2] + red[3];
}

__device__ __forceinline__ double log2_4(float x, float y, float z, float w) {
    return (double)log2f(x) + (double)log2f(y) + (double)log2f(z) + (double)log2f(w);
}

__device__ __forceinline__ void pm_lik_body(const float* __restrict__ p, int64_t n, int bid, int nb, double* red, double* __restrict__ dst) {
    double acc = 0.0;
    const int64_t gt = bid * (int64_t)PM_THREADS + threadIdx.x, stride = (int64_t)nb * PM_THREADS;
    const int64_t n4 = n >> 2;
    if (((uintptr_t)p & 15) == 0) {
        for (int64_t i = gt; i < n4; i += stride) {
            const f32x4 v = ((const f32x4*)p)[i];
            acc += log2_4(v.x, v.y, v.z, v.w);
        }
    } else {
        for (int64_t i = gt; i < n4; i += stride) acc += log2_4(p[4 * i], p[4 * i + 1], p[4 * i + 2], p[4 * i + 3]);
    }
    for (int64_t i = n4 * 4 + gt; i < n; i += stride) acc += (double)log2f(p[i]);
    const double s = block_sum(acc, red);
    if (threadIdx.x == 0) *dst = s;
}

// what the decoder's PNG holds for v (codec.quantise: clamp, * 255, round half to even, all in fp32); fmaxf would turn a NaN into 0
__device__ __forceinline__ float q8(float v) { return v != v ? v : rintf(fminf(fmaxf(v, 0.f), 1.f) * 255.f); }

__device__ __forceinline__ void pm_sq_body(const PmSq& q, int img, int C, int H, int W, int bid, int nb, double* red, double* __restrict__ dst) {
    const int npix = H * W;                                    // < 2^31 (checked by the launcher): a 32-bit index split
    const int64_t ba = img * q.as[0], bb = img * q.bs[0];
    double acc = 0.0, acc8 = 0.0;
    auto offsets = [&](int p, int64_t& oa, int64_t& ob) {
        const unsigned y = (unsigned)p / (unsigned)W, x = (unsigned)p - y * (unsigned)W;
        oa = ba + y * q.as[2] + x * q.as[3];
        ob = bb + y * q.bs[2] + x * q.bs[3];
    };
    const int64_t stride = (int64_t)nb * PM_THREADS;
    int64_t p = bid * (int64_t)PM_THREADS + threadIdx.x;
    if (C == 3) {
        // the image case, as in sum_sq_diff_body: 4 pixels x 3 channels x 2 operands = 24 independent loads in flight per lane.  The sums are
        // taken pixel by pixel in increasing order, exactly as the loop below would
        for (; p + 3 * stride < npix; p += 4 * stride) {
            float va[4][3], vb[4][3];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                int64_t oa, ob;
                offsets((int)(p + u * stride), oa, ob);
#pragma unroll
                for (int c = 0; c < 3; ++c) { va[u][c] = ld_any(q.a, oa + c * q.as[1], q.a_dt); vb[u][c] = ld_any(q.b, ob + c * q.bs[1], q.b_dt); }
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                float part = 0.f, part8 = 0.f;
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    const float df = va[u][c] - vb[u][c], d8 = q8(va[u][c]) - q8(vb[u][c]);
                    part = fmaf(df, df, part);
                    part8 = fmaf(d8, d8, part8);
                }
                acc += (double)part;
                acc8 += (double)part8;
            }
        }
    }
    for (; p < npix; p += stride) {
        int64_t oa, ob;
        offsets((int)p, oa, ob);
        float part = 0.f, part8 = 0.f;
        for (int c = 0; c < C; ++c) {
            const float va = ld_any(q.a, oa + c * q.as[1], q.a_dt), vb = ld_any(q.b, ob + c * q.bs[1], q.b_dt);
            const float df = va - vb, d8 = q8(va) - q8(vb);
            part = fmaf(df, df, part);
            part8 = fmaf(d8, d8, part8);
            if ((c & 7) == 7) { acc += (double)part; acc8 += (double)part8; part = 0.f; part8 = 0.f; }
        }
        acc += (double)part;
        acc8 += (double)part8;
    }
    const double s = block_sum(acc, red);
    const double s8 = block_sum(acc8, red + 4);
    if (threadIdx.x == 0) { dst[0] = s; dst[1] = s8; }
}

__global__ __launch_bounds__(PM_THREADS) void pair_metrics_partial_kernel(const PmBatch m) {
    __shared__ double red[8];
    const int n = m.n_lik + 2;
    int j = 0;
    while (j + 1 < n && (int)blockIdx.x >= m.start[j + 1]) ++j;
    const int r = (int)blockIdx.x - m.start[j], nb = m.nb[j];
    const int img = r / nb, bid = r - img * nb;
    if (j < m.n_lik)
        pm_lik_body(m.lik[j] + (int64_t)img * m.per[j], m.per[j], bid, nb, red, m.ws + m.ws_off[j] + r);
    else
        pm_sq_body(m.sq[j - m.n_lik], img, m.C, m.H, m.W, bid, nb, red, m.ws + m.ws_off[j] + 2 * (int64_t)r);
}

// One wave per (image, column): lane k fetches partial k of the job (at most 64, so one load each, all in flight together), then the wave adds
// them in index order through readlanes, starting FROM the first (not from +0, which would lose a -0).  A single thread walking the partials
// waits for one load per addition: at B = 1, 512^2 the whole call took 21.9 us that way and takes 19.1 us this way (33.5 -> 31.2 us at B = 8;
// graph replays, profiles/pair_metrics_bench.json).
static_assert(PM_LIK_MAX_BLOCKS <= 64 && PM_SQ_MAX_BLOCKS <= 64, "the finishing wave holds one partial per lane");
constexpr int PM_FINISH_WAVES = 4;
__global__ __launch_bounds__(64 * PM_FINISH_WAVES) void pair_metrics_finish_kernel(const PmBatch m, double* __restrict__ out) {
    const int ncol = m.n_lik + 4;
    const int i = blockIdx.x * PM_FINISH_WAVES + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (i >= m.B * ncol) return;                               // wave-uniform
    const int img = i / ncol, col = i - img * ncol;
    int j, step, first;
    if (col < m.n_lik) { j = col; step = 1; first = 0; }
    else { j = m.n_lik + ((col - m.n_lik) & 1); step = 2; first = (col - m.n_lik) >> 1; }
    const int nb = m.nb[j];
    const double* p = m.ws + m.ws_off[j] + (int64_t)img * nb * step + first;
    const double v = lane < nb ? p[(int64_t)lane * step] : 0.0;
    double s = __shfl(v, 0, 64);
    for (int k = 1; k < nb; ++k) s += __shfl(v, k, 64);
    if (lane == 0) out[i] = s;
}

// the argument checks both entry points share + the job table; `numel` may be NULL when n_lik == 0.  *n_partials: the fp64 values `ws` must hold
int pm_plan(const char* who, int B, int n_lik, const int64_t* numel, int H, int W, PmBatch* m, int64_t* n_partials) {
    HESIC_CHECK_ARG(n_lik >= 0 && n_lik <= HESIC_PAIR_METRICS_MAX_LIK, "%s: n_lik = %d outside 0..8", who, n_lik);
    HESIC_CHECK_ARG(B >= 1 && H >= 1 && W >= 1, "%s: non-positive dims B=%d H=%d W=%d", who, B, H, W);
    HESIC_CHECK_ARG(B <= (1 << 20), "%s: B = %d pairs, more than 2^20", who, B);
    HESIC_CHECK_ARG(n_lik == 0 || numel, "%s: null pointer (numel)", who);
    HESIC_CHECK_ARG((int64_t)H * W < (1ll << 31), "%s: H * W = %lld pixels an image, 2^31 or more", who, (long long)((int64_t)H * W));
    int64_t blocks = 0, partials = 0;
    for (int j = 0; j < n_lik + 2; ++j) {
        int nb;
        if (j < n_lik) {
            HESIC_CHECK_ARG(numel[j] > 0, "%s: likelihood map %d: non-positive numel %lld", who, j, (long long)numel[j]);
            HESIC_CHECK_ARG(numel[j] % B == 0, "%s: likelihood map %d: numel %lld is not a multiple of B = %d", who, j, (long long)numel[j], B);
            nb = lik_blocks(numel[j] / B);
            m->per[j] = numel[j] / B;
        } else {
            nb = sq_blocks((int64_t)H * W);
        }
        HESIC_CHECK_ARG(blocks + (int64_t)B * nb <= INT32_MAX / 2, "%s: too many blocks (B = %d)", who, B);
        m->start[j] = (int)blocks; m->nb[j] = nb; m->ws_off[j] = (int)partials;
        blocks += (int64_t)B * nb;
        partials += (int64_t)B * nb * (j < n_lik ? 1 : 2);
    }
    m->start[n_lik + 2] = (int)blocks;
    m->B = B; m->n_lik = n_lik; m->H = H; m->W = W;
    *n_partials = partials;
    return 0;
}

}  // namespace

extern "C" int64_t hesic_pair_metrics_ws_bytes(int B, int n_lik, const int64_t* numel, int H, int W) {
    PmBatch m;
    memset(&m, 0, sizeof(m));
    int64_t partials = 0;
    return pm_plan("pair_metrics_ws_bytes", B, n_lik, numel, H, W, &m, &partials) != 0 ? -1 : partials * (int64_t)sizeof(double);
}

extern "C" int hesic_pair_metrics(int B, int n_lik, const float* const* lik, const int64_t* numel, const void* const* a, const int* a_dtype,
                                  const int64_t* a_strides, const void* const* b, const int* b_dtype, const int64_t* b_strides, int C, int H,
                                  int W, double* out, void* ws, int64_t ws_bytes, void* stream) {
    HESIC_CHECK_ARG(a && b && a_dtype && b_dtype && a_strides && b_strides && out && ws, "pair_metrics: null pointer");
    HESIC_CHECK_ARG(n_lik <= 0 || (lik && numel), "pair_metrics: null pointer (likelihood maps)");
    HESIC_CHECK_ARG(C >= 1, "pair_metrics: non-positive dims C=%d", C);
    PmBatch m;
    memset(&m, 0, sizeof(m));
    int64_t partials = 0;
    if (pm_plan("pair_metrics", B, n_lik, numel, H, W, &m, &partials) != 0) return HESIC_EINVAL;
    for (int i = 0; i < n_lik; ++i) {
        HESIC_CHECK_ARG(lik[i], "pair_metrics: null pointer (likelihood map %d)", i);
        HESIC_CHECK_ARG(((uintptr_t)lik[i] & 3) == 0, "pair_metrics: likelihood map %d is not 4-byte aligned", i);
        m.lik[i] = lik[i];
    }
    for (int s = 0; s < 2; ++s) {
        HESIC_CHECK_ARG(a[s] && b[s], "pair_metrics: null pointer (image pair %d)", s);
        HESIC_CHECK_ARG((a_dtype[s] == HESIC_F32 || a_dtype[s] == HESIC_H16) && (b_dtype[s] == HESIC_F32 || b_dtype[s] == HESIC_H16),
                        "pair_metrics: image pair %d: bad dtype", s);
        PmSq& q = m.sq[s];
        q.a = a[s]; q.b = b[s]; q.a_dt = a_dtype[s]; q.b_dt = b_dtype[s];
        for (int k = 0; k < 4; ++k) { q.as[k] = a_strides[4 * s + k]; q.bs[k] = b_strides[4 * s + k]; }
    }
    HESIC_CHECK_ARG(((uintptr_t)ws & 7) == 0 && ((uintptr_t)out & 7) == 0, "pair_metrics: out / workspace not 8-byte aligned");
    HESIC_CHECK_ARG(ws_bytes >= partials * (int64_t)sizeof(double), "pair_metrics: workspace too small (%lld bytes, %lld needed)", (long long)ws_bytes,
                    (long long)(partials * (int64_t)sizeof(double)));
    m.C = C;
    m.ws = (double*)ws;
    hipLaunchKernelGGL(pair_metrics_partial_kernel, dim3((unsigned)m.start[n_lik + 2]), dim3(PM_THREADS), 0, (hipStream_t)stream, m);
    const int cells = B * (n_lik + 4);
    hipLaunchKernelGGL(pair_metrics_finish_kernel, dim3((unsigned)cdiv64(cells, PM_FINISH_WAVES)), dim3(64 * PM_FINISH_WAVES), 0,
                       (hipStream_t)stream, m, out);
    HESIC_LAUNCH_RETURN("pair_metrics");
}

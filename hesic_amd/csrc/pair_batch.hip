// A training batch of stereo crops gathered from uint8 images resident on the device (include/hesic_pair_batch.h): crop, ToTensor and the
// re-based homography of every item and both views in ONE launch.  It is the loader's host path (compressai.datasets.ImageFolder.__getitem__ /
// _pair_homography) with the decode taken out: the bytes were decoded once and stay in device memory.
//
// Thread map: a thread owns four consecutive pixels of one crop row, x fastest: a wave reads 768 contiguous source bytes and writes 1024
// contiguous bytes into each of the three channel planes (dwordx4 stores when pw % 4 == 0).  Stores carry the traffic (12 output bytes per
// source byte).  The 12 source bytes start at any byte alignment: they are fetched as the four aligned dwords that cover them and shifted into
// place (v_alignbit); where that 16-byte window would leave the item's view -- only at the first and last pixels of a stored image -- the
// thread reads exactly its bytes one by one.  No LDS, no atomics.  The value of a byte is computed (one IEEE division), not looked up, as in
// homography_prep.hip.
#include "common.h"
#include "../../include/hesic_pair_batch.h"

namespace {

constexpr int PB_THREADS = 256;

__device__ __forceinline__ float pb_unit(uint32_t byte) { return __fdiv_rn((float)byte, 255.0f); }

// T(-t) H T(t) / [2,2] in fp64, every operation rounded on its own (the header's formulas, operation for operation)
__device__ void pb_matrix(const hesic_pair_item& it, const double* __restrict__ h_table, float* __restrict__ out) {
    if (it.h_index < 0) {
#pragma unroll
        for (int i = 0; i < 9; ++i) out[i] = (i % 4 == 0) ? 1.f : 0.f;
        return;
    }
    const double* H = h_table + (int64_t)it.h_index * 9;
    const double hx = (double)it.hx, hy = (double)it.hy;
    double G[3][3], R[3][3];
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        const double h2 = H[6 + j];
        G[0][j] = __dadd_rn(H[j], -__dmul_rn(hx, h2));
        G[1][j] = __dadd_rn(H[3 + j], -__dmul_rn(hy, h2));
        G[2][j] = h2;
    }
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        R[i][0] = G[i][0];
        R[i][1] = G[i][1];
        R[i][2] = __dadd_rn(__dadd_rn(__dmul_rn(G[i][0], hx), __dmul_rn(G[i][1], hy)), G[i][2]);
    }
    const double d = R[2][2];
#pragma unroll
    for (int i = 0; i < 9; ++i) out[i] = (float)__ddiv_rn(R[i / 3][i % 3], d);
}

template <bool VEC>
__global__ __launch_bounds__(PB_THREADS) void pair_batch_gather_kernel(const hesic_pair_item* __restrict__ items,
                                                                       const double* __restrict__ h_table, int ph, int pw, int pw4,
                                                                       int blocks_per_image, float* __restrict__ x1, float* __restrict__ x2,
                                                                       float* __restrict__ h_out) {
    const int b = blockIdx.x / blocks_per_image;
    const int blk = blockIdx.x - b * blocks_per_image;
    const hesic_pair_item it = items[b];
    if (blk == 0 && blockIdx.y == 0 && threadIdx.x == 0) pb_matrix(it, h_table, h_out + (int64_t)b * 9);
    const int idx = blk * PB_THREADS + threadIdx.x;
    if (idx >= ph * pw4) return;
    const int r = idx / pw4, q = (idx - r * pw4) * 4;
    const int n = min(4, pw - q);                                   // pixels of this thread: 4, fewer at the end of a row when pw % 4 != 0
    const uint8_t* view = blockIdx.y == 0 ? it.left : it.right;
    float* x = blockIdx.y == 0 ? x1 : x2;
    const uintptr_t lo = (uintptr_t)view, hi = lo + (uintptr_t)it.rows * (uintptr_t)it.pitch_px * 3u;
    const uintptr_t a = lo + ((uintptr_t)(it.y0 + r) * (uintptr_t)it.pitch_px + (uintptr_t)(it.x0 + q)) * 3u;
    const uintptr_t a0 = a & ~(uintptr_t)3;
    uint32_t d[3];
    if (a0 >= lo && a0 + 16 <= hi) {
        const __attribute__((address_space(1))) uint32_t* w = (const __attribute__((address_space(1))) uint32_t*)a0;      // global, not flat, loads
        const uint32_t s = (uint32_t)(a & 3) * 8u;
        d[0] = __funnelshift_r(w[0], w[1], s);
        d[1] = __funnelshift_r(w[1], w[2], s);
        d[2] = __funnelshift_r(w[2], w[3], s);
    } else {
        const __attribute__((address_space(1))) uint8_t* p = (const __attribute__((address_space(1))) uint8_t*)a;
        d[0] = d[1] = d[2] = 0u;
#pragma unroll
        for (int j = 0; j < 12; ++j)
            if (j < 3 * n) d[j >> 2] |= (uint32_t)p[j] << (8 * (j & 3));
    }
    float v[3][4];                                                  // [channel][pixel]
#pragma unroll
    for (int j = 0; j < 12; ++j) v[j % 3][j / 3] = pb_unit((d[j >> 2] >> (8 * (j & 3))) & 0xffu);
    const int64_t plane = (int64_t)ph * pw;
    float* o = x + (int64_t)b * 3 * plane + (int64_t)r * pw + q;
    if (VEC) {
#pragma unroll
        for (int c = 0; c < 3; ++c) *(f32x4*)(o + c * plane) = f32x4{v[c][0], v[c][1], v[c][2], v[c][3]};
    } else {
#pragma unroll
        for (int c = 0; c < 3; ++c)
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (k < n) o[c * plane + k] = v[c][k];
    }
}

}  // namespace

extern "C" int hesic_pair_batch_gather(const hesic_pair_item* items, const double* h_table, int B, int ph, int pw, float* x1, float* x2,
                                       float* h_out, void* stream) {
    static_assert(sizeof(hesic_pair_item) == 48, "hesic_pair_item is 48 bytes");
    HESIC_CHECK_ARG(items && x1 && x2 && h_out, "pair_batch_gather: null pointer");
    HESIC_CHECK_ARG(B >= 1 && ph >= 1 && pw >= 1, "pair_batch_gather: bad shape B=%d ph=%d pw=%d", B, ph, pw);
    HESIC_CHECK_ARG((int64_t)B * 3 * ph <= INT32_MAX / (int64_t)pw, "pair_batch_gather: B * 3 * ph * pw overflows int32 (B=%d ph=%d pw=%d)", B, ph,
                    pw);
    HESIC_CHECK_ARG(((uintptr_t)items & 7) == 0 && ((uintptr_t)h_table & 7) == 0 && (((uintptr_t)x1 | (uintptr_t)x2 | (uintptr_t)h_out) & 3) == 0,
                    "pair_batch_gather: misaligned pointer");
    const int pw4 = (pw + 3) / 4;
    const int blocks_per_image = (int)cdiv64((int64_t)ph * pw4, PB_THREADS);
    const dim3 grid((unsigned)((int64_t)B * blocks_per_image), 2, 1);
    const bool vec = pw % 4 == 0 && (((uintptr_t)x1 | (uintptr_t)x2) & 15) == 0;
    if (vec)
        hipLaunchKernelGGL(pair_batch_gather_kernel<true>, grid, dim3(PB_THREADS), 0, (hipStream_t)stream, items, h_table, ph, pw, pw4,
                           blocks_per_image, x1, x2, h_out);
    else
        hipLaunchKernelGGL(pair_batch_gather_kernel<false>, grid, dim3(PB_THREADS), 0, (hipStream_t)stream, items, h_table, ph, pw, pw4,
                           blocks_per_image, x1, x2, h_out);
    HESIC_LAUNCH_RETURN("pair_batch_gather");
}

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
//
// hesic_pair_batch_gather_aug (include/hesic_pair_augment.h) is the same kernel with AUG = true: the descriptor's `reserved` word holds flip and
// swap bits.  The thread map is by OUTPUT pixels, so the stores are what they were; a swap picks the other view's pointer, a vertical flip
// another source row, and under a horizontal flip a thread's four output pixels come from four contiguous source pixels in reverse order:
// it loads the group that ENDS where the mirrored position lies and reverses it in registers.  A partial group (pw % 4 != 0) then occupies
// the LAST slots of the loaded group and lies at the crop's first columns; the bytes in front of it belong to the columns before the crop
// (or to the previous row, or to nothing at all at the view's first pixel): the 16-byte window is used only where it lies inside the view,
// and the byte path reads exactly the partial group's own bytes.  AUG = false compiles to the kernel as it was.
#include "common.h"
#include "../../include/hesic_pair_augment.h"

namespace {

constexpr int PB_THREADS = 256;

__device__ __forceinline__ float pb_unit(uint32_t byte) { return __fdiv_rn((float)byte, 255.0f); }

// a * b - c * d, both products and the difference rounded on their own
__device__ __forceinline__ double pb_det2(double a, double b, double c, double d) { return __dadd_rn(__dmul_rn(a, b), -__dmul_rn(c, d)); }

// R <- F R F with F the mirror of axis `ax` (0: x, 1: y) in a crop of extent e + 1 (hesic_pair_augment.h: S = F R, then T = S F)
__device__ __forceinline__ void pb_mirror(double (&R)[3][3], int ax, double e) {
#pragma unroll
    for (int j = 0; j < 3; ++j) R[ax][j] = __dadd_rn(__dmul_rn(e, R[2][j]), -R[ax][j]);
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        const double s = R[i][ax];
        R[i][ax] = -s;
        R[i][2] = __dadd_rn(__dmul_rn(e, s), R[i][2]);
    }
}

// T(-t) H T(t) / [2,2] in fp64, every operation rounded on its own (the headers' formulas, operation for operation); `flags`, `ph`, `pw`:
// the augmentation steps of hesic_pair_augment.h between the re-basing and the division (flags = 0: none)
__device__ void pb_matrix(const hesic_pair_item& it, const double* __restrict__ h_table, float* __restrict__ out, int flags, int ph, int pw) {
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
    if (flags & HESIC_PAIR_HFLIP) pb_mirror(R, 0, (double)(pw - 1));
    if (flags & HESIC_PAIR_VFLIP) pb_mirror(R, 1, (double)(ph - 1));
    if (flags & HESIC_PAIR_SWAP) {
        double U[3][3];
#pragma unroll
        for (int i = 0; i < 3; ++i)
#pragma unroll
            for (int j = 0; j < 3; ++j) {                           // U[i][j] = cofactor (j, i): rows j+1, j+2 and columns i+1, i+2, cyclically
                const int r1 = (j + 1) % 3, r2 = (j + 2) % 3, c1 = (i + 1) % 3, c2 = (i + 2) % 3;
                U[i][j] = pb_det2(R[r1][c1], R[r2][c2], R[r1][c2], R[r2][c1]);
            }
#pragma unroll
        for (int i = 0; i < 9; ++i) R[i / 3][i % 3] = U[i / 3][i % 3];
    }
    const double d = R[2][2];
#pragma unroll
    for (int i = 0; i < 9; ++i) out[i] = (float)__ddiv_rn(R[i / 3][i % 3], d);
}

template <bool VEC, bool AUG>
__global__ __launch_bounds__(PB_THREADS) void pair_batch_gather_kernel(const hesic_pair_item* __restrict__ items,
                                                                       const double* __restrict__ h_table, int ph, int pw, int pw4,
                                                                       int blocks_per_image, float* __restrict__ x1, float* __restrict__ x2,
                                                                       float* __restrict__ h_out) {
    const int b = blockIdx.x / blocks_per_image;
    const int blk = blockIdx.x - b * blocks_per_image;
    const hesic_pair_item it = items[b];
    const int flags = AUG ? it.reserved : 0;
    const bool hflip = AUG && (flags & HESIC_PAIR_HFLIP), vflip = AUG && (flags & HESIC_PAIR_VFLIP), swap = AUG && (flags & HESIC_PAIR_SWAP);
    if (blk == 0 && blockIdx.y == 0 && threadIdx.x == 0) pb_matrix(it, h_table, h_out + (int64_t)b * 9, flags, ph, pw);
    const int idx = blk * PB_THREADS + threadIdx.x;
    if (idx >= ph * pw4) return;
    const int r = idx / pw4, q = (idx - r * pw4) * 4;
    const int n = min(4, pw - q);                                   // pixels of this thread: 4, fewer at the end of a row when pw % 4 != 0
    const uint8_t* view = ((blockIdx.y == 0) != swap) ? it.left : it.right;
    float* x = blockIdx.y == 0 ? x1 : x2;
    // the four-pixel source group [qs, qs + 4) of the crop's row rs; this thread's n pixels are its slots [s0, s0 + n).  Mirrored, output
    // pixel q + k is source pixel pw - 1 - q - k: the group ends at pw - q, and a partial group fills its LAST slots (qs < 0 then)
    const int rs = vflip ? ph - 1 - r : r;
    const int qs = hflip ? pw - q - 4 : q;
    const int s0 = hflip ? 4 - n : 0;
    const uintptr_t lo = (uintptr_t)view, hi = lo + (uintptr_t)it.rows * (uintptr_t)it.pitch_px * 3u;
    const uintptr_t a = lo + (uintptr_t)(((int64_t)(it.y0 + rs) * it.pitch_px + (it.x0 + qs)) * 3);     // below lo only where the byte path is taken
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
            if (j >= 3 * s0 && j < 3 * (s0 + n)) d[j >> 2] |= (uint32_t)p[j] << (8 * (j & 3));
    }
    float v[3][4];                                                  // [channel][pixel of the output]
#pragma unroll
    for (int j = 0; j < 12; ++j) v[j % 3][j / 3] = pb_unit((d[j >> 2] >> (8 * (j & 3))) & 0xffu);
    if (AUG) {
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const float t0 = v[c][0], t1 = v[c][1];
            v[c][0] = hflip ? v[c][3] : t0;
            v[c][1] = hflip ? v[c][2] : t1;
            v[c][2] = hflip ? t1 : v[c][2];
            v[c][3] = hflip ? t0 : v[c][3];
        }
    }
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

// the shared host side of both entries: the checks, the launch shape (the headers state it) and the choice of the store path
template <bool AUG>
int pb_launch(const char* name, const hesic_pair_item* items, const double* h_table, int B, int ph, int pw, float* x1, float* x2, float* h_out,
              void* stream) {
    static_assert(sizeof(hesic_pair_item) == 48, "hesic_pair_item is 48 bytes");
    HESIC_CHECK_ARG(items && x1 && x2 && h_out, "%s: null pointer", name);
    HESIC_CHECK_ARG(B >= 1 && ph >= 1 && pw >= 1, "%s: bad shape B=%d ph=%d pw=%d", name, B, ph, pw);
    HESIC_CHECK_ARG((int64_t)B * 3 * ph <= INT32_MAX / (int64_t)pw, "%s: B * 3 * ph * pw overflows int32 (B=%d ph=%d pw=%d)", name, B, ph, pw);
    HESIC_CHECK_ARG(((uintptr_t)items & 7) == 0 && ((uintptr_t)h_table & 7) == 0 && (((uintptr_t)x1 | (uintptr_t)x2 | (uintptr_t)h_out) & 3) == 0,
                    "%s: misaligned pointer", name);
    const int pw4 = (pw + 3) / 4;
    const int blocks_per_image = (int)cdiv64((int64_t)ph * pw4, PB_THREADS);
    const dim3 grid((unsigned)((int64_t)B * blocks_per_image), 2, 1);
    const bool vec = pw % 4 == 0 && (((uintptr_t)x1 | (uintptr_t)x2) & 15) == 0;
    if (vec)
        hipLaunchKernelGGL((pair_batch_gather_kernel<true, AUG>), grid, dim3(PB_THREADS), 0, (hipStream_t)stream, items, h_table, ph, pw, pw4,
                           blocks_per_image, x1, x2, h_out);
    else
        hipLaunchKernelGGL((pair_batch_gather_kernel<false, AUG>), grid, dim3(PB_THREADS), 0, (hipStream_t)stream, items, h_table, ph, pw, pw4,
                           blocks_per_image, x1, x2, h_out);
    HESIC_LAUNCH_RETURN(name);
}

}  // namespace

extern "C" int hesic_pair_batch_gather(const hesic_pair_item* items, const double* h_table, int B, int ph, int pw, float* x1, float* x2,
                                       float* h_out, void* stream) {
    return pb_launch<false>("pair_batch_gather", items, h_table, B, ph, pw, x1, x2, h_out, stream);
}

extern "C" int hesic_pair_batch_gather_aug(const hesic_pair_item* items, const double* h_table, int B, int ph, int pw, float* x1, float* x2,
                                           float* h_out, void* stream) {
    return pb_launch<true>("pair_batch_gather_aug", items, h_table, B, ph, pw, x1, x2, h_out, stream);
}

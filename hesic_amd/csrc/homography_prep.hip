// HomographyNet's inputs from a stereo pair on the device (include/hesic_homography_prep.h): resize to S x S, quantise, normalise, average to
// grey, cut the P x P window and write its corners -- both views in ONE launch.  It is the loader's host path (compressai.datasets:
// _resize_bilinear + ImageFolder._homonet_inputs) written as an explicit fp32 sequence, so the two agree to the last grey level.
//
// Thread map: one grey element per thread, x fastest (a wave writes 256 contiguous bytes of grey and, inside the window, of the patch);
// blockIdx.y = item, blockIdx.z = view.  The four taps of a thread are two pairs of neighbouring columns on two rows: when shrinking by k
// a wave's reads cover 64 k consecutive columns per row and channel, every fetched line is used (by this wave or the next row's).  No LDS,
// no atomics; memory- and latency-bound (12 gathered loads, ~9 IEEE divisions, 4 B + the window's share stored per thread).
#include "common.h"
#include "homonet_prep_dev.h"
#include "../../include/hesic_homography_prep.h"

namespace {

struct PrepView {
    const void* x;
    int64_t sb, sc, sy, sx;
    float* grey;
    float* patch;
};

template <bool F32>
__global__ __launch_bounds__(PREP_THREADS) void homonet_prepare_kernel(const PrepView v1, const PrepView v2, const int32_t* __restrict__ xy,
                                                                       float* __restrict__ corners, int H, int W, int S, int P, float scale_y,
                                                                       float scale_x, float mean, float std) {
    const int b = blockIdx.y;
    const PrepView v = blockIdx.z == 0 ? v1 : v2;
    const int wx = xy[2 * b], wy = xy[2 * b + 1];
    if (blockIdx.x == 0 && blockIdx.z == 0 && threadIdx.x < 8) {
        // [[x, y], [x+P, y], [x+P, y+P], [x, y+P]]: corner k = threadIdx.x >> 1 adds P to x for k = 1, 2 and to y for k = 2, 3
        const int k = threadIdx.x >> 1;
        const int val = (threadIdx.x & 1) ? wy + (k >= 2 ? P : 0) : wx + ((k == 1 || k == 2) ? P : 0);
        corners[(int64_t)b * 8 + threadIdx.x] = (float)val;
    }
    const int idx = blockIdx.x * PREP_THREADS + threadIdx.x;
    if (idx >= S * S) return;
    const int y = idx / S, x = idx - y * S;
    const PrepAxis ay = prep_axis(y, H, scale_y), ax = prep_axis(x, W, scale_x);
    const int64_t base = (int64_t)b * v.sb;
    const int64_t r0 = base + (int64_t)ay.i0 * v.sy, r1 = base + (int64_t)ay.i1 * v.sy;
    const int64_t c0 = (int64_t)ax.i0 * v.sx, c1 = (int64_t)ax.i1 * v.sx;
    float n[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const int64_t co = (int64_t)c * v.sc;
        const float ta = prep_level<F32>(v.x, r0 + c0 + co), tb = prep_level<F32>(v.x, r0 + c1 + co);
        const float tc = prep_level<F32>(v.x, r1 + c0 + co), td = prep_level<F32>(v.x, r1 + c1 + co);
        n[c] = prep_normalise(prep_resample(ta, tb, tc, td, ax, ay), mean, std);
    }
    float g;
    {
#pragma clang fp contract(off)
        g = __fdiv_rn((n[0] + n[1]) + n[2], 3.f);
    }
    v.grey[((int64_t)b * S + y) * S + x] = g;
    // unsigned compares: inside the window AND inside the patch buffer whatever xy holds
    const unsigned px = (unsigned)(x - wx), py = (unsigned)(y - wy);
    if (px < (unsigned)P && py < (unsigned)P) v.patch[((int64_t)b * P + py) * P + px] = g;
}

// ------------------------------------------------------------------------------------------------------------------ the item form
// hesic_homonet_prepare_items (include/hesic_homonet_items.h): the same thread map and the same device functions (homonet_prep_dev.h), the
// sources being stored HWC bytes of per-item geometry.  blockIdx.y = item: the descriptor is block-uniform and read once (scalar loads).
__global__ __launch_bounds__(PREP_THREADS) void homonet_prepare_items_kernel(const hesic_homonet_item* __restrict__ items, float* __restrict__ grey1,
                                                                             float* __restrict__ grey2, float* __restrict__ patch1,
                                                                             float* __restrict__ patch2, float* __restrict__ corners, int S, int P,
                                                                             float mean, float std) {
    const int b = blockIdx.y;
    const hesic_homonet_item it = items[b];
    const int wx = it.wx, wy = it.wy;
    if (blockIdx.x == 0 && blockIdx.z == 0 && threadIdx.x < 8) corners[(int64_t)b * 8 + threadIdx.x] = prep_corner_word(threadIdx.x, wx, wy, P);
    const int idx = blockIdx.x * PREP_THREADS + threadIdx.x;
    if (idx >= S * S) return;
    const int y = idx / S, x = idx - y * S;
    const PrepCrop crop{blockIdx.z == 0 ? it.left : it.right, it.pitch_px, it.x0, it.y0, it.cw, it.ch};
    const float g = prep_item_grey(crop, S, x, y, mean, std);
    float* grey = blockIdx.z == 0 ? grey1 : grey2;
    float* patch = blockIdx.z == 0 ? patch1 : patch2;
    grey[((int64_t)b * S + y) * S + x] = g;
    // unsigned compares: inside the window AND inside the patch buffer whatever the descriptor holds
    const unsigned px = (unsigned)(x - wx), py = (unsigned)(y - wy);
    if (px < (unsigned)P && py < (unsigned)P) patch[((int64_t)b * P + py) * P + px] = g;
}

}  // namespace

extern "C" int hesic_homonet_prepare_items(const hesic_homonet_item* items, int B, int S, int P, float mean, float std, float* grey1, float* grey2,
                                           float* patch1, float* patch2, float* corners, void* stream) {
    static_assert(sizeof(hesic_homonet_item) == 48, "hesic_homonet_item is 48 bytes");
    HESIC_CHECK_ARG(items && grey1 && grey2 && patch1 && patch2 && corners, "homonet_prepare_items: null pointer");
    HESIC_CHECK_ARG(B >= 1 && B <= 65535, "homonet_prepare_items: bad shape B=%d", B);
    HESIC_CHECK_ARG(S >= 1 && S <= 16384 && P >= 1 && P <= S, "homonet_prepare_items: need 1 <= P <= S <= 16384, got S=%d P=%d", S, P);
    HESIC_CHECK_ARG(std == std && mean == mean && std != 0.f, "homonet_prepare_items: std must be non-zero, mean and std not NaN");
    HESIC_CHECK_ARG(((uintptr_t)items & 7) == 0 &&
                        (((uintptr_t)grey1 | (uintptr_t)grey2 | (uintptr_t)patch1 | (uintptr_t)patch2 | (uintptr_t)corners) & 3) == 0,
                    "homonet_prepare_items: misaligned pointer");
    const dim3 grid((unsigned)cdiv64((int64_t)S * S, PREP_THREADS), (unsigned)B, 2);
    hipLaunchKernelGGL(homonet_prepare_items_kernel, grid, dim3(PREP_THREADS), 0, (hipStream_t)stream, items, grey1, grey2, patch1, patch2, corners, S,
                       P, mean, std);
    HESIC_LAUNCH_RETURN("homonet_prepare_items");
}

extern "C" int hesic_homonet_prepare(const void* x1, const int64_t* xs1, const void* x2, const int64_t* xs2, const int32_t* xy, int B, int H, int W,
                                     int S, int P, float mean, float std, int dtype, float* grey1, float* grey2, float* patch1, float* patch2,
                                     float* corners, void* stream) {
    HESIC_CHECK_ARG(x1 && x2 && xs1 && xs2 && xy && grey1 && grey2 && patch1 && patch2 && corners, "homonet_prepare: null pointer");
    HESIC_CHECK_ARG(dtype == HESIC_PREP_U8 || dtype == HESIC_PREP_F32, "homonet_prepare: dtype %d (HESIC_PREP_U8 or HESIC_PREP_F32)", dtype);
    HESIC_CHECK_ARG(B >= 1 && B <= 65535 && H >= 1 && W >= 1, "homonet_prepare: bad shape B=%d H=%d W=%d", B, H, W);
    HESIC_CHECK_ARG(S >= 1 && S <= 16384 && P >= 1 && P <= S, "homonet_prepare: need 1 <= P <= S <= 16384, got S=%d P=%d", S, P);
    HESIC_CHECK_ARG(std == std && mean == mean && std != 0.f, "homonet_prepare: std must be non-zero, mean and std not NaN");
    for (int i = 0; i < 4; ++i) HESIC_CHECK_ARG(xs1[i] >= 0 && xs2[i] >= 0, "homonet_prepare: negative stride");
    const int align = dtype == HESIC_PREP_F32 ? 3 : 0;
    HESIC_CHECK_ARG((((uintptr_t)x1 | (uintptr_t)x2) & align) == 0 && (((uintptr_t)xy | (uintptr_t)grey1 | (uintptr_t)grey2 | (uintptr_t)patch1 |
                                                                       (uintptr_t)patch2 | (uintptr_t)corners) & 3) == 0,
                    "homonet_prepare: misaligned pointer");
    const PrepView v1{x1, xs1[0], xs1[1], xs1[2], xs1[3], grey1, patch1}, v2{x2, xs2[0], xs2[1], xs2[2], xs2[3], grey2, patch2};
    const float scale_y = (float)H / (float)S, scale_x = (float)W / (float)S;
    const dim3 grid((unsigned)cdiv64((int64_t)S * S, PREP_THREADS), (unsigned)B, 2);
    if (dtype == HESIC_PREP_F32)
        hipLaunchKernelGGL(homonet_prepare_kernel<true>, grid, dim3(PREP_THREADS), 0, (hipStream_t)stream, v1, v2, xy, corners, H, W, S, P, scale_y,
                           scale_x, mean, std);
    else
        hipLaunchKernelGGL(homonet_prepare_kernel<false>, grid, dim3(PREP_THREADS), 0, (hipStream_t)stream, v1, v2, xy, corners, H, W, S, P, scale_y,
                           scale_x, mean, std);
    HESIC_LAUNCH_RETURN("homonet_prepare");
}

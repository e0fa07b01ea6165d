// The per-axis, per-tap and per-level device functions of HomographyNet's input preparation, shared by homography_prep.hip
// (hesic_homonet_prepare, hesic_homonet_prepare_items) and homography_synth.hip (hesic_homonet_synth_items): one definition, so the entries
// that promise each other's bits cannot drift apart.
#pragma once
#include "common.h"

namespace {

constexpr int PREP_THREADS = 256;

struct PrepAxis {
    int i0, i1;
    float l0, l1;
};

// every product, sum and difference below is an fp32 operation of its own: a fused multiply-add would move values that sit at k + 0.5
// before the rounding to a level, and the host path (and the numpy restatement the tests hold this to) does not fuse
__device__ __forceinline__ PrepAxis prep_axis(int d, int n, float scale) {
#pragma clang fp contract(off)
    float s = scale * ((float)d + 0.5f) - 0.5f;
    s = s < 0.f ? 0.f : s;
    PrepAxis a;
    a.i0 = min((int)s, n - 1);
    a.i1 = min(a.i0 + 1, n - 1);
    a.l1 = s - (float)a.i0;
    a.l0 = 1.f - a.l1;
    return a;
}

template <bool F32> __device__ __forceinline__ float prep_level(const void* x, int64_t off) {
    if (F32) {
#pragma clang fp contract(off)
        const float q = rintf(255.f * ((const float*)x)[off]);
        return fminf(fmaxf(q, 0.f), 255.f);
    }
    return (float)((const uint8_t*)x)[off];
}

__device__ __forceinline__ float prep_resample(float a, float b, float c, float d, const PrepAxis& ax, const PrepAxis& ay) {
#pragma clang fp contract(off)
    const float top = ax.l0 * a + ax.l1 * b;
    const float bot = ax.l0 * c + ax.l1 * d;
    const float v = ay.l0 * top + ay.l1 * bot;
    return fminf(fmaxf(rintf(v), 0.f), 255.f);          // rintf: ties to even
}

__device__ __forceinline__ float prep_normalise(float r, float mean, float std) {
#pragma clang fp contract(off)
    return __fdiv_rn(__fdiv_rn(r, 255.f) - mean, std);
}

// ------------------------------------------------------------------------------------------------------------------ the item form
// The sources are stored HWC bytes of per-item geometry.  A row's two taps are two neighbouring pixels = six adjacent bytes: they are
// fetched as one dword and one ushort at byte alignment (gfx950 global loads take any alignment) instead of six strided bytes, so a thread
// issues 4 loads where the strided kernel issues 12, and one 64-bit address per row.  `xs` is the first of the two columns fetched: i0, or
// i0 - 1 at the crop's last column, where i1 == i0 and both taps are the second pixel -- the six bytes never leave the crop's row.  A crop
// one pixel wide (block-uniform) is read as its three bytes.
typedef uint32_t __attribute__((aligned(1))) prep_u32_any;      // a dword / ushort at any byte address
typedef uint16_t __attribute__((aligned(1))) prep_u16_any;

struct PrepTaps {
    uint32_t px[2];         // the two adjacent pixels, R G B in bits 0-23 of each (bits 24-31 are not used)
};

__device__ __forceinline__ PrepTaps prep_load_taps(const uint8_t* p, bool two) {
    const __attribute__((address_space(1))) uint8_t* g = (const __attribute__((address_space(1))) uint8_t*)p;       // global, not flat, loads
    PrepTaps t;
    if (two) {
        const uint32_t lo = *(const __attribute__((address_space(1))) prep_u32_any*)g;
        const uint32_t hi = *(const __attribute__((address_space(1))) prep_u16_any*)(g + 4);
        t.px[0] = lo;
        t.px[1] = __funnelshift_r(lo, hi, 24);
    } else {
        t.px[0] = t.px[1] = (uint32_t)g[0] | ((uint32_t)g[1] << 8) | ((uint32_t)g[2] << 16);       // the one pixel: either tap index reads it
    }
    return t;
}

// channel c of pixel k (0 or 1) of a fetched pair
__device__ __forceinline__ float prep_tap_level(const PrepTaps& t, int k, int c) {
    return (float)(((k ? t.px[1] : t.px[0]) >> (8 * c)) & 0xffu);
}

// the stored crop an item's frame is resized from (the geometry words hesic_homonet_item and hesic_homonet_synth_item share)
struct PrepCrop {
    const uint8_t* view;
    int pitch_px, x0, y0, cw, ch;
};

// element (x, y) of the S x S normalised grey frame of a crop: resize, quantise, normalise, grey
__device__ __forceinline__ float prep_item_grey(const PrepCrop& it, int S, int x, int y, float mean, float std) {
    const float scale_y = __fdiv_rn((float)it.ch, (float)S), scale_x = __fdiv_rn((float)it.cw, (float)S);
    const PrepAxis ay = prep_axis(y, it.ch, scale_y), ax = prep_axis(x, it.cw, scale_x);
    const bool two = it.cw >= 2;
    const int xs = two ? min(ax.i0, it.cw - 2) : 0;
    const int k0 = ax.i0 - xs, k1 = ax.i1 - xs;         // 0 or 1 each
    const int64_t col = (int64_t)(it.x0 + xs) * 3;
    const PrepTaps r0 = prep_load_taps(it.view + (int64_t)(it.y0 + ay.i0) * it.pitch_px * 3 + col, two);
    const PrepTaps r1 = prep_load_taps(it.view + (int64_t)(it.y0 + ay.i1) * it.pitch_px * 3 + col, two);
    float n[3];
#pragma unroll
    for (int c = 0; c < 3; ++c)
        n[c] = prep_normalise(prep_resample(prep_tap_level(r0, k0, c), prep_tap_level(r0, k1, c), prep_tap_level(r1, k0, c),
                                            prep_tap_level(r1, k1, c), ax, ay), mean, std);
    float g;
    {
#pragma clang fp contract(off)
        g = __fdiv_rn((n[0] + n[1]) + n[2], 3.f);
    }
    return g;
}

// corners (B, 4, 2) of item b's window, [[x, y], [x+P, y], [x+P, y+P], [x, y+P]]: thread t < 8 writes word t -- corner k = t >> 1 adds P to
// x for k = 1, 2 and to y for k = 2, 3
__device__ __forceinline__ float prep_corner_word(int t, int wx, int wy, int P) {
    const int k = t >> 1;
    return (float)((t & 1) ? wy + (k >= 2 ? P : 0) : wx + ((k == 1 || k == 2) ? P : 0));
}

}  // namespace

// Synthetic-warp pairs for HomographyNet (include/hesic_homonet_synth.h): the grey frame of one stored view, a known perspective warp of
// it, both windows, and the corner offsets as the label.  Three launches: per item the corners, the label and the fp64 DLT; the frame (the
// item kernel's thread map and device functions, homonet_prep_dev.h, one view); then the warp, one grey_b element per thread, its
// coordinates, weights and four-term sum in fp64 from the stored h, the taps read back from grey_a.  No LDS, no atomics.
#include "common.h"
#include "dlt.h"
#include "homonet_prep_dev.h"
#include "../../include/hesic_homonet_synth.h"

namespace {

// one thread per item: corners, the label, and the fp64 DLT (its 8 x 9 system lives in scratch, which is why it has a launch of its own
// instead of riding in the frame kernel's first block: there it cost every wave of that kernel 656 bytes of scratch and half its occupancy)
__global__ __launch_bounds__(64) void homonet_synth_label_kernel(const hesic_homonet_synth_item* __restrict__ items, float* __restrict__ corners,
                                                                 float* __restrict__ delta, double* __restrict__ h, int B, int P) {
    const int b = blockIdx.x * 64 + threadIdx.x;
    if (b >= B) return;
    const hesic_homonet_synth_item it = items[b];
    double sx[4], sy[4], dx[4], dy[4], hh[9];
    for (int k = 0; k < 4; ++k) {
        const float cx = prep_corner_word(2 * k, it.wx, it.wy, P), cy = prep_corner_word(2 * k + 1, it.wx, it.wy, P);
        corners[(int64_t)b * 8 + 2 * k] = cx;
        corners[(int64_t)b * 8 + 2 * k + 1] = cy;
        delta[(int64_t)b * 8 + 2 * k] = (float)it.delta[2 * k];
        delta[(int64_t)b * 8 + 2 * k + 1] = (float)it.delta[2 * k + 1];
        sx[k] = (double)cx;
        sy[k] = (double)cy;
        dx[k] = sx[k] + (double)it.delta[2 * k];
        dy[k] = sy[k] + (double)it.delta[2 * k + 1];
    }
    if (!dlt4(sx, sy, dx, dy, hh))
        for (int k = 0; k < 9; ++k) hh[k] = NAN;
    for (int k = 0; k < 9; ++k) h[(int64_t)b * 9 + k] = hh[k];
}

__global__ __launch_bounds__(PREP_THREADS) void homonet_synth_frame_kernel(const hesic_homonet_synth_item* __restrict__ items,
                                                                           float* __restrict__ grey_a, float* __restrict__ patch_a, int S, int P,
                                                                           float mean, float std) {
    const int b = blockIdx.y;
    const hesic_homonet_synth_item it = items[b];
    const int wx = it.wx, wy = it.wy;
    const int idx = blockIdx.x * PREP_THREADS + threadIdx.x;
    if (idx >= S * S) return;
    const int y = idx / S, x = idx - y * S;
    const PrepCrop crop{it.view, it.pitch_px, it.x0, it.y0, it.cw, it.ch};
    const float g = prep_item_grey(crop, S, x, y, mean, std);
    grey_a[((int64_t)b * S + y) * S + x] = g;
    // unsigned compares: inside the window AND inside the patch buffer whatever the descriptor holds
    const unsigned px = (unsigned)(x - wx), py = (unsigned)(y - wy);
    if (px < (unsigned)P && py < (unsigned)P) patch_a[((int64_t)b * P + py) * P + px] = g;
}

// floor(coordinate) as a tap index that can be tested against [0, S): anything below -2 (and NaN) becomes -2, anything above S becomes S,
// so neither the index nor its successor is inside unless the coordinate's own cell is
__device__ __forceinline__ int synth_cell(double f, int S) { return (int)fmin(fmax(f, -2.0), (double)S); }

// the header's arithmetic, operation by operation: no contraction anywhere in this kernel
__global__ __launch_bounds__(PREP_THREADS) void homonet_synth_warp_kernel(const hesic_homonet_synth_item* __restrict__ items,
                                                                          const float* __restrict__ grey_a, const double* __restrict__ h,
                                                                          float* __restrict__ grey_b, float* __restrict__ patch_b, int S, int P,
                                                                          int align_corners) {
#pragma clang fp contract(off)
    const int b = blockIdx.y;
    const int wx = items[b].wx, wy = items[b].wy;
    const int idx = blockIdx.x * PREP_THREADS + threadIdx.x;
    if (idx >= S * S) return;
    const int y = idx / S, x = idx - y * S;
    const double* hb = h + (int64_t)b * 9;
    float out;
    if (hb[0] != hb[0]) {
        out = NAN;                                      // a singular configuration: the label kernel wrote NaN into all nine words
    } else {
        const double xd = (double)x, yd = (double)y;
        const double X = (hb[0] * xd + hb[1] * yd) + hb[2];
        const double Y = (hb[3] * xd + hb[4] * yd) + hb[5];
        const double Z = (hb[6] * xd + hb[7] * yd) + hb[8];
        const double u = X / Z, v = Y / Z;
        double sx = u, sy = v;
        if (!align_corners) {
            const double k = (double)S / (double)(S - 1);
            sx = u * k - 0.5;
            sy = v * k - 0.5;
        }
        const double fx = floor(sx), fy = floor(sy);
        const double wx1 = sx - fx, wx0 = 1.0 - wx1, wy1 = sy - fy, wy0 = 1.0 - wy1;
        const int cx = synth_cell(fx, S), cy = synth_cell(fy, S);
        const bool vx0 = cx >= 0 && cx < S, vx1 = cx + 1 >= 0 && cx + 1 < S;
        const bool vy0 = cy >= 0 && cy < S, vy1 = cy + 1 >= 0 && cy + 1 < S;
        const float* src = grey_a + (int64_t)b * S * S + (int64_t)cy * S + cx;      // dereferenced only at taps inside the frame
        double acc = 0.0;
        if (vy0 && vx0) acc = acc + (double)src[0] * (wx0 * wy0);
        if (vy0 && vx1) acc = acc + (double)src[1] * (wx1 * wy0);
        if (vy1 && vx0) acc = acc + (double)src[S] * (wx0 * wy1);
        if (vy1 && vx1) acc = acc + (double)src[S + 1] * (wx1 * wy1);
        out = (float)acc;
    }
    grey_b[((int64_t)b * S + y) * S + x] = out;
    const unsigned px = (unsigned)(x - wx), py = (unsigned)(y - wy);
    if (px < (unsigned)P && py < (unsigned)P) patch_b[((int64_t)b * P + py) * P + px] = out;
}

}  // namespace

extern "C" int hesic_homonet_synth_items(const hesic_homonet_synth_item* items, int B, int S, int P, float mean, float std, int align_corners,
                                         float* grey_a, float* patch_a, float* corners, float* delta, double* h, float* grey_b, float* patch_b,
                                         void* stream) {
    static_assert(sizeof(hesic_homonet_synth_item) == 72, "hesic_homonet_synth_item is 72 bytes");
    HESIC_CHECK_ARG(items && grey_a && patch_a && corners && delta && h && grey_b && patch_b, "homonet_synth_items: null pointer");
    HESIC_CHECK_ARG(B >= 1 && B <= 65535, "homonet_synth_items: bad shape B=%d", B);
    HESIC_CHECK_ARG(S >= 1 && S <= 16384 && P >= 1 && P <= S, "homonet_synth_items: need 1 <= P <= S <= 16384, got S=%d P=%d", S, P);
    HESIC_CHECK_ARG(std == std && mean == mean && std != 0.f, "homonet_synth_items: std must be non-zero, mean and std not NaN");
    HESIC_CHECK_ARG((((uintptr_t)items | (uintptr_t)h) & 7) == 0 &&
                        (((uintptr_t)grey_a | (uintptr_t)patch_a | (uintptr_t)corners | (uintptr_t)delta | (uintptr_t)grey_b | (uintptr_t)patch_b) & 3) == 0,
                    "homonet_synth_items: misaligned pointer");
    const dim3 grid((unsigned)cdiv64((int64_t)S * S, PREP_THREADS), (unsigned)B);
    hipLaunchKernelGGL(homonet_synth_label_kernel, dim3((unsigned)cdiv64(B, 64)), dim3(64), 0, (hipStream_t)stream, items, corners, delta, h, B, P);
    hipLaunchKernelGGL(homonet_synth_frame_kernel, grid, dim3(PREP_THREADS), 0, (hipStream_t)stream, items, grey_a, patch_a, S, P, mean, std);
    hipLaunchKernelGGL(homonet_synth_warp_kernel, grid, dim3(PREP_THREADS), 0, (hipStream_t)stream, items, (const float*)grey_a, (const double*)h,
                       grey_b, patch_b, S, P, align_corners);
    HESIC_LAUNCH_RETURN("homonet_synth_items");
}

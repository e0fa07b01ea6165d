// Stereo homography estimation: SURF keypoints + U-SURF descriptors + 2-NN ratio matching + RANSAC + refit, the GPU form of the
// reference loader's get_H (compressai/datasets/utils.py:30-66: OpenCV-contrib SURF, BFMatcher knnMatch k=2 with the 0.7 ratio
// test, findHomography(RANSAC, 5.0)).  C ABI: include/hesic_stereo_h.h.  Stages, N images (view 1 of B pairs, then view 2):
//   1. grey + integral image     integral_rows_kernel / integral_cols_kernel (exact int32)
//   2. Fast-Hessian              hessian_kernel (20 layers), nms_kernel<false/true> (per-row counts, exclusive scan, ordered writes),
//                                select_kernel (strongest max_kp by a radix select on the response bits, kept in generation order)
//   3. U-SURF descriptor         describe_kernel (one wave per keypoint)
//      oriented / 128-d SURF     orient_kernel (dominant direction, one wave per keypoint), describe_ex_kernel<64 / 128> (the
//                                descriptor in the keypoint's frame; (1, 0) reproduces describe_kernel)
//   4. matching                  match_kernel<64 / 128> (f32 MFMA distance tiles, top-2 in registers), compact_matches_kernel
//   5. RANSAC                    ransac_kernel (one lane per hypothesis, one wave per block so that B = 1 still fills 32
//                                blocks; every block stages the pair's matches in LDS)
//   6. best + refit              finish_kernel (best hypothesis, inlier mask, normalised least-squares DLT + 10 LM steps, fp64)
// Every sum has a fixed order and nothing depends on atomics' order, so a result is bit-identical run to run and does not depend on the
// other pairs of the batch.  The fp32 arithmetic is restated operation by operation in tests/stereo_h_ref.py; contraction into fused
// multiply-adds is switched off here so that restatement can follow it.
#include <cmath>

#include "common.h"
#include "../../include/hesic_stereo_h.h"

#pragma clang fp contract(off)

namespace {

constexpr int N_OCT = 4, N_LAY = 5, N_MID = 3;           // OpenCV SURF defaults: 4 octaves, 3 layers (+2 for the 3x3x3 NMS)
constexpr float HESSIAN_THRESHOLD = 100.f;
constexpr int MAX_DRAWS = 16;
constexpr int LM_ITERS = 10;

struct Layer {
    int size, step, R, C, margin, si, sj;
    int64_t off;
};
struct MidLayer {
    int k, size, step, R, C, margin, ds, rows, row0;       // rows of the NMS scan and their first index in the per-image row table
};
struct Geo {
    Layer L[N_OCT * N_LAY];
    MidLayer M[N_OCT * N_MID];
    int64_t det_elems;
    int rows, cand_cap;
};

Geo geometry(int H, int W) {
    Geo g{};
    int64_t off = 0;
    for (int o = 0; o < N_OCT; ++o)
        for (int l = 0; l < N_LAY; ++l) {
            Layer& L = g.L[o * N_LAY + l];
            L.size = (9 + 6 * l) << o;
            L.step = 1 << o;
            L.R = H / L.step;
            L.C = W / L.step;
            L.margin = (L.size / 2) / L.step;
            const bool fits = L.size <= H && L.size <= W;
            L.si = fits ? 1 + (H - L.size) / L.step : 0;
            L.sj = fits ? 1 + (W - L.size) / L.step : 0;
            L.off = off;
            off += (int64_t)L.R * L.C;
        }
    g.det_elems = off;
    int rows = 0, cap = 0;
    for (int o = 0; o < N_OCT; ++o)
        for (int l = 1; l <= N_MID; ++l) {
            MidLayer& M = g.M[o * N_MID + l - 1];
            const Layer& L = g.L[o * N_LAY + l];
            M.k = o * N_LAY + l;
            M.size = L.size;
            M.step = L.step;
            M.R = L.R;
            M.C = L.C;
            M.margin = (g.L[M.k + 1].size / 2) / L.step + 1;
            M.ds = L.size - g.L[M.k - 1].size;
            M.rows = (L.R - 2 * M.margin > 0 && L.C - 2 * M.margin > 0) ? L.R - 2 * M.margin : 0;
            M.row0 = rows;
            rows += M.rows;
            cap += ((L.R + 1) / 2) * ((L.C + 1) / 2);          // strict 3x3 maxima are never adjacent: at most one per 2x2 cell
        }
    g.rows = rows;
    g.cand_cap = cap > 0 ? cap : 1;
    return g;
}

size_t align256(size_t v) { return (v + 255) & ~(size_t)255; }

struct WsLayout {
    size_t row_cnt, row_off, ncand, cand, best_t, hyp_cnt, hyp_esum, hyp_H, total;
};

WsLayout ws_layout(int B, int H, int W, int max_kp, int n_hyp) {
    const Geo g = geometry(H, W);
    const int64_t N = 2 * (int64_t)B;
    WsLayout w{};
    size_t o = 0;
    w.row_cnt = o; o = align256(o + sizeof(int) * N * (g.rows + 1));
    w.row_off = o; o = align256(o + sizeof(int) * N * (g.rows + 1));
    w.ncand = o; o = align256(o + sizeof(int) * N);
    w.cand = o; o = align256(o + sizeof(float4) * N * g.cand_cap);
    w.best_t = o; o = align256(o + sizeof(int) * B * (int64_t)max_kp);
    w.hyp_cnt = o; o = align256(o + sizeof(int) * B * (int64_t)n_hyp);
    w.hyp_esum = o; o = align256(o + sizeof(float) * B * (int64_t)n_hyp);
    w.hyp_H = o; o = align256(o + sizeof(float) * 9 * B * (int64_t)n_hyp);
    w.total = o;
    return w;
}

// ------------------------------------------------------------------------------------------------ 1. grey + integral image
// cvtColor(COLOR_BGR2GRAY) of the RGB array the reference hands SURF: OpenCV reads channel 0 as blue, so the grey level is
// 0.114 R + 0.587 G + 0.299 B in its 14-bit fixed point (coefficients 1868 / 9617 / 4899).
__device__ __forceinline__ int quant_u8(float v) { return (int)rintf(fminf(fmaxf(v, 0.f), 1.f) * 255.f); }

__global__ void integral_rows_kernel(const void* __restrict__ img, int is_f32, int64_t sb, int64_t sc, int64_t sy, int64_t sx, int H, int W,
                                     int* __restrict__ I) {
    __shared__ int part[256];
    const int y = blockIdx.x, n = blockIdx.y, t = threadIdx.x;
    const int per = (W + 255) / 256, x0 = t * per, x1 = min(W, x0 + per);
    int* row = I + ((int64_t)n * (H + 1) + y + 1) * (W + 1);
    auto grey = [&](int x) -> int {
        const int64_t base = n * sb + y * sy + x * sx;
        int c0, c1, c2;
        if (is_f32) {
            const float* p = (const float*)img;
            c0 = quant_u8(p[base]); c1 = quant_u8(p[base + sc]); c2 = quant_u8(p[base + 2 * sc]);
        } else {
            const uint8_t* p = (const uint8_t*)img;
            c0 = p[base]; c1 = p[base + sc]; c2 = p[base + 2 * sc];
        }
        return (c0 * 1868 + c1 * 9617 + c2 * 4899 + 8192) >> 14;
    };
    int s = 0;
    for (int x = x0; x < x1; ++x) s += grey(x);
    part[t] = s;
    __syncthreads();
    for (int d = 1; d < 256; d <<= 1) {                     // inclusive Hillis-Steele scan of the chunk sums
        const int v = t >= d ? part[t - d] : 0;
        __syncthreads();
        part[t] += v;
        __syncthreads();
    }
    s = t ? part[t - 1] : 0;
    for (int x = x0; x < x1; ++x) {
        s += grey(x);
        row[x + 1] = s;
    }
    if (t == 0) row[0] = 0;
}

__global__ void integral_cols_kernel(int H, int W, int N, int* __restrict__ I) {
    const int x = blockIdx.x * blockDim.x + threadIdx.x, n = blockIdx.y;
    if (x > W || n >= N) return;
    int* p = I + (int64_t)n * (H + 1) * (W + 1) + x;
    p[0] = 0;
    int s = 0;
    for (int y = 1; y <= H; ++y) {
        s += p[(int64_t)y * (W + 1)];
        p[(int64_t)y * (W + 1)] = s;
    }
}

// ------------------------------------------------------------------------------------------------ 2. Fast-Hessian
// OpenCV's calcLayerDetAndTrace: the size-9 Haar patterns scaled by cvRound(size / 9 * c), each box sum times its weight
// sign / area in fp32, the boxes summed in fp64 and rounded to fp32; det = Dxx Dyy - 0.81 Dxy^2 on the layer's sample grid.
struct Box { int x1, y1, x2, y2; float w; };

__device__ __forceinline__ Box scale_box(int x1, int y1, int x2, int y2, int sgn, int size) {
    const float ratio = (float)size / 9.f;
    Box b;
    b.x1 = (int)rintf(ratio * (float)x1); b.y1 = (int)rintf(ratio * (float)y1);
    b.x2 = (int)rintf(ratio * (float)x2); b.y2 = (int)rintf(ratio * (float)y2);
    b.w = (float)sgn / (float)((b.x2 - b.x1) * (b.y2 - b.y1));
    return b;
}

__device__ __forceinline__ float haar(const int* __restrict__ I, int ld, int r0, int c0, const Box* b, int n) {
    double d = 0;
    for (int k = 0; k < n; ++k) {
        const int64_t v = (int64_t)I[(int64_t)(r0 + b[k].y1) * ld + c0 + b[k].x1] + I[(int64_t)(r0 + b[k].y2) * ld + c0 + b[k].x2] -
                          I[(int64_t)(r0 + b[k].y2) * ld + c0 + b[k].x1] - I[(int64_t)(r0 + b[k].y1) * ld + c0 + b[k].x2];
        d += (double)((float)v * b[k].w);
    }
    return (float)d;
}

__global__ void hessian_kernel(const int* __restrict__ Iall, int H, int W, Geo g, float* __restrict__ det_all) {
    const int k = blockIdx.y, n = blockIdx.z;
    const Layer L = g.L[k];
    const int64_t e = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    if (e >= (int64_t)L.R * L.C) return;
    const int i = (int)(e / L.C), j = (int)(e % L.C);
    float v = 0.f;
    const int a = i - L.margin, c = j - L.margin;
    if (a >= 0 && a < L.si && c >= 0 && c < L.sj) {
        const int* I = Iall + (int64_t)n * (H + 1) * (W + 1);
        const Box bx[3] = {scale_box(0, 2, 3, 7, 1, L.size), scale_box(3, 2, 6, 7, -2, L.size), scale_box(6, 2, 9, 7, 1, L.size)};
        const Box by[3] = {scale_box(2, 0, 7, 3, 1, L.size), scale_box(2, 3, 7, 6, -2, L.size), scale_box(2, 6, 7, 9, 1, L.size)};
        const Box bxy[4] = {scale_box(1, 1, 4, 4, 1, L.size), scale_box(5, 1, 8, 4, -1, L.size), scale_box(1, 5, 4, 8, -1, L.size),
                            scale_box(5, 5, 8, 8, 1, L.size)};
        const int r0 = a * L.step, c0 = c * L.step;
        const float dx = haar(I, W + 1, r0, c0, bx, 3), dy = haar(I, W + 1, r0, c0, by, 3), dxy = haar(I, W + 1, r0, c0, bxy, 4);
        v = dx * dy - 0.81f * dxy * dxy;
    }
    det_all[(int64_t)n * g.det_elems + L.off + e] = v;
}

// 3x3x3 non-maximum suppression (strictly greater than all 26 neighbours, response > threshold), then OpenCV's interpolateKeypoint:
// a quadratic fit in (x, y, scale) solved by Cramer's rule (fp64 on the fp32 system), rejected when the offset leaves the cell.
__device__ bool candidate(const float* __restrict__ det, const Geo& g, const MidLayer& M, int i, int j, float4* kp) {
    const float* mid = det + g.L[M.k].off;
    const int C = M.C;
    const float v0 = mid[(int64_t)i * C + j];
    if (!(v0 > HESSIAN_THRESHOLD)) return false;
    float N[3][9];
    for (int s = 0; s < 3; ++s) {
        const float* d = det + g.L[M.k - 1 + s].off;
        for (int dy = -1; dy <= 1; ++dy)
            for (int dx = -1; dx <= 1; ++dx) N[s][(dy + 1) * 3 + dx + 1] = d[(int64_t)(i + dy) * C + j + dx];
    }
    for (int s = 0; s < 3; ++s)
        for (int q = 0; q < 9; ++q)
            if (!(s == 1 && q == 4) && !(v0 > N[s][q])) return false;
    const float b0 = -(N[1][5] - N[1][3]) / 2.f, b1 = -(N[1][7] - N[1][1]) / 2.f, b2 = -(N[2][4] - N[0][4]) / 2.f;
    const float dxx = N[1][3] - 2.f * N[1][4] + N[1][5];
    const float dyy = N[1][1] - 2.f * N[1][4] + N[1][7];
    const float dss = N[0][4] - 2.f * N[1][4] + N[2][4];
    const float dxy = (N[1][8] - N[1][6] - N[1][2] + N[1][0]) / 4.f;
    const float dxs = (N[2][5] - N[2][3] - N[0][5] + N[0][3]) / 4.f;
    const float dys = (N[2][7] - N[2][1] - N[0][7] + N[0][1]) / 4.f;
    const double a00 = dxx, a01 = dxy, a02 = dxs, a10 = dxy, a11 = dyy, a12 = dys, a20 = dxs, a21 = dys, a22 = dss;
    const double B0 = b0, B1 = b1, B2 = b2;
    const double dt = a00 * (a11 * a22 - a12 * a21) - a01 * (a10 * a22 - a12 * a20) + a02 * (a10 * a21 - a11 * a20);
    const double inv = dt != 0 ? 1.0 / dt : 0.0;
    const float x0 = (float)((B0 * (a11 * a22 - a12 * a21) - a01 * (B1 * a22 - a12 * B2) + a02 * (B1 * a21 - a11 * B2)) * inv);
    const float x1 = (float)((a00 * (B1 * a22 - a12 * B2) - B0 * (a10 * a22 - a12 * a20) + a02 * (a10 * B2 - B1 * a20)) * inv);
    const float x2 = (float)((a00 * (a11 * B2 - B1 * a21) - a01 * (a10 * B2 - B1 * a20) + B0 * (a10 * a21 - a11 * a20)) * inv);
    if (!((x0 != 0 || x1 != 0 || x2 != 0) && fabsf(x0) <= 1 && fabsf(x1) <= 1 && fabsf(x2) <= 1)) return false;
    const float ci = (float)(M.step * (i - (M.size / 2) / M.step)) + (float)((M.size - 1) * 0.5);
    const float cj = (float)(M.step * (j - (M.size / 2) / M.step)) + (float)((M.size - 1) * 0.5);
    kp->x = cj + x0 * (float)M.step;
    kp->y = ci + x1 * (float)M.step;
    kp->z = rintf((float)M.size + x2 * (float)M.ds);
    kp->w = v0;
    return true;
}

// one wave per NMS row; WRITE = false counts the row's candidates, WRITE = true writes them at the row's scanned offset, in column order
template <bool WRITE>
__global__ void nms_kernel(const float* __restrict__ det_all, Geo g, int* __restrict__ row_cnt, const int* __restrict__ row_off,
                           float4* __restrict__ cand) {
    const int n = blockIdx.y, lane = threadIdx.x & 63;
    const int row = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    if (row >= g.rows) return;
    int m = 0;
    while (m + 1 < N_OCT * N_MID && row >= g.M[m + 1].row0) ++m;
    const MidLayer M = g.M[m];
    const int i = M.margin + row - M.row0;
    const float* det = det_all + (int64_t)n * g.det_elems;
    int base = WRITE ? row_off[(int64_t)n * (g.rows + 1) + row] : 0;
    for (int j0 = M.margin; j0 < M.C - M.margin; j0 += 64) {
        const int j = j0 + lane;
        float4 kp;
        const bool ok = j < M.C - M.margin && candidate(det, g, M, i, j, &kp);
        const uint64_t bal = __ballot(ok);
        if (WRITE && ok) cand[(int64_t)n * g.cand_cap + base + __popcll(bal & ((1ull << lane) - 1))] = kp;
        base += __popcll(bal);
    }
    if (!WRITE && lane == 0) row_cnt[(int64_t)n * (g.rows + 1) + row] = base;
}

// exclusive scan of the per-row counts of one image (1024 threads, chunks of 1024 rows), the total into ncand[n]
__global__ void scan_rows_kernel(const int* __restrict__ row_cnt, int rows, int* __restrict__ row_off, int* __restrict__ ncand) {
    __shared__ int s[1024];
    const int n = blockIdx.x, t = threadIdx.x;
    int carry = 0;
    for (int c0 = 0; c0 < rows; c0 += 1024) {
        const int v = c0 + t < rows ? row_cnt[(int64_t)n * (rows + 1) + c0 + t] : 0;
        s[t] = v;
        __syncthreads();
        for (int d = 1; d < 1024; d <<= 1) {
            const int u = t >= d ? s[t - d] : 0;
            __syncthreads();
            s[t] += u;
            __syncthreads();
        }
        if (c0 + t < rows) row_off[(int64_t)n * (rows + 1) + c0 + t] = carry + s[t] - v;
        carry += s[1023];
        __syncthreads();
    }
    if (t == 0) ncand[n] = carry;
}

// exclusive prefix of a 0/1 flag over a 1024-thread block (16 waves), and the block total; order = thread order
__device__ int block_flag_scan(bool f, int* wsum, int* total) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const uint64_t bal = __ballot(f);
    if (lane == 0) wsum[w] = __popcll(bal);
    __syncthreads();
    int before = 0, all = 0;
    for (int k = 0; k < 16; ++k) {
        before += k < w ? wsum[k] : 0;
        all += wsum[k];
    }
    __syncthreads();
    *total = all;
    return before + __popcll(bal & ((1ull << lane) - 1));
}

// the strongest max_kp candidates of image n (response descending, ties to the earlier candidate), written in generation order.
// Responses are > 100, so their fp32 bit patterns order like their values: a 4-pass 8-bit radix select finds the max_kp-th largest.
__global__ void select_kernel(const float4* __restrict__ cand_all, const int* __restrict__ ncand, int cap, int max_kp,
                              float4* __restrict__ kp_out, int* __restrict__ n_kp) {
    __shared__ int hist[256];
    __shared__ int wsum[16];
    __shared__ uint32_t s_prefix;
    __shared__ int s_rem;
    const int n = blockIdx.x, t = threadIdx.x;
    const int cnt = ncand[n];
    const float4* cand = cand_all + (int64_t)n * cap;
    uint32_t T = 0;
    int rem = max_kp;
    if (cnt > max_kp) {
        if (t == 0) { s_prefix = 0; s_rem = max_kp; }
        for (int pass = 0; pass < 4; ++pass) {
            const int shift = 24 - 8 * pass;
            const uint32_t hmask = pass ? 0xFFFFFFFFu << (shift + 8) : 0u;
            if (t < 256) hist[t] = 0;
            __syncthreads();
            const uint32_t prefix = s_prefix;
            for (int i = t; i < cnt; i += blockDim.x) {
                const uint32_t b = __float_as_uint(cand[i].w);
                if ((b & hmask) == prefix) atomicAdd(&hist[(b >> shift) & 255], 1);
            }
            __syncthreads();
            if (t == 0) {
                int r = s_rem, bin = 255;
                for (; bin > 0 && hist[bin] < r; --bin) r -= hist[bin];
                s_prefix = prefix | ((uint32_t)bin << shift);
                s_rem = r;
            }
            __syncthreads();
        }
        T = s_prefix;
        rem = s_rem;                   // items > T: max_kp - rem; keep the first rem items equal to T
    }
    int kept = 0, eq = 0;
    for (int c0 = 0; c0 < cnt; c0 += blockDim.x) {
        const int i = c0 + t;
        float4 v = make_float4(0, 0, 0, 0);
        uint32_t b = 0;
        if (i < cnt) { v = cand[i]; b = __float_as_uint(v.w); }
        int eq_tot;
        const bool is_eq = i < cnt && cnt > max_kp && b == T;
        const int eq_rank = eq + block_flag_scan(is_eq, wsum, &eq_tot);
        const bool keep = i < cnt && (cnt <= max_kp || b > T || (is_eq && eq_rank < rem));
        int keep_tot;
        const int pos = kept + block_flag_scan(keep, wsum, &keep_tot);
        if (keep) kp_out[(int64_t)n * max_kp + pos] = v;
        kept += keep_tot;
        eq += eq_tot;
    }
    if (t == 0) n_kp[n] = kept;
}

// ------------------------------------------------------------------------------------------------ 3. U-SURF descriptor
// 20 x 20 samples spaced s = 1.2 size / 9 around the keypoint, Haar responses of size 2 round(s) on the integral image (boxes clamped
// to the image), Gaussian weights sigma = 3.3 s, (sum dx, sum |dx|, sum dy, sum |dy|) of each 5 x 5 sub-region, L2-normalised.
__device__ __forceinline__ int64_t box_sum(const int* I, int H, int W, int y0, int y1, int x0, int x1) {
    y0 = min(max(y0, 0), H); y1 = min(max(y1, 0), H); x0 = min(max(x0, 0), W); x1 = min(max(x1, 0), W);
    const int ld = W + 1;
    return (int64_t)I[(int64_t)y1 * ld + x1] - I[(int64_t)y0 * ld + x1] - I[(int64_t)y1 * ld + x0] + I[(int64_t)y0 * ld + x0];
}

__global__ void __launch_bounds__(64) describe_kernel(const int* __restrict__ Iall, int H, int W, const float4* __restrict__ kp_all,
                                                      const int* __restrict__ n_kp, int max_kp, float* __restrict__ desc_all,
                                                      float* __restrict__ nrm_all) {
    __shared__ float sdx[400], sdy[400], comp[64];
    const int k = blockIdx.x, n = blockIdx.y, lane = threadIdx.x;
    if (k >= n_kp[n]) return;
    const int* I = Iall + (int64_t)n * (H + 1) * (W + 1);
    const float4 kp = kp_all[(int64_t)n * max_kp + k];
    const float s = kp.z * 1.2f / 9.f;
    const int hs = max(1, (int)rintf(s));
    for (int q = lane; q < 400; q += 64) {
        const int v = q / 20, u = q % 20;
        const int px = (int)rintf(kp.x + ((float)u - 9.5f) * s);
        const int py = (int)rintf(kp.y + ((float)v - 9.5f) * s);
        const float dx = (float)(box_sum(I, H, W, py - hs, py + hs, px, px + hs) - box_sum(I, H, W, py - hs, py + hs, px - hs, px));
        const float dy = (float)(box_sum(I, H, W, py, py + hs, px - hs, px + hs) - box_sum(I, H, W, py - hs, py, px - hs, px + hs));
        const double du = u - 9.5, dv = v - 9.5;
        const float gw = (float)exp(-(du * du + dv * dv) / (2.0 * 3.3 * 3.3));
        sdx[q] = gw * dx;
        sdy[q] = gw * dy;
    }
    __syncthreads();
    {
        const int sub = lane >> 2, kind = lane & 3, sy = sub >> 2, sx = sub & 3;
        const float* src = kind < 2 ? sdx : sdy;
        float acc = 0.f;
        for (int vv = 0; vv < 5; ++vv)
            for (int uu = 0; uu < 5; ++uu) {
                const float a = src[(sy * 5 + vv) * 20 + sx * 5 + uu];
                acc += (kind & 1) ? fabsf(a) : a;
            }
        comp[lane] = acc;
    }
    __syncthreads();
    float ss = 0.f;
    for (int c = 0; c < 64; ++c) ss = ss + comp[c] * comp[c];
    const float nrm = sqrtf(ss);
    const float d = nrm > 0 ? comp[lane] / nrm : 0.f;
    desc_all[((int64_t)n * max_kp + k) * 64 + lane] = d;
    __syncthreads();
    comp[lane] = d;
    __syncthreads();
    if (lane == 0) {
        float acc = 0.f;
        for (int c = 0; c < 64; ++c) acc = fmaf(comp[c], comp[c], acc);
        nrm_all[(int64_t)n * max_kp + k] = acc;
    }
}

// ------------------------------------------------------------------------------------------------ 3b. oriented / extended SURF
// Orientation (OpenCV SURF's SURFInvoker): Haar responses of size g = 2 round(2 s) at the 109 grid points (i, j), i^2 + j^2 < 36,
// spaced s around the keypoint, each weighted by G[i + 6] G[j + 6] (13-tap Gaussian, sigma 2.5); the 60-degree window, slid in
// steps of 5 degrees, whose summed response is longest gives the direction.  Angles come from OpenCV's fastAtan2 polynomial in
// fp32 so that the restatement reproduces them bit for bit.
constexpr int ORI_SAMPLES = 109, ORI_WINDOWS = 72;

struct OriTable {
    float w[ORI_SAMPLES];                                   // G[i + 6] * G[j + 6] in fp32
    signed char i[ORI_SAMPLES], j[ORI_SAMPLES];             // row-major: i outer, j inner
};

OriTable ori_table() {
    double g[13], sum = 0;
    for (int k = 0; k < 13; ++k) {
        g[k] = std::exp(-(double)((k - 6) * (k - 6)) / (2.0 * 2.5 * 2.5));
        sum += g[k];
    }
    float G[13];
    for (int k = 0; k < 13; ++k) G[k] = (float)(g[k] / sum);
    OriTable t{};
    int q = 0;
    for (int i = -6; i <= 6; ++i)
        for (int j = -6; j <= 6; ++j)
            if (i * i + j * j < 36) {
                t.w[q] = G[i + 6] * G[j + 6];
                t.i[q] = (signed char)i;
                t.j[q] = (signed char)j;
                ++q;
            }
    return t;
}

// OpenCV's fastAtan2 (degrees in [0, 360]), every step in fp32
__device__ __forceinline__ float fast_atan2_deg(float y, float x) {
    constexpr float R2D = (float)(180.0 / 3.14159265358979323846);
    constexpr float P1 = 0.9997878412794807f * R2D, P3 = -0.3258083974640975f * R2D, P5 = 0.1555786518463281f * R2D,
                    P7 = -0.04432655554792128f * R2D;
    constexpr float EPS = (float)2.220446049250313080847e-16;   // (float)DBL_EPSILON
    const float ax = fabsf(x), ay = fabsf(y);
    float a;
    if (ax >= ay) {
        const float c = ay / (ax + EPS), c2 = c * c;
        a = (((P7 * c2 + P5) * c2 + P3) * c2 + P1) * c;
    } else {
        const float c = ax / (ay + EPS), c2 = c * c;
        a = 90.f - (((P7 * c2 + P5) * c2 + P3) * c2 + P1) * c;
    }
    if (x < 0) a = 180.f - a;
    if (y < 0) a = 360.f - a;
    return a;
}

// one wave per keypoint: lanes take samples q and q + 64, then windows w and w + 64; lane 0 keeps the first longest window.
// Out: (cos, sin) of the direction, (1, 0) when no window sums to a non-zero response.
__global__ void __launch_bounds__(64) orient_kernel(const int* __restrict__ Iall, int H, int W, const float4* __restrict__ kp_all,
                                                    const int* __restrict__ n_kp, int max_kp, OriTable tab, float2* __restrict__ ori_all) {
    __shared__ float sX[ORI_SAMPLES], sY[ORI_SAMPLES], wmod[ORI_WINDOWS], wx[ORI_WINDOWS], wy[ORI_WINDOWS];
    __shared__ int sA[ORI_SAMPLES];
    const int k = blockIdx.x, n = blockIdx.y, lane = threadIdx.x;
    if (k >= n_kp[n]) return;
    const int* I = Iall + (int64_t)n * (H + 1) * (W + 1);
    const float4 kp = kp_all[(int64_t)n * max_kp + k];
    const float s = kp.z * 1.2f / 9.f;
    const int g = 2 * (int)rintf(2.f * s), h = g / 2;
    const float half = (float)(g - 1) / 2.f;
    for (int q = lane; q < ORI_SAMPLES; q += 64) {
        const int x0 = (int)rintf(kp.x + (float)tab.i[q] * s - half);
        const int y0 = (int)rintf(kp.y + (float)tab.j[q] * s - half);
        float X = 0.f, Y = 0.f;
        int ang = -1;                                       // -1: the box leaves the image, the sample is skipped
        if (x0 >= 0 && y0 >= 0 && x0 + g <= W && y0 + g <= H) {
            const int64_t gx = box_sum(I, H, W, y0, y0 + g, x0 + h, x0 + g) - box_sum(I, H, W, y0, y0 + g, x0, x0 + h);
            const int64_t gy = box_sum(I, H, W, y0 + h, y0 + g, x0, x0 + g) - box_sum(I, H, W, y0, y0 + h, x0, x0 + g);
            X = (float)gx * tab.w[q];
            Y = (float)gy * tab.w[q];
            ang = (int)rintf(fast_atan2_deg(Y, X));
        }
        sX[q] = X;
        sY[q] = Y;
        sA[q] = ang;
    }
    __syncthreads();
    for (int w = lane; w < ORI_WINDOWS; w += 64) {
        const int w0 = 5 * w;
        float sx = 0.f, sy = 0.f;
        for (int q = 0; q < ORI_SAMPLES; ++q) {
            const int d = abs(sA[q] - w0);
            if (sA[q] >= 0 && (d < 30 || d > 330)) {
                sx += sX[q];
                sy += sY[q];
            }
        }
        wmod[w] = sx * sx + sy * sy;
        wx[w] = sx;
        wy[w] = sy;
    }
    __syncthreads();
    if (lane == 0) {
        float best = 0.f, bx = 0.f, by = 0.f;
        for (int w = 0; w < ORI_WINDOWS; ++w)
            if (wmod[w] > best) { best = wmod[w]; bx = wx[w]; by = wy[w]; }
        float2 o = make_float2(1.f, 0.f);
        if (best > 0.f) {
            const float r = sqrtf(bx * bx + by * by);
            o = make_float2(bx / r, by / r);
        }
        ori_all[(int64_t)n * max_kp + k] = o;
    }
}

// describe_kernel in the keypoint's frame (ori = nullptr: upright) with D = 64 or 128 components.  The sample (u, v) sits at
// kp + s R(phi) (u - 9.5, v - 9.5); its axis-aligned Haar responses are rotated into the frame, dx' = c dx + s dy, dy' = -s dx + c dy.
// With (c, s) = (1, 0) every product by 0 vanishes exactly and D = 64 gives describe_kernel's bits.  D = 128 splits each sum by the
// sign of the other response, in OpenCV's order: dx, |dx| over dy >= 0; dx, |dx| over dy < 0; dy, |dy| over dx >= 0; dy, |dy| over dx < 0.
template <int D>
__global__ void __launch_bounds__(64) describe_ex_kernel(const int* __restrict__ Iall, int H, int W, const float4* __restrict__ kp_all,
                                                         const float2* __restrict__ ori_all, const int* __restrict__ n_kp, int max_kp,
                                                         float* __restrict__ desc_all, float* __restrict__ nrm_all) {
    static_assert(D == 64 || D == 128, "64- or 128-d SURF");
    __shared__ float sdx[400], sdy[400], comp[D];
    const int k = blockIdx.x, n = blockIdx.y, lane = threadIdx.x;
    if (k >= n_kp[n]) return;
    const int* I = Iall + (int64_t)n * (H + 1) * (W + 1);
    const float4 kp = kp_all[(int64_t)n * max_kp + k];
    float c = 1.f, sn = 0.f;
    if (ori_all) {
        const float2 o = ori_all[(int64_t)n * max_kp + k];
        c = o.x;
        sn = o.y;
    }
    const float s = kp.z * 1.2f / 9.f;
    const int hs = max(1, (int)rintf(s));
    for (int q = lane; q < 400; q += 64) {
        const int v = q / 20, u = q % 20;
        const float fu = (float)u - 9.5f, fv = (float)v - 9.5f;
        const int px = (int)rintf(kp.x + (fu * c - fv * sn) * s);
        const int py = (int)rintf(kp.y + (fu * sn + fv * c) * s);
        const float dx = (float)(box_sum(I, H, W, py - hs, py + hs, px, px + hs) - box_sum(I, H, W, py - hs, py + hs, px - hs, px));
        const float dy = (float)(box_sum(I, H, W, py, py + hs, px - hs, px + hs) - box_sum(I, H, W, py - hs, py, px - hs, px + hs));
        const float rx = c * dx + sn * dy, ry = -sn * dx + c * dy;
        const double du = u - 9.5, dv = v - 9.5;
        const float gw = (float)exp(-(du * du + dv * dv) / (2.0 * 3.3 * 3.3));
        sdx[q] = gw * rx;
        sdy[q] = gw * ry;
    }
    __syncthreads();
    for (int cc = lane; cc < D; cc += 64) {
        const int per = D / 16, sub = cc / per, kind = cc % per, sy = sub >> 2, sx = sub & 3;
        const float* src = (D == 64 ? kind < 2 : kind < 4) ? sdx : sdy;
        const float* oth = src == sdx ? sdy : sdx;
        const bool neg = D == 128 && (kind & 2), absv = kind & 1;
        float acc = 0.f;
        for (int vv = 0; vv < 5; ++vv)
            for (int uu = 0; uu < 5; ++uu) {
                const int i = (sy * 5 + vv) * 20 + sx * 5 + uu;
                const float a = src[i];
                if (D == 64 || (oth[i] < 0.f) == neg) acc += absv ? fabsf(a) : a;
            }
        comp[cc] = acc;
    }
    __syncthreads();
    float ss = 0.f;
    for (int cc = 0; cc < D; ++cc) ss = ss + comp[cc] * comp[cc];
    const float nrm = sqrtf(ss);
    float d[D / 64];
    for (int r = 0; r < D / 64; ++r) {
        d[r] = nrm > 0 ? comp[lane + 64 * r] / nrm : 0.f;
        desc_all[((int64_t)n * max_kp + k) * D + lane + 64 * r] = d[r];
    }
    __syncthreads();
    for (int r = 0; r < D / 64; ++r) comp[lane + 64 * r] = d[r];
    __syncthreads();
    if (lane == 0) {
        float acc = 0.f;
        for (int cc = 0; cc < D; ++cc) acc = fmaf(comp[cc], comp[cc], acc);
        nrm_all[(int64_t)n * max_kp + k] = acc;
    }
}

// ------------------------------------------------------------------------------------------------ 4. matching
// d^2(q, t) = (|a|^2 + |b|^2) - 2 a.b: a.b on v_mfma_f32_16x16x4_f32 (exact fp32 products, k-ordered accumulation), one wave per
// 16 queries sweeping the whole train set in tiles of 16; each lane keeps the top-2 (distance, then index) of its 4 query rows over
// its train column, the 16 columns merge by butterfly.  The distance matrix never leaves registers.  D: descriptor width (64 / 128).
__device__ __forceinline__ bool lessdi(float a, int i, float b, int j) { return a < b || (a == b && i < j); }

template <int D>
__global__ void __launch_bounds__(256) match_kernel(const float* __restrict__ desc_all, const float* __restrict__ nrm_all,
                                                    const int* __restrict__ n_kp, int B, int max_kp, int* __restrict__ best_t) {
    const int b = blockIdx.y, lane = threadIdx.x & 63;
    const int q0 = (blockIdx.x * 4 + (threadIdx.x >> 6)) * 16;
    const int n1 = n_kp[b], n2 = n_kp[B + b];
    if (q0 >= n1) return;
    const float* d1 = desc_all + (int64_t)b * max_kp * D;
    const float* d2 = desc_all + (int64_t)(B + b) * max_kp * D;
    const int r16 = lane & 15, kq = lane >> 4;
    float a[D / 4];
    const int qa = q0 + r16;
    for (int kk = 0; kk < D / 4; ++kk) a[kk] = qa < n1 ? d1[(int64_t)qa * D + 4 * kk + kq] : 0.f;
    float na[4], bd1[4], bd2[4];
    int bi1[4], bi2[4];
    for (int r = 0; r < 4; ++r) {
        const int q = q0 + 4 * kq + r;
        na[r] = q < n1 ? nrm_all[(int64_t)b * max_kp + q] : 0.f;
        bd1[r] = bd2[r] = INFINITY;
        bi1[r] = bi2[r] = 0x7FFFFFFF;
    }
    for (int t0 = 0; t0 < n2; t0 += 16) {
        const int tb = t0 + r16;
        f32x4 acc = {0.f, 0.f, 0.f, 0.f};
        for (int kk = 0; kk < D / 4; ++kk) {
            const float bv = tb < n2 ? d2[(int64_t)tb * D + 4 * kk + kq] : 0.f;
            acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a[kk], bv, acc, 0, 0, 0);
        }
        if (tb < n2) {
            const float nb = nrm_all[(int64_t)(B + b) * max_kp + tb];
            for (int r = 0; r < 4; ++r) {
                const float d = (na[r] + nb) - 2.f * acc[r];
                if (lessdi(d, tb, bd1[r], bi1[r])) {
                    bd2[r] = bd1[r]; bi2[r] = bi1[r]; bd1[r] = d; bi1[r] = tb;
                } else if (lessdi(d, tb, bd2[r], bi2[r])) {
                    bd2[r] = d; bi2[r] = tb;
                }
            }
        }
    }
    for (int off = 1; off < 16; off <<= 1)
        for (int r = 0; r < 4; ++r) {
            const float od1 = __shfl_xor(bd1[r], off), od2 = __shfl_xor(bd2[r], off);
            const int oi1 = __shfl_xor(bi1[r], off), oi2 = __shfl_xor(bi2[r], off);
            if (lessdi(od1, oi1, bd1[r], bi1[r])) {
                const bool k2 = lessdi(bd1[r], bi1[r], od2, oi2);
                bd2[r] = k2 ? bd1[r] : od2; bi2[r] = k2 ? bi1[r] : oi2;
                bd1[r] = od1; bi1[r] = oi1;
            } else if (lessdi(od1, oi1, bd2[r], bi2[r])) {
                bd2[r] = od1; bi2[r] = oi1;
            }
        }
    if (r16 == 0)
        for (int r = 0; r < 4; ++r) {
            const int q = q0 + 4 * kq + r;
            if (q < n1) best_t[(int64_t)b * max_kp + q] = (n2 >= 2 && bd1[r] < 0.49f * bd2[r]) ? bi1[r] : -1;
        }
}

__global__ void compact_matches_kernel(const int* __restrict__ best_t, const int* __restrict__ n_kp, int max_kp, int2* __restrict__ matches,
                                       int* __restrict__ n_match) {
    __shared__ int wsum[16];
    const int b = blockIdx.x, t = threadIdx.x;
    const int n1 = n_kp[b];
    int kept = 0;
    for (int c0 = 0; c0 < n1; c0 += blockDim.x) {
        const int q = c0 + t;
        const int tr = q < n1 ? best_t[(int64_t)b * max_kp + q] : -1;
        int tot;
        const int pos = kept + block_flag_scan(tr >= 0, wsum, &tot);
        if (tr >= 0) matches[(int64_t)b * max_kp + pos] = make_int2(q, tr);
        kept += tot;
    }
    if (t == 0) n_match[b] = kept;
}

// ------------------------------------------------------------------------------------------------ 5. RANSAC
__device__ __forceinline__ uint32_t mix32(uint32_t x) {
    x ^= x >> 16; x *= 0x7FEB352Du; x ^= x >> 15; x *= 0x846CA68Bu; x ^= x >> 16;
    return x;
}
__device__ __forceinline__ uint32_t hash4(uint32_t seed, uint32_t pair, uint32_t hyp, uint32_t draw) {
    return mix32(mix32(mix32(mix32(seed) ^ pair) ^ hyp) ^ draw);
}

__device__ bool collinear(const double* x, const double* y) {
    const int tri[4][3] = {{0, 1, 2}, {0, 1, 3}, {0, 2, 3}, {1, 2, 3}};
    for (int q = 0; q < 4; ++q) {
        const int i = tri[q][0], j = tri[q][1], k = tri[q][2];
        const double dx1 = x[j] - x[i], dy1 = y[j] - y[i], dx2 = x[k] - x[i], dy2 = y[k] - y[i];
        if (fabs(dx2 * dy1 - dy2 * dx1) <= 1.1920928955078125e-07 /* FLT_EPSILON */ * (fabs(dx1) + fabs(dy1) + fabs(dx2) + fabs(dy2))) return true;
    }
    return false;
}

__device__ __forceinline__ double orient(const double* x, const double* y, int i, int j, int k) {
    return (x[j] - x[i]) * (y[k] - y[i]) - (y[j] - y[i]) * (x[k] - x[i]);
}

__device__ bool hartley(const double* x, const double* y, double* cx, double* cy, double* sc) {
    *cx = ((x[0] + x[1]) + x[2] + x[3]) / 4.0;
    *cy = ((y[0] + y[1]) + y[2] + y[3]) / 4.0;
    double md = 0;
    for (int i = 0; i < 4; ++i) md = md + sqrt((x[i] - *cx) * (x[i] - *cx) + (y[i] - *cy) * (y[i] - *cy));
    md = md / 4.0;
    if (!(md > 0)) return false;
    *sc = sqrt(2.0) / md;
    return true;
}

// 4-point DLT, h33 = 1: Gaussian elimination with partial pivoting on the 8 x 9 system (fp64)
__device__ bool dlt4(const double* sx, const double* sy, const double* dx, const double* dy, double* h) {
    double A[8][9];
    for (int i = 0; i < 4; ++i) {
        const double x = sx[i], y = sy[i], u = dx[i], v = dy[i];
        double* r0 = A[2 * i];
        double* r1 = A[2 * i + 1];
        r0[0] = x; r0[1] = y; r0[2] = 1; r0[3] = 0; r0[4] = 0; r0[5] = 0; r0[6] = -x * u; r0[7] = -y * u; r0[8] = u;
        r1[0] = 0; r1[1] = 0; r1[2] = 0; r1[3] = x; r1[4] = y; r1[5] = 1; r1[6] = -x * v; r1[7] = -y * v; r1[8] = v;
    }
    for (int c = 0; c < 8; ++c) {
        int piv = c;
        for (int r = c + 1; r < 8; ++r)
            if (fabs(A[r][c]) > fabs(A[piv][c])) piv = r;
        if (fabs(A[piv][c]) < 1e-300) return false;
        if (piv != c)
            for (int k = 0; k < 9; ++k) { const double t = A[c][k]; A[c][k] = A[piv][k]; A[piv][k] = t; }
        const double inv = 1.0 / A[c][c];
        for (int r = c + 1; r < 8; ++r) {
            const double f = A[r][c] * inv;
            for (int k = c; k < 9; ++k) A[r][k] = A[r][k] - f * A[c][k];
        }
    }
    for (int c = 7; c >= 0; --c) {
        double s = A[c][8];
        for (int k = c + 1; k < 8; ++k) s = s - A[c][k] * h[k];
        h[c] = s / A[c][c];
    }
    h[8] = 1.0;
    return true;
}

__device__ void mul3(const double* a, const double* b, double* o) {
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) o[3 * i + j] = a[3 * i] * b[j] + a[3 * i + 1] * b[3 + j] + a[3 * i + 2] * b[6 + j];
}

// H from 4 correspondences: OpenCV's subset check (no collinear triple in either view, consistent orientation of the 4 triangles),
// Hartley normalisation, DLT, denormalisation, h33 = 1.  fp32 result for the scoring loop.
__device__ bool hypothesis(const float4* p, float* hf) {
    double sx[4], sy[4], dx[4], dy[4];
    for (int i = 0; i < 4; ++i) { sx[i] = p[i].x; sy[i] = p[i].y; dx[i] = p[i].z; dy[i] = p[i].w; }
    if (collinear(sx, sy) || collinear(dx, dy)) return false;
    const int tt[4][3] = {{0, 1, 2}, {1, 2, 3}, {0, 2, 3}, {0, 1, 3}};
    int neg = 0;
    for (int q = 0; q < 4; ++q) neg += orient(sx, sy, tt[q][0], tt[q][1], tt[q][2]) * orient(dx, dy, tt[q][0], tt[q][1], tt[q][2]) < 0;
    if (neg != 0 && neg != 4) return false;
    double c1x, c1y, s1, c2x, c2y, s2;
    if (!hartley(sx, sy, &c1x, &c1y, &s1) || !hartley(dx, dy, &c2x, &c2y, &s2)) return false;
    double nsx[4], nsy[4], ndx[4], ndy[4], hn[9];
    for (int i = 0; i < 4; ++i) {
        nsx[i] = (sx[i] - c1x) * s1; nsy[i] = (sy[i] - c1y) * s1;
        ndx[i] = (dx[i] - c2x) * s2; ndy[i] = (dy[i] - c2y) * s2;
    }
    if (!dlt4(nsx, nsy, ndx, ndy, hn)) return false;
    const double T1[9] = {s1, 0, -s1 * c1x, 0, s1, -s1 * c1y, 0, 0, 1};
    const double T2i[9] = {1.0 / s2, 0, c2x, 0, 1.0 / s2, c2y, 0, 0, 1};
    double t[9], Hm[9];
    mul3(hn, T1, t);
    mul3(T2i, t, Hm);
    if (!(fabs(Hm[8]) > 1e-12)) return false;
    const double h8 = Hm[8];
    for (int k = 0; k < 9; ++k) hf[k] = (float)(Hm[k] / h8);
    return true;
}

__device__ __forceinline__ float reproj(const float* h, float4 p) {
    const float u = h[0] * p.x + h[1] * p.y + h[2];
    const float v = h[3] * p.x + h[4] * p.y + h[5];
    const float w = h[6] * p.x + h[7] * p.y + h[8];
    const float ex = u / w - p.z, ey = v / w - p.w;
    return ex * ex + ey * ey;
}

__device__ __forceinline__ float4 match_points(const float4* kp_all, const int2* matches, int B, int b, int max_kp, int i) {
    const int2 m = matches[(int64_t)b * max_kp + i];
    const float4 a = kp_all[(int64_t)b * max_kp + m.x], c = kp_all[(int64_t)(B + b) * max_kp + m.y];
    return make_float4(a.x, a.y, c.x, c.y);
}

__global__ void __launch_bounds__(64) ransac_kernel(const float4* __restrict__ kp_all, const int2* __restrict__ matches,
                                                     const int* __restrict__ n_match, int B, int max_kp, int n_hyp, uint32_t seed,
                                                     const uint32_t* __restrict__ pair_ids, int* __restrict__ hyp_cnt, float* __restrict__ hyp_esum,
                                                     float* __restrict__ hyp_H) {
    extern __shared__ float4 pts[];
    const int b = blockIdx.y, t = threadIdx.x;
    const int M = n_match[b];
    for (int i = t; i < M; i += blockDim.x) pts[i] = match_points(kp_all, matches, B, b, max_kp, i);
    __syncthreads();
    const int h = blockIdx.x * blockDim.x + t;
    if (h >= n_hyp) return;
    int cnt = -1;
    float esum = 0.f, hf[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    if (M >= 4) {
        int idx[4], got = 0;
        for (int c = 0; c < MAX_DRAWS && got < 4; ++c) {
            const int v = (int)(hash4(seed, pair_ids[b], (uint32_t)h, (uint32_t)c) % (uint32_t)M);
            bool fresh = true;
            for (int q = 0; q < got; ++q) fresh &= idx[q] != v;
            if (fresh) idx[got++] = v;
        }
        float4 p[4];
        for (int q = 0; q < 4; ++q) p[q] = pts[q < got ? idx[q] : 0];
        if (got == 4 && hypothesis(p, hf)) {
            cnt = 0;
            for (int i = 0; i < M; ++i) {
                const float e = reproj(hf, pts[i]);
                cnt += e <= 25.f;
                esum += fminf(e, 25.f);
            }
        }
    }
    const int64_t o = (int64_t)b * n_hyp + h;
    hyp_cnt[o] = cnt;
    hyp_esum[o] = cnt >= 0 ? esum : 0.f;
    for (int k = 0; k < 9; ++k) hyp_H[o * 9 + k] = hf[k];
}

// ------------------------------------------------------------------------------------------------ 6. best hypothesis + refit
__device__ __forceinline__ bool better(int c, float e, int h, int c2, float e2, int h2) {
    return c > c2 || (c == c2 && (e < e2 || (e == e2 && h < h2)));
}

// block-wide fixed-order sum of NV doubles per thread (butterfly within each wave, then the 4 waves in order); every thread gets the sums
template <int NV>
__device__ void block_sum(double* v, double* red) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    for (int k = 0; k < NV; ++k) {
        double x = v[k];
        for (int off = 32; off > 0; off >>= 1) x = x + __shfl_xor(x, off);
        v[k] = x;
    }
    if (lane == 0)
        for (int k = 0; k < NV; ++k) red[w * NV + k] = v[k];
    __syncthreads();
    for (int k = 0; k < NV; ++k) v[k] = ((red[k] + red[NV + k]) + red[2 * NV + k]) + red[3 * NV + k];
    __syncthreads();
}

// Gaussian elimination with partial pivoting, n x (n + 1) augmented row-major (fp64); false on a zero pivot
__device__ bool solve_aug(double* A, int n, double* x) {
    for (int c = 0; c < n; ++c) {
        int p = c;
        for (int r = c + 1; r < n; ++r)
            if (fabs(A[r * (n + 1) + c]) > fabs(A[p * (n + 1) + c])) p = r;
        if (!(fabs(A[p * (n + 1) + c]) > 0)) return false;
        if (p != c)
            for (int k = 0; k <= n; ++k) { const double t = A[c * (n + 1) + k]; A[c * (n + 1) + k] = A[p * (n + 1) + k]; A[p * (n + 1) + k] = t; }
        for (int r = c + 1; r < n; ++r) {
            const double f = A[r * (n + 1) + c] / A[c * (n + 1) + c];
            for (int k = c; k <= n; ++k) A[r * (n + 1) + k] = A[r * (n + 1) + k] - f * A[c * (n + 1) + k];
        }
    }
    for (int c = n - 1; c >= 0; --c) {
        double s = A[c * (n + 1) + n];
        for (int k = c + 1; k < n; ++k) s = s - A[c * (n + 1) + k] * x[k];
        x[c] = s / A[c * (n + 1) + c];
    }
    return true;
}

// residuals and Jacobian rows (h33 = 1) of one normalised correspondence; accumulates J^T J (upper triangle, 36), J^T r (8), r^T r
__device__ __forceinline__ void lm_accum(const double* h, double x, double y, double u, double v, double* acc, bool jac) {
    const double U = h[0] * x + h[1] * y + h[2], V = h[3] * x + h[4] * y + h[5], Wd = h[6] * x + h[7] * y + 1.0;
    const double ru = U / Wd - u, rv = V / Wd - v;
    acc[44] += ru * ru + rv * rv;
    if (!jac) return;
    const double iw = 1.0 / Wd;
    const double ju[8] = {x * iw, y * iw, iw, 0, 0, 0, -x * U * iw * iw, -y * U * iw * iw};
    const double jv[8] = {0, 0, 0, x * iw, y * iw, iw, -x * V * iw * iw, -y * V * iw * iw};
    int q = 0;
    for (int i = 0; i < 8; ++i) {
        for (int j = i; j < 8; ++j) acc[q++] += ju[i] * ju[j] + jv[i] * jv[j];
        acc[36 + i] += ju[i] * ru + jv[i] * rv;
    }
}

__global__ void __launch_bounds__(256) finish_kernel(const float4* __restrict__ kp_all, const int2* __restrict__ matches,
                                                     const int* __restrict__ n_match, int B, int max_kp, int n_hyp,
                                                     const int* __restrict__ hyp_cnt, const float* __restrict__ hyp_esum,
                                                     const float* __restrict__ hyp_H, float* __restrict__ H_out, int* __restrict__ valid,
                                                     int* __restrict__ inliers, int* __restrict__ best_out, uint8_t* __restrict__ mask) {
    __shared__ int s_c[256], s_h[256];
    __shared__ float s_e[256];
    __shared__ double red[4 * 45];
    __shared__ double s_h8[8];
    __shared__ int s_ok;
    const int b = blockIdx.x, t = threadIdx.x;
    const int M = n_match[b];
    int bc = -2, bh = 0x7FFFFFFF;
    float be = INFINITY;
    for (int h = t; h < n_hyp; h += blockDim.x) {
        const int c = hyp_cnt[(int64_t)b * n_hyp + h];
        const float e = hyp_esum[(int64_t)b * n_hyp + h];
        if (better(c, e, h, bc, be, bh)) { bc = c; be = e; bh = h; }
    }
    s_c[t] = bc; s_e[t] = be; s_h[t] = bh;
    __syncthreads();
    for (int st = 128; st > 0; st >>= 1) {
        if (t < st && better(s_c[t + st], s_e[t + st], s_h[t + st], s_c[t], s_e[t], s_h[t])) {
            s_c[t] = s_c[t + st]; s_e[t] = s_e[t + st]; s_h[t] = s_h[t + st];
        }
        __syncthreads();
    }
    const int best = s_h[0], bcnt = s_c[0];
    if (bcnt < 4) {
        for (int i = t; i < M; i += blockDim.x) mask[(int64_t)b * max_kp + i] = 0;
        if (t < 9) H_out[b * 9 + t] = 0.f;
        if (t == 0) { valid[b] = 0; inliers[b] = bcnt > 0 ? bcnt : 0; best_out[b] = bcnt >= 0 ? best : -1; }
        return;
    }
    float hf[9];
    for (int k = 0; k < 9; ++k) hf[k] = hyp_H[((int64_t)b * n_hyp + best) * 9 + k];
    // centroids of the inliers
    double acc[45];
    for (int k = 0; k < 5; ++k) acc[k] = 0;
    for (int i = t; i < M; i += blockDim.x) {
        const float4 p = match_points(kp_all, matches, B, b, max_kp, i);
        const bool in = reproj(hf, p) <= 25.f;
        mask[(int64_t)b * max_kp + i] = in;
        if (in) { acc[0] += 1; acc[1] += p.x; acc[2] += p.y; acc[3] += p.z; acc[4] += p.w; }
    }
    block_sum<5>(acc, red);
    const double cnt = acc[0], c1x = acc[1] / cnt, c1y = acc[2] / cnt, c2x = acc[3] / cnt, c2y = acc[4] / cnt;
    acc[0] = acc[1] = 0;
    for (int i = t; i < M; i += blockDim.x)
        if (mask[(int64_t)b * max_kp + i]) {
            const float4 p = match_points(kp_all, matches, B, b, max_kp, i);
            acc[0] += sqrt(((double)p.x - c1x) * ((double)p.x - c1x) + ((double)p.y - c1y) * ((double)p.y - c1y));
            acc[1] += sqrt(((double)p.z - c2x) * ((double)p.z - c2x) + ((double)p.w - c2y) * ((double)p.w - c2y));
        }
    block_sum<2>(acc, red);
    const double s1 = sqrt(2.0) / (acc[0] / cnt), s2 = sqrt(2.0) / (acc[1] / cnt);
    // least-squares DLT (h33 = 1) through the normal equations
    for (int k = 0; k < 45; ++k) acc[k] = 0;
    for (int i = t; i < M; i += blockDim.x)
        if (mask[(int64_t)b * max_kp + i]) {
            const float4 p = match_points(kp_all, matches, B, b, max_kp, i);
            const double x = (p.x - c1x) * s1, y = (p.y - c1y) * s1, u = (p.z - c2x) * s2, v = (p.w - c2y) * s2;
            const double ru[9] = {x, y, 1, 0, 0, 0, -x * u, -y * u, u}, rv[9] = {0, 0, 0, x, y, 1, -x * v, -y * v, v};
            int q = 0;
            for (int i2 = 0; i2 < 8; ++i2) {
                for (int j = i2; j < 8; ++j) acc[q++] += ru[i2] * ru[j] + rv[i2] * rv[j];
                acc[36 + i2] += ru[i2] * ru[8] + rv[i2] * rv[8];
            }
        }
    block_sum<44>(acc, red);
    double h[8];
    bool ok = true;
    {
        double A[8 * 9];
        int q = 0;
        for (int i = 0; i < 8; ++i) {
            for (int j = i; j < 8; ++j) { A[i * 9 + j] = acc[q]; A[j * 9 + i] = acc[q]; ++q; }
            A[i * 9 + 8] = acc[36 + i];
        }
        ok = solve_aug(A, 8, h);
    }
    // Levenberg-Marquardt on the reprojection error in the normalised frames (same minimiser as in pixels: the scale is a constant)
    double lam = 1e-3, cost = 0;
    for (int it = 0; it <= LM_ITERS && ok; ++it) {
        for (int k = 0; k < 45; ++k) acc[k] = 0;
        for (int i = t; i < M; i += blockDim.x)
            if (mask[(int64_t)b * max_kp + i]) {
                const float4 p = match_points(kp_all, matches, B, b, max_kp, i);
                lm_accum(it == 0 ? h : s_h8, (p.x - c1x) * s1, (p.y - c1y) * s1, (p.z - c2x) * s2, (p.w - c2y) * s2, acc, true);
            }
        block_sum<45>(acc, red);
        if (it > 0) {                                   // acc[44] is the cost of the candidate s_h8; accept or reject it
            if (acc[44] < cost) {
                for (int k = 0; k < 8; ++k) h[k] = s_h8[k];
                lam *= 0.1;
            } else {
                lam *= 10.0;
                // the Jacobian at the kept h is needed again: recompute it
                for (int k = 0; k < 45; ++k) acc[k] = 0;
                for (int i = t; i < M; i += blockDim.x)
                    if (mask[(int64_t)b * max_kp + i]) {
                        const float4 p = match_points(kp_all, matches, B, b, max_kp, i);
                        lm_accum(h, (p.x - c1x) * s1, (p.y - c1y) * s1, (p.z - c2x) * s2, (p.w - c2y) * s2, acc, true);
                    }
                block_sum<45>(acc, red);
            }
        }
        cost = acc[44];
        if (it == LM_ITERS) break;
        __syncthreads();                                // every thread has read s_h8 before it is overwritten
        if (t == 0) {
            double A[8 * 9], step[8];
            int q = 0;
            for (int i = 0; i < 8; ++i) {
                for (int j = i; j < 8; ++j) { A[i * 9 + j] = acc[q]; A[j * 9 + i] = acc[q]; ++q; }
                A[i * 9 + 8] = -acc[36 + i];
            }
            for (int i = 0; i < 8; ++i) A[i * 9 + i] = A[i * 9 + i] + lam * A[i * 9 + i];
            s_ok = solve_aug(A, 8, step);
            for (int k = 0; k < 8; ++k) s_h8[k] = h[k] + (s_ok ? step[k] : 0.0);
        }
        __syncthreads();
        if (!s_ok) break;
    }
    if (t == 0) {
        const double hn[9] = {h[0], h[1], h[2], h[3], h[4], h[5], h[6], h[7], 1.0};
        const double T1[9] = {s1, 0, -s1 * c1x, 0, s1, -s1 * c1y, 0, 0, 1};
        const double T2i[9] = {1.0 / s2, 0, c2x, 0, 1.0 / s2, c2y, 0, 0, 1};
        double tm[9], Hm[9];
        mul3(hn, T1, tm);
        mul3(T2i, tm, Hm);
        bool fin = ok && fabs(Hm[8]) > 1e-12;
        for (int k = 0; k < 9; ++k) fin = fin && isfinite(Hm[k] / Hm[8]);
        for (int k = 0; k < 9; ++k) H_out[b * 9 + k] = fin ? (float)(Hm[k] / Hm[8]) : 0.f;
        valid[b] = fin;
        inliers[b] = bcnt;
        best_out[b] = best;
    }
}

}  // namespace

// ------------------------------------------------------------------------------------------------ C ABI
#define WS_CHECK(need) HESIC_CHECK_ARG(ws && ws_bytes >= (need), "stereo_h: workspace of %zu bytes, %zu needed", ws_bytes, (size_t)(need))

extern "C" int64_t hesic_stereo_h_det_elems(int H, int W) {
    if (H <= 0 || W <= 0) return 0;
    return geometry(H, W).det_elems;
}

extern "C" size_t hesic_stereo_h_ws_bytes(int B, int H, int W, int max_kp, int n_hyp) {
    if (B <= 0 || H <= 0 || W <= 0 || max_kp <= 0 || n_hyp <= 0) return 0;
    return ws_layout(B, H, W, max_kp, n_hyp).total;
}

extern "C" int hesic_stereo_h_integral(const void* img, int is_f32, int64_t sb, int64_t sc, int64_t sy, int64_t sx, int N, int H, int W,
                                       int32_t* I, void* stream) {
    HESIC_CHECK_ARG(img && I && N > 0 && H > 0 && W > 0, "stereo_h_integral: bad arguments");
    HESIC_CHECK_ARG((int64_t)H * W * 255 < (int64_t)1 << 31, "stereo_h_integral: %d x %d image overflows the int32 integral", H, W);
    HESIC_CHECK_ARG(N <= 65535 && H <= 2147483647 / 2, "stereo_h_integral: too many images");
    hipLaunchKernelGGL(integral_rows_kernel, dim3(H, N), dim3(256), 0, (hipStream_t)stream, img, is_f32, sb, sc, sy, sx, H, W, (int*)I);
    hipLaunchKernelGGL(integral_cols_kernel, dim3((W + 1 + 255) / 256, N), dim3(256), 0, (hipStream_t)stream, H, W, N, (int*)I);
    HESIC_LAUNCH_RETURN("stereo_h_integral");
}

extern "C" int hesic_stereo_h_hessian(const int32_t* I, int N, int H, int W, float* det, void* stream) {
    HESIC_CHECK_ARG(I && det && N > 0 && N <= 65535 && H > 0 && W > 0, "stereo_h_hessian: bad arguments");
    const Geo g = geometry(H, W);
    const int64_t maxe = (int64_t)H * W;
    hipLaunchKernelGGL(hessian_kernel, dim3((unsigned)((maxe + 255) / 256), N_OCT * N_LAY, N), dim3(256), 0, (hipStream_t)stream,
                       (const int*)I, H, W, g, det);
    HESIC_LAUNCH_RETURN("stereo_h_hessian");
}

extern "C" int hesic_stereo_h_keypoints(const float* det, int B, int H, int W, int max_kp, int n_hyp, void* ws, size_t ws_bytes,
                                        float* kp, int32_t* n_kp, void* stream) {
    HESIC_CHECK_ARG(det && kp && n_kp && B > 0 && H > 0 && W > 0 && max_kp > 0 && max_kp <= HESIC_STEREO_H_MAX_KEYPOINTS && n_hyp > 0,
                    "stereo_h_keypoints: bad arguments");
    const WsLayout L = ws_layout(B, H, W, max_kp, n_hyp);
    WS_CHECK(L.total);
    const Geo g = geometry(H, W);
    const int N = 2 * B;
    char* w = (char*)ws;
    int* row_cnt = (int*)(w + L.row_cnt);
    int* row_off = (int*)(w + L.row_off);
    int* ncand = (int*)(w + L.ncand);
    float4* cand = (float4*)(w + L.cand);
    hipStream_t s = (hipStream_t)stream;
    const int rb = (g.rows + 3) / 4;
    if (g.rows > 0) {
        hipLaunchKernelGGL(nms_kernel<false>, dim3(rb, N), dim3(256), 0, s, det, g, row_cnt, row_off, cand);
        hipLaunchKernelGGL(scan_rows_kernel, dim3(N), dim3(1024), 0, s, row_cnt, g.rows, row_off, ncand);
        hipLaunchKernelGGL(nms_kernel<true>, dim3(rb, N), dim3(256), 0, s, det, g, row_cnt, row_off, cand);
    } else {
        const hipError_t e = hipMemsetAsync(ncand, 0, sizeof(int) * N, s);
        if (e != hipSuccess) { hesic_set_error("stereo_h_keypoints: %s", hipGetErrorString(e)); return (int)e; }
    }
    hipLaunchKernelGGL(select_kernel, dim3(N), dim3(1024), 0, s, cand, ncand, g.cand_cap, max_kp, (float4*)kp, (int*)n_kp);
    HESIC_LAUNCH_RETURN("stereo_h_keypoints");
}

extern "C" int hesic_stereo_h_describe(const int32_t* I, const float* kp, const int32_t* n_kp, int N, int H, int W, int max_kp, float* desc,
                                       float* nrm, void* stream) {
    HESIC_CHECK_ARG(I && kp && n_kp && desc && nrm && N > 0 && N <= 65535 && H > 0 && W > 0 && max_kp > 0, "stereo_h_describe: bad arguments");
    hipLaunchKernelGGL(describe_kernel, dim3(max_kp, N), dim3(64), 0, (hipStream_t)stream, (const int*)I, H, W, (const float4*)kp,
                       (const int*)n_kp, max_kp, desc, nrm);
    HESIC_LAUNCH_RETURN("stereo_h_describe");
}

extern "C" int hesic_stereo_h_match(const float* desc, const float* nrm, const int32_t* n_kp, int B, int H, int W, int max_kp, int n_hyp,
                                    void* ws, size_t ws_bytes, int32_t* matches, int32_t* n_match, void* stream) {
    HESIC_CHECK_ARG(desc && nrm && n_kp && matches && n_match && B > 0 && max_kp > 0 && n_hyp > 0, "stereo_h_match: bad arguments");
    const WsLayout L = ws_layout(B, H, W, max_kp, n_hyp);
    WS_CHECK(L.total);
    int* best_t = (int*)((char*)ws + L.best_t);
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(match_kernel<64>, dim3((max_kp + 63) / 64, B), dim3(256), 0, s, desc, nrm, (const int*)n_kp, B, max_kp, best_t);
    hipLaunchKernelGGL(compact_matches_kernel, dim3(B), dim3(1024), 0, s, best_t, (const int*)n_kp, max_kp, (int2*)matches, (int*)n_match);
    HESIC_LAUNCH_RETURN("stereo_h_match");
}

extern "C" int hesic_stereo_h_ransac(const float* kp, const int32_t* matches, const int32_t* n_match, int B, int H, int W, int max_kp,
                                     int n_hyp, uint32_t seed, const uint32_t* pair_ids, void* ws, size_t ws_bytes, float* H_out,
                                     int32_t* valid, int32_t* inliers, int32_t* best, uint8_t* inlier_mask, void* stream) {
    HESIC_CHECK_ARG(kp && matches && n_match && pair_ids && H_out && valid && inliers && best && inlier_mask && B > 0 && B <= 65535 && max_kp > 0 &&
                    max_kp <= HESIC_STEREO_H_MAX_KEYPOINTS && n_hyp > 0, "stereo_h_ransac: bad arguments");
    const WsLayout L = ws_layout(B, H, W, max_kp, n_hyp);
    WS_CHECK(L.total);
    char* w = (char*)ws;
    int* hc = (int*)(w + L.hyp_cnt);
    float* he = (float*)(w + L.hyp_esum);
    float* hh = (float*)(w + L.hyp_H);
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(ransac_kernel, dim3((n_hyp + 63) / 64, B), dim3(64), sizeof(float4) * max_kp, s, (const float4*)kp,
                       (const int2*)matches, (const int*)n_match, B, max_kp, n_hyp, seed, pair_ids, hc, he, hh);
    hipLaunchKernelGGL(finish_kernel, dim3(B), dim3(256), 0, s, (const float4*)kp, (const int2*)matches, (const int*)n_match, B, max_kp,
                       n_hyp, hc, he, hh, H_out, (int*)valid, (int*)inliers, (int*)best, inlier_mask);
    HESIC_LAUNCH_RETURN("stereo_h_ransac");
}

extern "C" int hesic_stereo_h_orient(const int32_t* I, const float* kp, const int32_t* n_kp, int N, int H, int W, int max_kp, float* ori,
                                     void* stream) {
    HESIC_CHECK_ARG(I && kp && n_kp && ori && N > 0 && N <= 65535 && H > 0 && W > 0 && max_kp > 0 && max_kp <= HESIC_STEREO_H_MAX_KEYPOINTS,
                    "stereo_h_orient: bad arguments");
    hipLaunchKernelGGL(orient_kernel, dim3(max_kp, N), dim3(64), 0, (hipStream_t)stream, (const int*)I, H, W, (const float4*)kp,
                       (const int*)n_kp, max_kp, ori_table(), (float2*)ori);
    HESIC_LAUNCH_RETURN("stereo_h_orient");
}

extern "C" int hesic_stereo_h_describe_ex(const int32_t* I, const float* kp, const float* ori, const int32_t* n_kp, int N, int H, int W,
                                          int max_kp, int dim, float* desc, float* nrm, void* stream) {
    HESIC_CHECK_ARG(I && kp && n_kp && desc && nrm && N > 0 && N <= 65535 && H > 0 && W > 0 && max_kp > 0 &&
                    max_kp <= HESIC_STEREO_H_MAX_KEYPOINTS, "stereo_h_describe_ex: bad arguments");
    HESIC_CHECK_ARG(dim == 64 || dim == 128, "stereo_h_describe_ex: dim %d, 64 or 128 expected", dim);
    auto kern = dim == 64 ? describe_ex_kernel<64> : describe_ex_kernel<128>;
    hipLaunchKernelGGL(kern, dim3(max_kp, N), dim3(64), 0, (hipStream_t)stream, (const int*)I, H, W, (const float4*)kp, (const float2*)ori,
                       (const int*)n_kp, max_kp, desc, nrm);
    HESIC_LAUNCH_RETURN("stereo_h_describe_ex");
}

extern "C" int hesic_stereo_h_match_ex(const float* desc, const float* nrm, const int32_t* n_kp, int B, int H, int W, int max_kp, int n_hyp,
                                       int dim, void* ws, size_t ws_bytes, int32_t* matches, int32_t* n_match, void* stream) {
    HESIC_CHECK_ARG(desc && nrm && n_kp && matches && n_match && B > 0 && B <= 65535 && max_kp > 0 && max_kp <= HESIC_STEREO_H_MAX_KEYPOINTS &&
                    n_hyp > 0, "stereo_h_match_ex: bad arguments");
    HESIC_CHECK_ARG(dim == 64 || dim == 128, "stereo_h_match_ex: dim %d, 64 or 128 expected", dim);
    const WsLayout L = ws_layout(B, H, W, max_kp, n_hyp);
    WS_CHECK(L.total);
    int* best_t = (int*)((char*)ws + L.best_t);
    hipStream_t s = (hipStream_t)stream;
    auto kern = dim == 64 ? match_kernel<64> : match_kernel<128>;
    hipLaunchKernelGGL(kern, dim3((max_kp + 63) / 64, B), dim3(256), 0, s, desc, nrm, (const int*)n_kp, B, max_kp, best_t);
    hipLaunchKernelGGL(compact_matches_kernel, dim3(B), dim3(1024), 0, s, best_t, (const int*)n_kp, max_kp, (int2*)matches, (int*)n_match);
    HESIC_LAUNCH_RETURN("stereo_h_match_ex");
}

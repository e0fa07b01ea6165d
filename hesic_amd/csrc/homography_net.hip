// HomographyNet in training mode (include/hesic_homography_net.h): what ywz/mywork/model.py:73-101 needs beside the conv kernels --
//   * the backward of MaxPool2d(2,2) (argmax recomputed from the pool's input, every element of gx written);
//   * flatten (NHWC map -> the reference's NCHW flatten order) fused with inverted dropout, forward and backward, the mask a counter-based
//     Philox4x32-10 stream of the LOGICAL output index (nothing stored, no dependence on grid or vector width);
//   * a small-batch Linear layer over the fp32 master weight in nn.Linear's own layout: forward, data gradient, weight / bias gradient.
//   * order-fixed forms of the conv bias gradient and of the first layer's (two input channels) weight gradient, whose usual kernels end
//     in float atomics.
//
// The Linear kernels stream the weight (fc.2: 1024 x 32768 fp32 = 134 MB) exactly once per pass, straight from global memory into the
// operand registers of v_mfma_f32_16x16x4_f32 (exact fp32: a k-ordered fma chain per output, so a row's bits do not depend on its
// neighbours).  The batch (<= 64 rows, NB tiles of 16) sits on the MFMA's N side in the forward and the data gradient and is the
// contraction of the weight gradient.  Why the matrix cores for a bandwidth-bound kernel: a VALU form needs B x (rows per lane)
// accumulators per lane and reads x from LDS once per weight row -- at B = 64 that is 64 ds_read_b128 per 16 weight bytes, six times what
// the LDS delivers at the HBM rate -- while the MFMA shares one x fragment among 16 weight rows and leaves the VALU idle.
// No atomics; every sum has a fixed order.
#include "common.h"
#include "../../include/hesic_homography_net.h"
#include "../../include/hesic_dropout_state.h"

namespace {

// four consecutive elements of type T <-> f32x4 (one 16-byte access for fp32, one 8-byte access for the 16-bit format)
template <typename T> struct vec4;
template <> struct vec4<float> {
    static __device__ __forceinline__ f32x4 ld(const float* p) { return *(const f32x4*)p; }
    static __device__ __forceinline__ void st(float* p, f32x4 v) { *(f32x4*)p = v; }
};
template <> struct vec4<h16_t> {
    static __device__ __forceinline__ f32x4 ld(const h16_t* p) {
        const u32x2 r = *(const u32x2*)p;
        return f32x4{h2f_lo(r.x), h2f_hi(r.x), h2f_lo(r.y), h2f_hi(r.y)};
    }
    static __device__ __forceinline__ void st(h16_t* p, f32x4 v) { *(u32x2*)p = u32x2{pack_h2(v.x, v.y), pack_h2(v.z, v.w)}; }
};

// ------------------------------------------------------------------------------------------------------------ max pool backward
// One thread per 2x2 window and 16-byte channel group, over ceil(H/2) x ceil(W/2) windows: the windows of an odd last row / column hold
// no maximum and are zero-filled where they lie inside the map.
template <typename T>
__global__ void maxpool2_bwd_kernel(const T* __restrict__ x, const T* __restrict__ gy, T* __restrict__ gx, int B, int H, int W, int C) {
    constexpr int V = 16 / sizeof(T);
    const int Ho = H >> 1, Wo = W >> 1, Hc = (H + 1) >> 1, Wc = (W + 1) >> 1, cg = C / V;
    const int64_t total = (int64_t)B * Hc * Wc * cg;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int c = (int)(i % cg) * V;
        int64_t r = i / cg;
        const int wx = r % Wc; r /= Wc;
        const int wy = r % Hc;
        const int b = r / Hc;
        const int64_t base = (((int64_t)b * H + 2 * wy) * W + 2 * wx) * C + c;
        if (wy < Ho && wx < Wo) {
            float m[V];
            int arg[V];
#pragma unroll
            for (int e = 0; e < V; ++e) { m[e] = -INFINITY; arg[e] = 0; }
#pragma unroll
            for (int pos = 0; pos < 4; ++pos) {
                const u32x4 raw = *(const u32x4*)(x + base + ((int64_t)(pos >> 1) * W + (pos & 1)) * C);
                const T* v = (const T*)&raw;
#pragma unroll
                for (int e = 0; e < V; ++e) {
                    const float f = elem<T>::ld(v + e);
                    if (f > m[e]) { m[e] = f; arg[e] = pos; }          // strictly greater: the first maximum keeps the gradient
                }
            }
            const u32x4 graw = *(const u32x4*)(gy + (((int64_t)b * Ho + wy) * Wo + wx) * C + c);
            const T* g = (const T*)&graw;
#pragma unroll
            for (int pos = 0; pos < 4; ++pos) {
                u32x4 out;
                T* o = (T*)&out;
#pragma unroll
                for (int e = 0; e < V; ++e) o[e] = arg[e] == pos ? g[e] : (T)0;
                *(u32x4*)(gx + base + ((int64_t)(pos >> 1) * W + (pos & 1)) * C) = out;
            }
        } else {
#pragma unroll
            for (int pos = 0; pos < 4; ++pos)
                if (2 * wy + (pos >> 1) < H && 2 * wx + (pos & 1) < W)
                    *(u32x4*)(gx + base + ((int64_t)(pos >> 1) * W + (pos & 1)) * C) = u32x4{0u, 0u, 0u, 0u};
        }
    }
}

// ------------------------------------------------------------------------------------------------------------ flatten + dropout
struct DropArgs { uint32_t thr; float scale; uint32_t k0, k1, step, site; };

// Where a launch finds (k0, k1, step): in its kernel arguments, or in the 16 bytes {seed lo, seed hi, step, reserved} that
// hesic_dropout_state_take left in device memory (wave-uniform: every thread loads the three words once).
struct KeysByValue {
    __device__ __forceinline__ DropArgs resolve(const DropArgs& a) const { return a; }
};
struct KeysFromState {
    const uint32_t* __restrict__ taken;
    __device__ __forceinline__ DropArgs resolve(const DropArgs& a) const { return DropArgs{a.thr, a.scale, taken[0], taken[1], taken[2], a.site}; }
};

// state -> taken, then state.step += 1 (mod 2^32): what Net._forward_train does to its host counter, as one lane's work
__global__ void dropout_state_take_kernel(uint32_t* __restrict__ state, uint32_t* __restrict__ taken) {
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        const uint32_t lo = state[0], hi = state[1], step = state[2], rsv = state[3];
        taken[0] = lo; taken[1] = hi; taken[2] = step; taken[3] = rsv;
        state[2] = step + 1u;
    }
}

__device__ __forceinline__ u32x4 philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint32_t h0 = __umulhi(0xD2511F53u, c0), l0 = 0xD2511F53u * c0;
        const uint32_t h1 = __umulhi(0xCD9E8D57u, c2), l1 = 0xCD9E8D57u * c2;
        c0 = h1 ^ c1 ^ k0; c1 = l1; c2 = h0 ^ c3 ^ k1; c3 = l0;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    return u32x4{c0, c1, c2, c3};
}

// the four elements whose logical index starts at e0 = b * F + j (a multiple of 4): kept ones times scale, dropped ones +0
__device__ __forceinline__ f32x4 drop4(f32x4 v, int64_t e0, const DropArgs& a) {
    const uint64_t q = (uint64_t)e0 >> 2;
    const u32x4 w = philox4x32_10((uint32_t)q, (uint32_t)(q >> 32), a.step, a.site, a.k0, a.k1);
    return f32x4{w.x >= a.thr ? v.x * a.scale : 0.f, w.y >= a.thr ? v.y * a.scale : 0.f, w.z >= a.thr ? v.z * a.scale : 0.f,
                 w.w >= a.thr ? v.w * a.scale : 0.f};
}

// HW % 4 == 0 and C % 4 == 0: a 32-pixel x 32-channel tile goes through LDS, so that the NHWC side is accessed in runs of four channels
// and the flat side in runs of four pixels.  FWD: src = NHWC map, dst = flat rows; else src = flat gradient, dst = NHWC gradient.
template <typename T, bool FWD, typename Keys>
__global__ __launch_bounds__(256) void flatten_dropout_tile_kernel(const T* __restrict__ src, T* __restrict__ dst, int HW, int C, DropArgs a0,
                                                                   Keys keys) {
    __shared__ float s[32][33];                     // [channel][pixel]
    const DropArgs a = keys.resolve(a0);
    const int b = blockIdx.z, p0 = blockIdx.x * 32, c0 = blockIdx.y * 32;
    const int rl = threadIdx.x >> 3, g4 = (threadIdx.x & 7) * 4;
    const int64_t F = (int64_t)C * HW;
    const int pn = p0 + rl, cn = c0 + g4;           // this thread's run on the NHWC side: pixel pn, channels cn .. cn+3
    const int cf = c0 + rl, pf = p0 + g4;           // and on the flat side: channel cf, pixels pf .. pf+3
    const int64_t e0 = (int64_t)b * F + (int64_t)cf * HW + pf;
    if (FWD) {
        if (pn < HW && cn < C) {
            const f32x4 v = vec4<T>::ld(src + ((int64_t)b * HW + pn) * C + cn);
            s[g4 + 0][rl] = v.x; s[g4 + 1][rl] = v.y; s[g4 + 2][rl] = v.z; s[g4 + 3][rl] = v.w;
        }
        __syncthreads();
        if (cf < C && pf < HW)
            vec4<T>::st(dst + e0, drop4(f32x4{s[rl][g4], s[rl][g4 + 1], s[rl][g4 + 2], s[rl][g4 + 3]}, e0, a));
    } else {
        if (cf < C && pf < HW) {
            const f32x4 v = drop4(vec4<T>::ld(src + e0), e0, a);
            s[rl][g4] = v.x; s[rl][g4 + 1] = v.y; s[rl][g4 + 2] = v.z; s[rl][g4 + 3] = v.w;
        }
        __syncthreads();
        if (pn < HW && cn < C)
            vec4<T>::st(dst + ((int64_t)b * HW + pn) * C + cn, f32x4{s[g4][rl], s[g4 + 1][rl], s[g4 + 2][rl], s[g4 + 3][rl]});
    }
}

// any HW (HW = 1: the second dropout site, where both orders coincide): one thread per four flat elements, the NHWC side element by element
template <typename T, bool FWD, typename Keys>
__global__ void flatten_dropout_flat_kernel(const T* __restrict__ src, T* __restrict__ dst, int B, int HW, int C, DropArgs a0, Keys keys) {
    const DropArgs a = keys.resolve(a0);
    const int64_t F = (int64_t)C * HW, total = (int64_t)B * F / 4;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t e0 = 4 * i, b = e0 / F, j = e0 % F;
        int64_t at[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) at[e] = (b * HW + (j + e) % HW) * C + (j + e) / HW;
        if (FWD) {
            const f32x4 v{elem<T>::ld(src + at[0]), elem<T>::ld(src + at[1]), elem<T>::ld(src + at[2]), elem<T>::ld(src + at[3])};
            vec4<T>::st(dst + e0, drop4(v, e0, a));
        } else {
            const f32x4 v = drop4(vec4<T>::ld(src + e0), e0, a);
            elem<T>::st(dst + at[0], v.x); elem<T>::st(dst + at[1], v.y); elem<T>::st(dst + at[2], v.z); elem<T>::st(dst + at[3], v.w);
        }
    }
}

template <typename T, bool FWD, typename Keys>
void launch_flatten_dropout(const void* src, void* dst, int B, int HW, int C, const DropArgs& a, Keys keys, hipStream_t st) {
    if (HW % 4 == 0)
        hipLaunchKernelGGL((flatten_dropout_tile_kernel<T, FWD, Keys>), dim3((HW + 31) / 32, (C + 31) / 32, B), dim3(256), 0, st, (const T*)src,
                           (T*)dst, HW, C, a, keys);
    else
        hipLaunchKernelGGL((flatten_dropout_flat_kernel<T, FWD, Keys>), dim3(grid_for((int64_t)B * C * HW / 4, 256)), dim3(256), 0, st,
                           (const T*)src, (T*)dst, B, HW, C, a, keys);
}

// `a` holds thr, scale and site, and with KeysByValue the keys and the step too
template <typename Keys>
int flatten_dropout(const char* name, bool fwd, const void* src, void* dst, int B, int HW, int C, const DropArgs& a, Keys keys, int dtype,
                    void* stream) {
    HESIC_CHECK_ARG(src && dst, "%s: null pointer", name);
    HESIC_CHECK_ARG(B > 0 && B <= 65535 && HW > 0 && C > 0, "%s: bad sizes B=%d HW=%d C=%d", name, B, HW, C);
    HESIC_CHECK_ARG(dtype == HESIC_H16 || dtype == HESIC_F32, "%s: bad dtype", name);
    HESIC_CHECK_ARG(((int64_t)C * HW) % 4 == 0, "%s: F = C * HW = %lld must be a multiple of 4", name, (long long)C * HW);
    HESIC_CHECK_ARG(HW == 1 || C % 4 == 0, "%s: C=%d must be a multiple of 4", name, C);
    const hipStream_t st = (hipStream_t)stream;
    if (dtype == HESIC_H16) {
        if (fwd) launch_flatten_dropout<h16_t, true>(src, dst, B, HW, C, a, keys, st);
        else launch_flatten_dropout<h16_t, false>(src, dst, B, HW, C, a, keys, st);
    } else {
        if (fwd) launch_flatten_dropout<float, true>(src, dst, B, HW, C, a, keys, st);
        else launch_flatten_dropout<float, false>(src, dst, B, HW, C, a, keys, st);
    }
    HESIC_LAUNCH_RETURN(name);
}

int flatten_dropout_value(const char* name, bool fwd, const void* src, void* dst, int B, int HW, int C, uint32_t thr, float scale, uint64_t seed,
                          uint32_t step, uint32_t site, int dtype, void* stream) {
    const DropArgs a{thr, scale, (uint32_t)(seed & 0xffffffffu), (uint32_t)(seed >> 32), step, site};
    return flatten_dropout(name, fwd, src, dst, B, HW, C, a, KeysByValue{}, dtype, stream);
}

int flatten_dropout_state(const char* name, bool fwd, const void* src, void* dst, int B, int HW, int C, uint32_t thr, float scale,
                          const void* taken, uint32_t site, int dtype, void* stream) {
    HESIC_CHECK_ARG(taken, "%s: null taken (the 16 bytes hesic_dropout_state_take wrote)", name);
    const DropArgs a{thr, scale, 0u, 0u, 0u, site};
    return flatten_dropout(name, fwd, src, dst, B, HW, C, a, KeysFromState{(const uint32_t*)taken}, dtype, stream);
}

// ------------------------------------------------------------------------------------------------------------ small-batch Linear
// v_mfma_f32_16x16x4_f32: lane l supplies A[m = l & 15][k = l >> 4] and B[k = l >> 4][n = l & 15]; it receives D[m = 4 (l >> 4) + reg][n = l & 15].
#define mfma_16x16x4 __builtin_amdgcn_mfma_f32_16x16x4f32

constexpr int LIN_FWD_OUT = 32;         // outputs per forward block (two M tiles per wave)
constexpr int LIN_WG_OUT = 128;         // outputs per weight-gradient block (four waves x two M tiles)
constexpr int LIN_WG_CHUNKS = 4;        // 64-column chunks per weight-gradient block
constexpr int LIN_FWD_UNROLL = 4;       // K steps of 16 whose loads are issued together (forward)
constexpr int LIN_DG_UNROLL = 8;        // K steps of 4 whose loads are issued together (data gradient)

// In-slice of one forward block: a function of In alone (a row's bits must not depend on B).  Each of the four waves takes a quarter.
static inline int lin_fwd_kb(int In) { return In >= 8192 ? 1024 : 256; }
static inline int lin_fwd_outp(int Out) { return (Out + LIN_FWD_OUT - 1) / LIN_FWD_OUT * LIN_FWD_OUT; }

// Forward partials: block (o-tile of 32, In-slice s) -> ws[s][b][o].  M = outputs, N = rows, K = In.  A lane's 16-byte weight load is four
// K steps of its row; the same lane pattern loads x, so the two operands agree on k.
template <typename T, int NB>
__global__ __launch_bounds__(256) void linear_fwd_kernel(const T* __restrict__ x, const float* __restrict__ W, float* __restrict__ ws, int B,
                                                         int In, int Out, int Outp, int KB) {
    __shared__ f32x4 red[3][2 * NB][64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, r = lane & 15, g = lane >> 4;
    const int o0 = blockIdx.x * LIN_FWD_OUT, s = blockIdx.y;
    const int kq = KB / 4, kbeg = s * KB + wave * kq, kend = min(kbeg + kq, In);
    const float* wp[2];
    bool wok[2];
#pragma unroll
    for (int t = 0; t < 2; ++t) {
        const int o = o0 + 16 * t + r;
        wok[t] = o < Out;
        wp[t] = W + (int64_t)(wok[t] ? o : 0) * In;
    }
    const T* xp[NB];
    bool xok[NB];
#pragma unroll
    for (int n = 0; n < NB; ++n) {
        const int b = 16 * n + r;
        xok[n] = b < B;
        xp[n] = x + (int64_t)(xok[n] ? b : 0) * In;
    }
    f32x4 acc[2][NB];
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int n = 0; n < NB; ++n) acc[t][n] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int ks = kbeg; ks < kend; ks += 16 * LIN_FWD_UNROLL) {          // all loads of LIN_FWD_UNROLL K steps in flight, then their MFMAs
        f32x4 a[LIN_FWD_UNROLL][2], bb[LIN_FWD_UNROLL][NB];
#pragma unroll
        for (int u = 0; u < LIN_FWD_UNROLL; ++u) {
            const int k = ks + 16 * u + 4 * g;
            const bool kin = k < kend;
            const int kk = kin ? k : 0;             // always a valid address; the value is dropped below
#pragma unroll
            for (int t = 0; t < 2; ++t) {
                a[u][t] = *(const f32x4*)(wp[t] + kk);
                if (!(kin && wok[t])) a[u][t] = f32x4{0.f, 0.f, 0.f, 0.f};
            }
#pragma unroll
            for (int n = 0; n < NB; ++n) {
                bb[u][n] = vec4<T>::ld(xp[n] + kk);
                if (!(kin && xok[n])) bb[u][n] = f32x4{0.f, 0.f, 0.f, 0.f};
            }
        }
#pragma unroll
        for (int u = 0; u < LIN_FWD_UNROLL; ++u)
#pragma unroll
            for (int e = 0; e < 4; ++e)
#pragma unroll
                for (int t = 0; t < 2; ++t)
#pragma unroll
                    for (int n = 0; n < NB; ++n) acc[t][n] = mfma_16x16x4(a[u][t][e], bb[u][n][e], acc[t][n], 0, 0, 0);
    }
    if (wave > 0) {
#pragma unroll
        for (int t = 0; t < 2; ++t)
#pragma unroll
            for (int n = 0; n < NB; ++n) red[wave - 1][t * NB + n][lane] = acc[t][n];
    }
    __syncthreads();
    if (wave == 0) {
#pragma unroll
        for (int t = 0; t < 2; ++t)
#pragma unroll
            for (int n = 0; n < NB; ++n) {
                f32x4 v = acc[t][n];
#pragma unroll
                for (int w = 0; w < 3; ++w) v += red[w][t * NB + n][lane];
                const int b = 16 * n + r;
                if (b < B) *(f32x4*)(ws + ((int64_t)s * B + b) * Outp + o0 + 16 * t + 4 * g) = v;      // outputs o0+16t+4g .. +3 (zeros past Out)
            }
    }
}

template <typename T>
__global__ void linear_fwd_finish_kernel(const float* __restrict__ ws, const float* __restrict__ bias, T* __restrict__ y, int B, int Out,
                                         int Outp, int S, int act) {
    const int64_t total = (int64_t)B * Out;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int b = (int)(i / Out), o = (int)(i % Out);
        float v = ws[(int64_t)b * Outp + o];
        for (int s = 1; s < S; ++s) v += ws[((int64_t)s * B + b) * Outp + o];
        if (bias) v += bias[o];
        elem<T>::st(y + i, apply_act(v, act));
    }
}

// Data gradient: block = 64 columns of W, the four waves split Out.  M = columns (a lane's 16-byte load feeds four M tiles: tile e holds
// columns i0 + 4 m + e), N = rows, K = outputs.
template <typename T, int NB>
__global__ __launch_bounds__(256) void linear_dgrad_kernel(const T* __restrict__ gy, const float* __restrict__ W, T* __restrict__ gx, int B,
                                                           int In, int Out) {
    __shared__ f32x4 red[3][4 * NB][64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, r = lane & 15, g = lane >> 4;
    const int i = blockIdx.x * 64 + 4 * r;
    const bool iok = i < In;
    const int kq = (((Out + 3) / 4 + 3) / 4) * 4, kbeg = wave * kq, kend = min(kbeg + kq, Out);
    const float* wp = W + (iok ? i : 0);
    const T* gp[NB];
    bool bok[NB];
#pragma unroll
    for (int n = 0; n < NB; ++n) {
        const int b = 16 * n + r;
        bok[n] = b < B;
        gp[n] = gy + (int64_t)(bok[n] ? b : 0) * Out;
    }
    f32x4 acc[4][NB];
#pragma unroll
    for (int e = 0; e < 4; ++e)
#pragma unroll
        for (int n = 0; n < NB; ++n) acc[e][n] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int k0 = kbeg; k0 < kend; k0 += 4 * LIN_DG_UNROLL) {
        f32x4 a[LIN_DG_UNROLL];
        float bb[LIN_DG_UNROLL][NB];
#pragma unroll
        for (int u = 0; u < LIN_DG_UNROLL; ++u) {
            const int o = k0 + 4 * u + g;
            const bool ook = o < kend;
            const int oo = ook ? o : 0;
            a[u] = *(const f32x4*)(wp + (int64_t)oo * In);
            if (!(ook && iok)) a[u] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int n = 0; n < NB; ++n) {
                bb[u][n] = elem<T>::ld(gp[n] + oo);
                if (!(ook && bok[n])) bb[u][n] = 0.f;
            }
        }
#pragma unroll
        for (int u = 0; u < LIN_DG_UNROLL; ++u)
#pragma unroll
            for (int e = 0; e < 4; ++e)
#pragma unroll
                for (int n = 0; n < NB; ++n) acc[e][n] = mfma_16x16x4(a[u][e], bb[u][n], acc[e][n], 0, 0, 0);
    }
    if (wave > 0) {
#pragma unroll
        for (int e = 0; e < 4; ++e)
#pragma unroll
            for (int n = 0; n < NB; ++n) red[wave - 1][e * NB + n][lane] = acc[e][n];
    }
    __syncthreads();
    if (wave == 0) {
#pragma unroll
        for (int e = 0; e < 4; ++e)
#pragma unroll
            for (int n = 0; n < NB; ++n)
#pragma unroll
                for (int w = 0; w < 3; ++w) acc[e][n] += red[w][e * NB + n][lane];
        // D[m = 4 g + reg][n = r] of tile e is column i0 + 4 (4 g + reg) + e: the four tiles of one reg are four consecutive columns
        const int ic = blockIdx.x * 64 + 16 * g;
#pragma unroll
        for (int n = 0; n < NB; ++n) {
            const int b = 16 * n + r;
#pragma unroll
            for (int q = 0; q < 4; ++q)
                if (b < B && ic + 4 * q < In)
                    vec4<T>::st(gx + (int64_t)b * In + ic + 4 * q, f32x4{acc[0][n][q], acc[1][n][q], acc[2][n][q], acc[3][n][q]});
        }
    }
}

// Weight gradient: M = outputs (two tiles per wave), N = columns (four tiles per 16-byte x load, as above), K = rows (ascending).  The gy
// fragments stay in registers while the wave walks its chunks of 64 columns; every dW element is written (or read and written) once.
template <typename T, int NB>
__global__ __launch_bounds__(256) void linear_wgrad_kernel(const T* __restrict__ x, const T* __restrict__ gy, float* __restrict__ dW,
                                                           float* __restrict__ db, int B, int In, int Out, int accumulate) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, r = lane & 15, g = lane >> 4;
    const int o0 = blockIdx.x * LIN_WG_OUT + wave * 32;
    float a[2][4 * NB];
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int ks = 0; ks < 4 * NB; ++ks) {
            const int b = 4 * ks + g, o = o0 + 16 * t + r;
            const bool ok = b < B && o < Out;
            const float v = elem<T>::ld(gy + (ok ? (int64_t)b * Out + o : 0));
            a[t][ks] = ok ? v : 0.f;
        }
    for (int c = 0; c < LIN_WG_CHUNKS; ++c) {
        const int i0 = (blockIdx.y * LIN_WG_CHUNKS + c) * 64;
        if (i0 >= In) break;
        const int i = i0 + 4 * r;
        const bool iok = i < In;
        // rows this lane group really has in this chunk (none past In): one per-chunk count instead of 4 NB loop-invariant lane masks,
        // which the compiler would keep in scalar register pairs across the whole chunk loop
        const int kmax = iok ? (B - g + 3) >> 2 : 0;
        const T* xp = x + (iok ? i : 0);
        f32x4 acc[2][4];
#pragma unroll
        for (int t = 0; t < 2; ++t)
#pragma unroll
            for (int e = 0; e < 4; ++e) acc[t][e] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int ks = 0; ks < 4 * NB; ++ks) {
            f32x4 xv = vec4<T>::ld(xp + (int64_t)min(4 * ks + g, B - 1) * In);          // always a valid row; dropped below
            if (ks >= kmax) xv = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int t = 0; t < 2; ++t)
#pragma unroll
                for (int e = 0; e < 4; ++e) acc[t][e] = mfma_16x16x4(a[t][ks], xv[e], acc[t][e], 0, 0, 0);
        }
        // D[m = 4 g + reg][n = r] of tile e: output o0 + 16 t + 4 g + reg, column i0 + 4 r + e
#pragma unroll
        for (int t = 0; t < 2; ++t)
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int o = o0 + 16 * t + 4 * g + q;
                if (o < Out && iok) {
                    float* p = dW + (int64_t)o * In + i;
                    f32x4 v{acc[t][0][q], acc[t][1][q], acc[t][2][q], acc[t][3][q]};
                    if (accumulate) v += *(const f32x4*)p;
                    *(f32x4*)p = v;
                }
            }
    }
    if (db && blockIdx.y == 0 && threadIdx.x < LIN_WG_OUT) {
        const int o = blockIdx.x * LIN_WG_OUT + threadIdx.x;
        if (o < Out) {
            float v = 0.f;
            for (int b = 0; b < B; ++b) v += elem<T>::ld(gy + (int64_t)b * Out + o);
            db[o] = accumulate ? db[o] + v : v;
        }
    }
}

// ------------------------------------------------------------------------------------------------ order-fixed conv bias / first-layer gradients
// The conv kernels' own bias gradient (column sums) and the weight gradient of a conv with a few input channels end in float atomics, so
// their last bits change from run to run.  HomographyNet's training promises the same bits in every run and after a resume: under
// functional.deterministic_conv_grads() those two gradients come from the kernels below -- per-block partial sums over a pixel range that
// depends on the sizes alone, in a caller-provided workspace, added in block order by a second launch.
constexpr int DET_BLOCKS = HESIC_DET_MAX_BLOCKS;

// thread = (row lane, channel): 256 / C rows of the NHWC gradient per pass, each thread a sequential sum; row lanes meet in LDS in order
template <typename T>
__global__ __launch_bounds__(256) void bias_grad_partial_kernel(const T* __restrict__ gy, float* __restrict__ part, int64_t P, int C, int64_t chunk) {
    __shared__ float red[256];
    const int c = threadIdx.x % C, rl = threadIdx.x / C, R = 256 / C;
    const int64_t p0 = blockIdx.x * chunk, p1 = min(p0 + chunk, P);
    float acc = 0.f;
    for (int64_t p = p0 + rl; p < p1; p += R) acc += elem<T>::ld(gy + p * C + c);
    red[threadIdx.x] = acc;
    __syncthreads();
    if (rl == 0) {
        for (int r = 1; r < R; ++r) acc += red[r * C + c];
        part[(int64_t)blockIdx.x * C + c] = acc;
    }
}

// out[i] (+)= sum over blocks, ascending
__global__ void det_finish_kernel(const float* __restrict__ part, float* __restrict__ out, int n, int nblocks, int accumulate) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    float v = part[i];
    for (int b = 1; b < nblocks; ++b) v += part[(int64_t)b * n + i];
    out[i] = accumulate ? out[i] + v : v;
}

// dW[co][ci][ky][kx] of a 3x3, stride 1, pad 1 conv with CIN input channels: x (B, CIN, H, W) fp32 contiguous, gy (B, H, W, Cout) NHWC.
// thread = (row lane, output channel); the x taps of a pixel are the same address for all channels of a row lane (one broadcast load).
template <typename T, int CIN>
__global__ __launch_bounds__(256) void narrow_in_wgrad_partial_kernel(const float* __restrict__ x, const T* __restrict__ gy, float* __restrict__ part,
                                                                      int B, int H, int W, int C, int64_t chunk) {
    constexpr int NT = CIN * 9;
    __shared__ float red[256];
    const int c = threadIdx.x % C, rl = threadIdx.x / C, R = 256 / C;
    const int64_t P = (int64_t)B * H * W, p0 = blockIdx.x * chunk, p1 = min(p0 + chunk, P);
    float acc[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t) acc[t] = 0.f;
    for (int64_t p = p0 + rl; p < p1; p += R) {
        const int px = (int)(p % W), py = (int)((p / W) % H), b = (int)(p / ((int64_t)W * H));
        const float g = elem<T>::ld(gy + p * C + c);
#pragma unroll
        for (int ci = 0; ci < CIN; ++ci)
#pragma unroll
            for (int ky = 0; ky < 3; ++ky)
#pragma unroll
                for (int kx = 0; kx < 3; ++kx) {
                    const int yy = py + ky - 1, xx = px + kx - 1;
                    const bool ok = yy >= 0 && yy < H && xx >= 0 && xx < W;
                    const float xv = ok ? x[(((int64_t)b * CIN + ci) * H + yy) * W + xx] : 0.f;
                    acc[(ci * 3 + ky) * 3 + kx] += g * xv;
                }
    }
#pragma unroll
    for (int t = 0; t < NT; ++t) {
        __syncthreads();
        red[threadIdx.x] = acc[t];
        __syncthreads();
        if (rl == 0) {
            float v = acc[t];
            for (int r = 1; r < R; ++r) v += red[r * C + c];
            part[((int64_t)blockIdx.x * C + c) * NT + t] = v;
        }
    }
}

// pixel range per block and block count: functions of P alone
static inline int det_blocks(int64_t P, int64_t* chunk) {
    int64_t ch = (P + DET_BLOCKS - 1) / DET_BLOCKS;
    if (ch < 64) ch = 64;
    *chunk = ch;
    return (int)((P + ch - 1) / ch);
}

int linear_check(const char* name, int B, int In, int Out, int dtype) {
    HESIC_CHECK_ARG(B >= 1 && B <= HESIC_LINEAR_MAX_ROWS, "%s: B=%d outside 1 .. %d", name, B, HESIC_LINEAR_MAX_ROWS);
    HESIC_CHECK_ARG(In >= 4 && In % 4 == 0, "%s: In=%d must be a positive multiple of 4", name, In);
    HESIC_CHECK_ARG(Out >= 1, "%s: Out=%d", name, Out);
    HESIC_CHECK_ARG((int64_t)In * Out < ((int64_t)1 << 40), "%s: weight too large", name);
    HESIC_CHECK_ARG(dtype == HESIC_H16 || dtype == HESIC_F32, "%s: bad dtype", name);
    return 0;
}

// launch KERNEL<T, NB> with NB = row tiles of 16 (1 .. 4)
#define LINEAR_LAUNCH(KERNEL, T, grid, ...)                                                                  \
    switch ((B + 15) / 16) {                                                                                 \
        case 1: hipLaunchKernelGGL((KERNEL<T, 1>), grid, dim3(256), 0, st, __VA_ARGS__); break;              \
        case 2: hipLaunchKernelGGL((KERNEL<T, 2>), grid, dim3(256), 0, st, __VA_ARGS__); break;              \
        case 3: hipLaunchKernelGGL((KERNEL<T, 3>), grid, dim3(256), 0, st, __VA_ARGS__); break;              \
        default: hipLaunchKernelGGL((KERNEL<T, 4>), grid, dim3(256), 0, st, __VA_ARGS__); break;             \
    }

}  // namespace

extern "C" int hesic_maxpool2_backward(const void* x, const void* gy, void* gx, int B, int H, int W, int C, int dtype, void* stream) {
    HESIC_CHECK_ARG(x && gy && gx, "maxpool2_backward: null pointer");
    HESIC_CHECK_ARG(B > 0 && H > 1 && W > 1 && C > 0, "maxpool2_backward: bad sizes B=%d H=%d W=%d C=%d", B, H, W, C);
    HESIC_CHECK_ARG(dtype == HESIC_H16 || dtype == HESIC_F32, "maxpool2_backward: bad dtype");
    const int V = dtype == HESIC_H16 ? 8 : 4;
    HESIC_CHECK_ARG(C % V == 0, "maxpool2_backward: C=%d must be a multiple of %d", C, V);
    const int64_t total = (int64_t)B * ((H + 1) / 2) * ((W + 1) / 2) * (C / V);
    if (dtype == HESIC_H16)
        hipLaunchKernelGGL(maxpool2_bwd_kernel<h16_t>, dim3(grid_for(total, 256)), dim3(256), 0, (hipStream_t)stream, (const h16_t*)x,
                           (const h16_t*)gy, (h16_t*)gx, B, H, W, C);
    else
        hipLaunchKernelGGL(maxpool2_bwd_kernel<float>, dim3(grid_for(total, 256)), dim3(256), 0, (hipStream_t)stream, (const float*)x,
                           (const float*)gy, (float*)gx, B, H, W, C);
    HESIC_LAUNCH_RETURN("maxpool2_backward");
}

extern "C" int hesic_flatten_dropout_forward(const void* x, void* y, int B, int HW, int C, uint32_t thr, float scale, uint64_t seed,
                                             uint32_t step, uint32_t site, int dtype, void* stream) {
    return flatten_dropout_value("flatten_dropout_forward", true, x, y, B, HW, C, thr, scale, seed, step, site, dtype, stream);
}

extern "C" int hesic_flatten_dropout_backward(const void* gy, void* gx, int B, int HW, int C, uint32_t thr, float scale, uint64_t seed,
                                              uint32_t step, uint32_t site, int dtype, void* stream) {
    return flatten_dropout_value("flatten_dropout_backward", false, gy, gx, B, HW, C, thr, scale, seed, step, site, dtype, stream);
}

extern "C" int hesic_dropout_state_take(void* state, void* taken, void* stream) {
    HESIC_CHECK_ARG(state && taken, "dropout_state_take: null pointer");
    HESIC_CHECK_ARG(state != taken, "dropout_state_take: state and taken are one buffer");
    hipLaunchKernelGGL(dropout_state_take_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, (uint32_t*)state, (uint32_t*)taken);
    HESIC_LAUNCH_RETURN("dropout_state_take");
}

extern "C" int hesic_flatten_dropout_forward_state(const void* x, void* y, int B, int HW, int C, uint32_t thr, float scale, const void* taken,
                                                   uint32_t site, int dtype, void* stream) {
    return flatten_dropout_state("flatten_dropout_forward_state", true, x, y, B, HW, C, thr, scale, taken, site, dtype, stream);
}

extern "C" int hesic_flatten_dropout_backward_state(const void* gy, void* gx, int B, int HW, int C, uint32_t thr, float scale, const void* taken,
                                                    uint32_t site, int dtype, void* stream) {
    return flatten_dropout_state("flatten_dropout_backward_state", false, gy, gx, B, HW, C, thr, scale, taken, site, dtype, stream);
}

extern "C" size_t hesic_linear_forward_ws_bytes(int B, int In, int Out) {
    if (B < 1 || B > HESIC_LINEAR_MAX_ROWS || In < 4 || Out < 1) return 0;
    const int KB = lin_fwd_kb(In), S = (In + KB - 1) / KB;
    return (size_t)S * B * lin_fwd_outp(Out) * sizeof(float);
}

extern "C" int hesic_linear_forward(const void* x, const float* W, const float* bias, void* y, int B, int In, int Out, int act, int dtype,
                                    void* ws, size_t ws_bytes, void* stream) {
    if (int rc = linear_check("linear_forward", B, In, Out, dtype)) return rc;
    HESIC_CHECK_ARG(x && W && y && ws, "linear_forward: null pointer");
    HESIC_CHECK_ARG(act == HESIC_ACT_NONE || act == HESIC_ACT_RELU, "linear_forward: act=%d (NONE or RELU)", act);
    HESIC_CHECK_ARG(ws_bytes >= hesic_linear_forward_ws_bytes(B, In, Out), "linear_forward: workspace of %zu bytes, need %zu", ws_bytes,
                    hesic_linear_forward_ws_bytes(B, In, Out));
    const int KB = lin_fwd_kb(In), S = (In + KB - 1) / KB, Outp = lin_fwd_outp(Out);
    HESIC_CHECK_ARG(S <= 65535, "linear_forward: In=%d too large (%d slices of %d)", In, S, KB);
    const hipStream_t st = (hipStream_t)stream;
    const dim3 grid(Outp / LIN_FWD_OUT, S);
    const int fgrid = grid_for((int64_t)B * Out, 256);
    if (dtype == HESIC_H16) {
        LINEAR_LAUNCH(linear_fwd_kernel, h16_t, grid, (const h16_t*)x, W, (float*)ws, B, In, Out, Outp, KB);
        hipLaunchKernelGGL(linear_fwd_finish_kernel<h16_t>, dim3(fgrid), dim3(256), 0, st, (const float*)ws, bias, (h16_t*)y, B, Out, Outp, S, act);
    } else {
        LINEAR_LAUNCH(linear_fwd_kernel, float, grid, (const float*)x, W, (float*)ws, B, In, Out, Outp, KB);
        hipLaunchKernelGGL(linear_fwd_finish_kernel<float>, dim3(fgrid), dim3(256), 0, st, (const float*)ws, bias, (float*)y, B, Out, Outp, S, act);
    }
    HESIC_LAUNCH_RETURN("linear_forward");
}

extern "C" int hesic_linear_dgrad(const void* gy, const float* W, void* gx, int B, int In, int Out, int dtype, void* stream) {
    if (int rc = linear_check("linear_dgrad", B, In, Out, dtype)) return rc;
    HESIC_CHECK_ARG(gy && W && gx, "linear_dgrad: null pointer");
    const hipStream_t st = (hipStream_t)stream;
    const dim3 grid((In + 63) / 64);
    if (dtype == HESIC_H16) {
        LINEAR_LAUNCH(linear_dgrad_kernel, h16_t, grid, (const h16_t*)gy, W, (h16_t*)gx, B, In, Out);
    } else {
        LINEAR_LAUNCH(linear_dgrad_kernel, float, grid, (const float*)gy, W, (float*)gx, B, In, Out);
    }
    HESIC_LAUNCH_RETURN("linear_dgrad");
}

extern "C" int hesic_linear_wgrad(const void* x, const void* gy, float* dW, float* db, int B, int In, int Out, int accumulate, int dtype,
                                  void* stream) {
    if (int rc = linear_check("linear_wgrad", B, In, Out, dtype)) return rc;
    HESIC_CHECK_ARG(x && gy && dW, "linear_wgrad: null pointer");
    const hipStream_t st = (hipStream_t)stream;
    const dim3 grid((Out + LIN_WG_OUT - 1) / LIN_WG_OUT, (In + 64 * LIN_WG_CHUNKS - 1) / (64 * LIN_WG_CHUNKS));
    HESIC_CHECK_ARG(grid.y <= 65535, "linear_wgrad: In=%d too large", In);
    if (dtype == HESIC_H16) {
        LINEAR_LAUNCH(linear_wgrad_kernel, h16_t, grid, (const h16_t*)x, (const h16_t*)gy, dW, db, B, In, Out, accumulate);
    } else {
        LINEAR_LAUNCH(linear_wgrad_kernel, float, grid, (const float*)x, (const float*)gy, dW, db, B, In, Out, accumulate);
    }
    HESIC_LAUNCH_RETURN("linear_wgrad");
}

extern "C" int hesic_bias_grad(const void* gy, float* db, float* ws, int64_t P, int C, int accumulate, int dtype, void* stream) {
    HESIC_CHECK_ARG(gy && db && ws, "bias_grad: null pointer");
    HESIC_CHECK_ARG(P > 0 && C > 0 && C <= 256 && 256 % C == 0, "bias_grad: bad sizes P=%lld C=%d (C must divide 256)", (long long)P, C);
    HESIC_CHECK_ARG(dtype == HESIC_H16 || dtype == HESIC_F32, "bias_grad: bad dtype");
    const hipStream_t st = (hipStream_t)stream;
    int64_t chunk;
    const int nb = det_blocks(P, &chunk);
    if (dtype == HESIC_H16)
        hipLaunchKernelGGL(bias_grad_partial_kernel<h16_t>, dim3(nb), dim3(256), 0, st, (const h16_t*)gy, ws, P, C, chunk);
    else
        hipLaunchKernelGGL(bias_grad_partial_kernel<float>, dim3(nb), dim3(256), 0, st, (const float*)gy, ws, P, C, chunk);
    hipLaunchKernelGGL(det_finish_kernel, dim3((C + 255) / 256), dim3(256), 0, st, (const float*)ws, db, C, nb, accumulate);
    HESIC_LAUNCH_RETURN("bias_grad");
}

extern "C" int hesic_narrow_in_wgrad(const float* x, const void* gy, float* dW, float* ws, int B, int Cin, int H, int W, int Cout,
                                     int accumulate, int dtype, void* stream) {
    HESIC_CHECK_ARG(x && gy && dW && ws, "narrow_in_wgrad: null pointer");
    HESIC_CHECK_ARG(B > 0 && H > 0 && W > 0 && Cout > 0 && Cout <= 256 && 256 % Cout == 0, "narrow_in_wgrad: bad sizes B=%d H=%d W=%d Cout=%d", B, H,
                    W, Cout);
    HESIC_CHECK_ARG(Cin == 2, "narrow_in_wgrad: Cin=%d (2: the patch pair of HomographyNet)", Cin);
    HESIC_CHECK_ARG(dtype == HESIC_H16 || dtype == HESIC_F32, "narrow_in_wgrad: bad dtype");
    const hipStream_t st = (hipStream_t)stream;
    int64_t chunk;
    const int nb = det_blocks((int64_t)B * H * W, &chunk), n = Cout * Cin * 9;
    if (dtype == HESIC_H16)
        hipLaunchKernelGGL((narrow_in_wgrad_partial_kernel<h16_t, 2>), dim3(nb), dim3(256), 0, st, x, (const h16_t*)gy, ws, B, H, W, Cout, chunk);
    else
        hipLaunchKernelGGL((narrow_in_wgrad_partial_kernel<float, 2>), dim3(nb), dim3(256), 0, st, x, (const float*)gy, ws, B, H, W, Cout, chunk);
    hipLaunchKernelGGL(det_finish_kernel, dim3((n + 255) / 256), dim3(256), 0, st, (const float*)ws, dW, n, nb, accumulate);
    HESIC_LAUNCH_RETURN("narrow_in_wgrad");
}

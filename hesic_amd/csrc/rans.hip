// Device rANS coder for batches of independent streams (include/hesic_rans.h): the z strings of HSIC / HSICJoint.compress_batch and
// decompress_batch(z_coder="device").  Byte for byte the host coder of host/hesic_host.cpp (hesic_rans_encoder_push / _flush,
// hesic_rans_decoder_decode); tests/test_gpu_rans_device.py holds both directions to it.
// One stream is one serial state machine, so a stream is latency-bound by construction; everything that is not the state recurrence is
// kept out of the chain:
//   encode  rans_itemise_kernel   one lane per symbol of the batch: v = symbol - offset, the escape decision and raw, the modelled
//                                 (start, freq - 1) of the row, the nibble count; z_hat = float(symbol) + median on the way (9 bytes / symbol)
//           rans_fold_kernel      one wave per stream: the items of 64 symbols in the lanes' registers (the next 64 already in flight),
//                                 1 / freq formed by all lanes at once, then the backward walk -- lane j's item by v_readlane, the
//                                 state update, the emitted word stored by lane 0 DOWNWARDS from the end of the slot, so the finished
//                                 stream is contiguous and in final order
//           rans_compact_kernel   the ends of the slots -> one dense payload
//   decode  rans_decode_kernel    one wave per stream: the row in registers (KPL entries per lane, reloaded when the row index changes),
//                                 the search by ballot + popcount, start / next by v_readlane, the division-free state update, the
//                                 stream's words 64 at a time in a register (the next 64 in flight), the decoded symbols gathered in the
//                                 lanes and stored 64 at a time
// x / freq of the encoder: the compiler's 64-bit division is ~100 dependent instructions.  Here q = floor(double(x) * (1.0 / freq)) is
// within one of the quotient (x < 2^63, q < 2^47: the three roundings err by < 2^-4 in all), and one remainder check makes it exact.
#include "common.h"
#include "../../include/hesic_rans.h"

#ifndef HESIC_RANS_PLAIN_DIV
#define HESIC_RANS_PLAIN_DIV 0    /* A/B builds only (-DHESIC_RANS_PLAIN_DIV=1): the compiler's 64-bit division in the fold */
#endif

namespace {

constexpr int kPrecision = 16, kBypassBits = 4;
constexpr uint64_t kLow = 1ull << 31;
constexpr uint32_t ITEM_BAD = 0xff;          // flag byte: 0 modelled only, 1 + nib an escape of nib data nibbles, ITEM_BAD see HESIC_RANS_BAD_TABLE

__device__ __forceinline__ uint32_t lane_u32(uint32_t v, int l) { return (uint32_t)__builtin_amdgcn_readlane((int)v, l); }
__device__ __forceinline__ double lane_f64(double v, int l) {
    return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(v), l), __builtin_amdgcn_readlane(__double2loint(v), l));
}

__device__ __forceinline__ void st_z(void* z, int64_t i, int dtype, float v) {
    // the bare conversion (no saturation): what tensor.to(float16 / bfloat16) yields
    if (dtype == HESIC_H16) ((h16_t*)z)[i] = (h16_t)(pack_h2_raw(v, 0.f) & 0xffffu);
    else ((float*)z)[i] = v;
}

// ------------------------------------------------------------------------------------------------------------------ encode
__global__ __launch_bounds__(256) void rans_itemise_kernel(const int32_t* __restrict__ symbols, int64_t sb, int64_t sc, int64_t sp, int64_t total,
                                                           uint32_t n, uint32_t P, const int32_t* __restrict__ indexes, int64_t index_stride,
                                                           const int32_t* __restrict__ cdfs, int ncdf, int cdf_stride,
                                                           const int32_t* __restrict__ sizes, const int32_t* __restrict__ offsets,
                                                           uint2* __restrict__ items, uint8_t* __restrict__ flags,
                                                           const float* __restrict__ medians, void* __restrict__ z_hat, int z_dtype) {
    for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (int64_t)gridDim.x * blockDim.x) {
        const int64_t b = e / n;
        const uint32_t i = (uint32_t)(e - b * n), c = i / P, p = i - c * P;
        const int64_t at = b * sb + (int64_t)c * sc + (int64_t)p * sp;
        const int32_t sym = symbols[at];
        const int32_t ci = indexes ? indexes[b * index_stride + i] : (int32_t)c;
        uint2 item = make_uint2(0u, 0u);
        uint32_t flag = ITEM_BAD;
        const int32_t size = (ci >= 0 && ci < ncdf) ? sizes[ci] : 0;
        if (size >= 2 && size <= cdf_stride) {
            const int32_t* cdf = cdfs + (int64_t)ci * cdf_stride;
            const int32_t last = size - 2;
            int32_t v = (int32_t)((uint32_t)sym - (uint32_t)offsets[ci]);
            uint32_t raw = 0;
            flag = 0;
            if (v < 0) { raw = ~((uint32_t)v << 1); v = last; }                       // -2 v - 1: odd => below the support
            else if (v >= last) { raw = (uint32_t)(v - last) << 1; v = last; }        // even => at / above it
            if (v == last) {
                uint32_t nib = 0;
                while (nib < 8 && (raw >> (nib * kBypassBits)) != 0) ++nib;
                flag = 1 + nib;
            }
            // freq - 1 in 16 bits: a row that is its escape bin only has the frequency 2^16 (the state update is then the identity)
            const uint32_t start = (uint32_t)cdf[v] & 0xffffu, freq = (uint32_t)(cdf[v + 1] - cdf[v]);
            if (freq == 0 || freq > 65536u) flag = ITEM_BAD;
            item = make_uint2(start | ((freq - 1) << 16), raw);
            if (medians) st_z(z_hat, at, z_dtype, (float)sym + medians[ci]);
        }
        items[e] = item;
        flags[e] = (uint8_t)flag;
    }
}

// x = floor(x / f), r = x % f, with inv = 1.0 / f (see the head of the file)
__device__ __forceinline__ void divmod_exact(uint64_t x, uint32_t f, double inv, uint64_t& q, uint32_t& r) {
#if HESIC_RANS_PLAIN_DIV
    q = x / f;
    r = (uint32_t)(x % f);
    return;
#endif
    uint64_t qe = (uint64_t)((double)x * inv);
    int64_t rr = (int64_t)(x - qe * f);
    if (rr < 0) { --qe; rr += f; }
    else if (rr >= (int64_t)f) { ++qe; rr -= f; }
    q = qe;
    r = (uint32_t)rr;
}

__global__ __launch_bounds__(64) void rans_fold_kernel(const uint2* __restrict__ items, const uint8_t* __restrict__ flags, uint32_t n,
                                                       uint8_t* __restrict__ slots, int64_t slot_bytes, int32_t* __restrict__ counts,
                                                       int32_t* __restrict__ status) {
    const int b = blockIdx.x, lane = threadIdx.x;
    const uint2* it = items + (int64_t)b * n;
    const uint8_t* fl = flags + (int64_t)b * n;
    uint32_t* words = reinterpret_cast<uint32_t*>(slots + (int64_t)b * slot_bytes);
    const int64_t slot_words = slot_bytes / 4;
    int64_t wp = slot_words;                         // the stream so far is words[wp .. slot_words)
    uint64_t x = kLow;
    int st = 0;
    // x >= x_max: emit the low word
    auto emit = [&]() {
        if (wp == 0) { st |= HESIC_RANS_OVERFLOW; return; }
        --wp;
        if (lane == 0) words[wp] = (uint32_t)x;
        x >>= 32;
    };
    auto put_bits = [&](uint32_t val) {
        if (x >= (1ull << 59)) emit();               // ((kLow >> 16) << 32) << (16 - 4)
        x = (x << kBypassBits) | val;
    };
    auto load = [&](int64_t ck, uint2& a, uint32_t& f) {
        const int64_t i = ck * 64 + lane;
        a = make_uint2(0u, 0u);
        f = 0;
        if (i < n) { a = it[i]; f = fl[i]; }
    };
    const int64_t nchunks = ((int64_t)n + 63) / 64;
    uint2 a, na;
    uint32_t f, nf;
    load(nchunks - 1, a, f);
    for (int64_t ck = nchunks - 1; ck >= 0 && !st; --ck) {
        na = make_uint2(0u, 0u);
        nf = 0;
        if (ck > 0) load(ck - 1, na, nf);            // in flight during the walk below
        const double inv_l = 1.0 / (double)((a.x >> 16) + 1u);
        const int cnt = (int)(((int64_t)n - ck * 64) < 64 ? ((int64_t)n - ck * 64) : 64);
        for (int j = cnt - 1; j >= 0 && !st; --j) {
            const uint32_t sf = lane_u32(a.x, j), raw = lane_u32(a.y, j), flag = lane_u32(f, j);
            const double inv = lane_f64(inv_l, j);
            if (flag == ITEM_BAD) { st |= HESIC_RANS_BAD_TABLE; break; }
            if (flag) {
                // pushed as: count nibble, data nibbles lowest first -- folded in reverse
                const int nib = (int)flag - 1;
                for (int k = nib - 1; k >= 0; --k) put_bits((raw >> (k * kBypassBits)) & 15u);
                put_bits((uint32_t)nib);
            }
            const uint32_t start = sf & 0xffffu, freq = (sf >> 16) + 1u;
            if (x >= ((uint64_t)freq << 47)) emit();             // ((kLow >> 16) << 32) * freq
            uint64_t q;
            uint32_t r;
            divmod_exact(x, freq, inv, q, r);
            x = (q << kPrecision) + r + start;
        }
        a = na;
        f = nf;
    }
    if (!st) {
        // the flush: (x >> 32) is pushed first, x last, and the stream is the pushes reversed
        if (wp < 2) st |= HESIC_RANS_OVERFLOW;
        else {
            wp -= 2;
            if (lane == 0) { words[wp] = (uint32_t)x; words[wp + 1] = (uint32_t)(x >> 32); }
        }
    }
    if (lane == 0) {
        counts[b] = st ? 0 : (int32_t)((slot_words - wp) * 4);
        status[b] = st;
    }
}

__global__ __launch_bounds__(256) void rans_compact_kernel(const uint8_t* __restrict__ slots, int64_t slot_bytes, const int32_t* __restrict__ counts,
                                                           const int64_t* __restrict__ offsets, uint8_t* __restrict__ out, int64_t out_bytes) {
    const int64_t t = blockIdx.x;
    int64_t n = counts[t];
    const int64_t off = offsets[t];
    if (n < 0) n = 0;
    if (n > slot_bytes) n = slot_bytes;
    const uint8_t* src = slots + t * slot_bytes + (slot_bytes - n);      // the stream is the END of its slot
    if (off < 0 || off > out_bytes) return;
    if (off + n > out_bytes) n = out_bytes - off;
    for (int64_t i = threadIdx.x; i < n; i += blockDim.x) out[off + i] = src[i];
}

// ------------------------------------------------------------------------------------------------------------------ decode
template <int KPL>
__global__ __launch_bounds__(64) void rans_decode_kernel(const uint8_t* __restrict__ data, int64_t n_bytes, const int64_t* __restrict__ data_offsets,
                                                         const int32_t* __restrict__ counts, uint32_t n, uint32_t P,
                                                         const int32_t* __restrict__ indexes, int64_t index_stride,
                                                         const int32_t* __restrict__ cdfs, int ncdf, int cdf_stride,
                                                         const int32_t* __restrict__ sizes, const int32_t* __restrict__ offsets,
                                                         int32_t* __restrict__ symbols_out, int64_t sb, int64_t sc, int64_t sp,
                                                         const float* __restrict__ medians, void* __restrict__ z_hat, int z_dtype,
                                                         int32_t* __restrict__ status) {
    const int b = blockIdx.x, lane = threadIdx.x;
    const int64_t off = data_offsets[b], nb = counts[b];
    if (nb < 8 || (nb & 3) || off < 0 || (off & 3) || off > n_bytes || nb > n_bytes - off) {
        if (lane == 0) status[b] = HESIC_RANS_BAD_STREAM;
        return;
    }
    const uint32_t* words = reinterpret_cast<const uint32_t*>(data + off);
    const int64_t nw = nb / 4;
    auto ld_words = [&](int64_t base) -> uint32_t {
        const int64_t i = base + lane;
        return i < nw ? words[i] : 0u;               // past the end of the stream: zeros, as next_word
    };
    int64_t wbase = 0, pos = 2;
    uint32_t wbuf = ld_words(0), wnxt = ld_words(64);
    uint64_t x = (uint64_t)lane_u32(wbuf, 0) | ((uint64_t)lane_u32(wbuf, 1) << 32);
    auto next_word = [&]() -> uint32_t {
        if (pos - wbase >= 64) {
            wbuf = wnxt;
            wbase += 64;
            wnxt = ld_words(wbase + 64);             // in flight while the 64 words of wbuf are consumed
        }
        const uint32_t w = lane_u32(wbuf, (int)(pos - wbase));
        ++pos;
        return w;
    };
    auto get_bits = [&]() -> uint32_t {
        const uint32_t v = (uint32_t)x & 15u;
        x >>= kBypassBits;
        if (x < kLow) x = (x << 32) | next_word();
        return v;
    };

    int st = 0;
    int32_t cur = 0, last = 0, size = 0;
    bool loaded = false;                             // no value of an index entry can stand for "no row yet": -1 is one a caller can pass
    uint32_t off_ci = 0;
    uint32_t row[KPL];
#pragma unroll
    for (int k = 0; k < KPL; ++k) row[k] = 0xffffffffu;
    const int64_t idx_base = (int64_t)b * index_stride;

    for (int64_t i0 = 0; i0 < n && !st; i0 += 64) {
        const uint32_t il = (uint32_t)i0 + lane;                 // this lane's symbol of the chunk
        const bool have = il < n;
        const uint32_t c_l = have ? il / P : 0u;
        const int32_t ci_l = have ? (indexes ? indexes[idx_base + il] : (int32_t)c_l) : 0;
        const int cnt = (int)(((int64_t)n - i0) < 64 ? ((int64_t)n - i0) : 64);
        int32_t out_l = 0;
        for (int j = 0; j < cnt; ++j) {
            const int32_t ci = (int32_t)lane_u32((uint32_t)ci_l, j);
            if (!loaded || ci != cur) {
                size = (ci >= 0 && ci < ncdf) ? sizes[ci] : 0;
                if (size < 2 || size > cdf_stride) { st |= HESIC_RANS_BAD_TABLE; break; }
                const int32_t* cdf = cdfs + (int64_t)ci * cdf_stride;
#pragma unroll
                for (int k = 0; k < KPL; ++k) {
                    const int e = lane + 64 * k;
                    row[k] = e < size ? (uint32_t)cdf[e] : 0xffffffffu;       // beyond the row: never <= slot
                }
                cur = ci;
                loaded = true;
                last = size - 2;
                off_ci = (uint32_t)offsets[ci];
            }
            const uint32_t slot = (uint32_t)x & 0xffffu;
            int s = -1;
#pragma unroll
            for (int k = 0; k < KPL; ++k) s += __popcll(__ballot(row[k] <= slot));
            s = s < 0 ? 0 : (s > last ? last : s);               // acts on damaged tables only: cdf[0] = 0 <= slot < cdf[size - 1]
            uint32_t start = 0, next = 0;
#pragma unroll
            for (int k = 0; k < KPL; ++k) {
                const uint32_t u = lane_u32(row[k], s & 63), w = lane_u32(row[k], (s + 1) & 63);
                if (k == (s >> 6)) start = u;
                if (k == ((s + 1) >> 6)) next = w;
            }
            x = (uint64_t)(next - start) * (x >> kPrecision) + slot - start;
            if (x < kLow) x = (x << 32) | next_word();
            int32_t v = s;
            if (s == last) {
                uint32_t c = get_bits(), nib = c;
                while (c == 15u && nib <= 8u) { c = get_bits(); nib += c; }
                if (nib > 8u) { st |= HESIC_RANS_BAD_ESCAPE; break; }        // the host would shift by >= 32 here
                uint32_t raw = 0;
                for (uint32_t k = 0; k < nib; ++k) raw |= get_bits() << (k * kBypassBits);
                const uint32_t h = raw >> 1;
                v = (int32_t)((raw & 1u) ? ~h : h + (uint32_t)last);         // -h - 1 below the support, h + last at / above it
            }
            const int32_t sym = (int32_t)((uint32_t)v + off_ci);
            if (lane == j) out_l = sym;
        }
        if (st) break;
        if (have) {
            const uint32_t p_l = il - c_l * P;
            const int64_t at = (int64_t)b * sb + (int64_t)c_l * sc + (int64_t)p_l * sp;
            if (symbols_out) symbols_out[at] = out_l;
            if (medians) st_z(z_hat, at, z_dtype, (float)out_l + medians[ci_l]);   // every index of the chunk went through the row check (a bad one ends the stream above)
        }
    }
    if (lane == 0) status[b] = st;
}

int check_tables(const char* who, int64_t n_streams, int64_t n, int64_t P, const int32_t* cdfs, int ncdf, int cdf_stride, const int32_t* sizes,
                 const int32_t* offsets, const int32_t* indexes, int64_t index_stride, const float* medians, const void* z_hat, int z_dtype) {
    HESIC_CHECK_ARG(n_streams > 0 && n_streams < (1 << 20) && n > 0 && n < (1ll << 31) && P > 0 && P <= n && n % P == 0 &&
                    n_streams * n < (1ll << 40), "%s: bad geometry (n_streams %lld, n %lld = C * P, P %lld)", who, (long long)n_streams,
                    (long long)n, (long long)P);
    HESIC_CHECK_ARG(cdfs && sizes && offsets && ncdf > 0, "%s: null table", who);
    HESIC_CHECK_ARG(cdf_stride >= 2 && cdf_stride <= HESIC_RANS_MAX_ROW, "%s: rows of %d entries, the coder holds up to %d", who, cdf_stride,
                    HESIC_RANS_MAX_ROW);
    HESIC_CHECK_ARG(indexes ? (index_stride == 0 || index_stride == n) : n / P <= ncdf,
                    "%s: index_stride must be 0 or n; without indexes the table needs a row per channel", who);
    HESIC_CHECK_ARG(!medians == !z_hat, "%s: medians and z_hat go together", who);
    HESIC_CHECK_ARG(!medians || z_dtype == HESIC_F32 || z_dtype == HESIC_H16, "%s: bad z_hat dtype", who);
    return 0;
}

}  // namespace

extern "C" int64_t hesic_rans_slot_bytes(int64_t n) { return n < 0 ? -1 : 8 * n + 16; }
extern "C" int64_t hesic_rans_encode_ws_bytes(int64_t n_streams, int64_t n) {
    return (n_streams < 0 || n < 0) ? -1 : ((n_streams * n * 9 + 7) & ~7ll);
}

extern "C" int hesic_rans_encode(const int32_t* symbols, int64_t sb, int64_t sc, int64_t sp, int n_streams, int64_t n, int64_t P,
                                 const int32_t* indexes, int64_t index_stride, const int32_t* cdfs, int ncdf, int cdf_stride,
                                 const int32_t* sizes, const int32_t* offsets, void* ws, int64_t ws_bytes, uint8_t* slots, int64_t slot_bytes,
                                 int32_t* counts, int32_t* status, const float* medians, void* z_hat, int z_dtype, void* stream) {
    if (int e = check_tables("rans_encode", n_streams, n, P, cdfs, ncdf, cdf_stride, sizes, offsets, indexes, index_stride, medians, z_hat, z_dtype))
        return e;
    HESIC_CHECK_ARG(symbols && ws && slots && counts && status, "rans_encode: null pointer");
    HESIC_CHECK_ARG(ws_bytes >= hesic_rans_encode_ws_bytes(n_streams, n) && ((uintptr_t)ws & 7) == 0,
                    "rans_encode: workspace of %lld bytes, %lld needed (8-byte aligned)", (long long)ws_bytes,
                    (long long)hesic_rans_encode_ws_bytes(n_streams, n));
    HESIC_CHECK_ARG(slot_bytes >= hesic_rans_slot_bytes(n) && slot_bytes % 4 == 0 && ((uintptr_t)slots & 3) == 0,
                    "rans_encode: slots of %lld bytes, a stream needs %lld (whole 32-bit words)", (long long)slot_bytes,
                    (long long)hesic_rans_slot_bytes(n));
    const int64_t total = (int64_t)n_streams * n;
    uint2* items = (uint2*)ws;
    uint8_t* flags = (uint8_t*)ws + total * 8;
    hipLaunchKernelGGL(rans_itemise_kernel, dim3(grid_for(total, 256)), dim3(256), 0, (hipStream_t)stream, symbols, sb, sc, sp, total, (uint32_t)n,
                       (uint32_t)P, indexes, index_stride, cdfs, ncdf, cdf_stride, sizes, offsets, items, flags, medians, z_hat, z_dtype);
    hipLaunchKernelGGL(rans_fold_kernel, dim3(n_streams), dim3(64), 0, (hipStream_t)stream, items, flags, (uint32_t)n, slots, slot_bytes, counts,
                       status);
    HESIC_LAUNCH_RETURN("rans_encode");
}

extern "C" int hesic_rans_compact(const uint8_t* slots, int64_t slot_bytes, const int32_t* counts, const int64_t* out_offsets, int n_streams,
                                  uint8_t* out, int64_t out_bytes, void* stream) {
    HESIC_CHECK_ARG(slots && counts && out_offsets && slot_bytes > 0 && n_streams > 0 && out_bytes >= 0 && (out || out_bytes == 0),
                    "rans_compact: bad arguments");
    if (out_bytes == 0) return 0;
    hipLaunchKernelGGL(rans_compact_kernel, dim3(n_streams), dim3(256), 0, (hipStream_t)stream, slots, slot_bytes, counts, out_offsets, out,
                       out_bytes);
    HESIC_LAUNCH_RETURN("rans_compact");
}

extern "C" int hesic_rans_decode(const uint8_t* data, int64_t n_bytes, const int64_t* data_offsets, const int32_t* counts, int n_streams, int64_t n,
                                 int64_t P, const int32_t* indexes, int64_t index_stride, const int32_t* cdfs, int ncdf, int cdf_stride,
                                 const int32_t* sizes, const int32_t* offsets, int32_t* symbols_out, int64_t sb, int64_t sc, int64_t sp,
                                 const float* medians, void* z_hat, int z_dtype, int32_t* status, void* stream) {
    if (int e = check_tables("rans_decode", n_streams, n, P, cdfs, ncdf, cdf_stride, sizes, offsets, indexes, index_stride, medians, z_hat, z_dtype))
        return e;
    HESIC_CHECK_ARG(data && n_bytes >= 0 && data_offsets && counts && status && ((uintptr_t)data & 3) == 0,
                    "rans_decode: null or misaligned pointer");
    HESIC_CHECK_ARG(symbols_out || z_hat, "rans_decode: no output");
    const int kpl = (cdf_stride + 63) / 64;
#define HESIC_RANS_DECODE(K)                                                                                                                       \
    hipLaunchKernelGGL(rans_decode_kernel<K>, dim3(n_streams), dim3(64), 0, (hipStream_t)stream, data, n_bytes, data_offsets, counts, (uint32_t)n,  \
                       (uint32_t)P, indexes, index_stride, cdfs, ncdf, cdf_stride, sizes, offsets, symbols_out, sb, sc, sp, medians, z_hat,         \
                       z_dtype, status)
    if (kpl <= 1) HESIC_RANS_DECODE(1);
    else if (kpl <= 2) HESIC_RANS_DECODE(2);
    else if (kpl <= 4) HESIC_RANS_DECODE(4);
    else HESIC_RANS_DECODE(8);
#undef HESIC_RANS_DECODE
    HESIC_LAUNCH_RETURN("rans_decode");
}

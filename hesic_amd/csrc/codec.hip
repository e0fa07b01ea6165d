// Device-resident range coder for the HESIC latents (include/hesic_codec.h): HSIC.compress_batch / decompress_batch.
// The per-pair path (HSIC.compress) forms a full cumulative-frequency table per latent element on the device -- (2 minmax + 2) * 4 bytes
// for a symbol that codes to about one byte --, ships the tables to the host and walks them with one thread.  Here the rows never leave
// the chip:
//   encode  rc_ranges_kernel      one wave per (image, coded channel, pixel): the row of hesic_gmm_cdf in LDS, and of it only the triple
//                                 (c[s], c[s+1] - c[s], c[A]) of the symbol that is coded (12 bytes)
//           rc_encode_kernel      one lane per stream: the host coder's state machine over the stream's triples, bytes into its own slot
//           rc_compact_kernel     slots -> one dense payload (offsets = exclusive scan of the byte counts)
//   decode  rc_decode_kernel      one wave per stream: per symbol the row in LDS, a wave scan to cumulative counts, the search by
//                                 ballot / popcount, the state update; the symbol goes straight into the channels-last y_hat
// Rows of up to 64 symbols (a trained model's) spread their A * K mixture terms over the whole wave (rc_fill_row_small).
// HESIC+ (HSICJoint.compress_batch / decompress_batch) codes the same streams in wavefront order, pixel-major:
//   encode  rc_encode_ordered_kernel   rc_encode_kernel's loop over the triples of the whole maps, walked through a pixel permutation
//   decode  joint_gather_batch_kernel  the 5 x 5 crops and feature rows of one wavefront group of every image of the batch
//           rc_decode_step_kernel      rc_decode_kernel cut at group boundaries: coder state in device memory, symbols straight into the
//                                      padded latent maps the next group's crops are cut from
// The rows are formed by the expressions of gmm_cdf.h, the ones the table kernels of entropy.hip evaluate: a stream coded here decodes
// with the host coder over hesic_gmm_cdf's tables and the other way round (tests/test_gpu_device_codec.py holds both to that).
#include "common.h"
#include "gmm_cdf.h"
#include "../../include/hesic_codec.h"

namespace {

constexpr uint64_t RC_TOP = 1ull << 56, RC_BOT = 1ull << 48;
static_assert(HESIC_CODEC_MAX_ALPHABET == CDF_WAVE_MAX, "the coder's rows are the wave table kernel's rows");

__device__ __forceinline__ uint32_t wave_sum_u32(uint32_t v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += (uint32_t)__shfl_xor((int)v, o, 64);
    return v;
}

// The row's clipped pmf into frow (LDS, one wave), as gmm_cdf_wave_kernel fills it; returns numpy's pairwise sum of the row.
__device__ __forceinline__ float rc_fill_row(const float* mu, const float* sg, const float* wk, int K, int A, float* frow, int lane) {
    for (int s = lane; s < A; s += 64) frow[s] = cdf_pm(s, mu, sg, wk, K);
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    return np_pairwise_sum(frow, A);
}

// Small alphabets (A <= RC_SMALL_A; a trained model's minmax is ~10, A = 21): with one symbol per lane a third of the wave would walk
// the K mixtures serially.  Here the A * K terms Phi(..) - Phi(..) are spread over all lanes (each term is cdf_pm's expression for its
// (s, k), evaluated alone), staged in LDS, and lane s then accumulates its K terms in cdf_pm's order: pm = fma(term_k, w_k, pm), the
// contraction the compiler applies to cdf_pm's `pm += term * w` (held to the tables bit for bit by tests/test_gpu_device_codec.py).
// raw: lane k < K holds the mean of mixture k, lane K + k its scale, as loaded.
constexpr int RC_SMALL_A = 64, RC_TERMS = RC_SMALL_A * GMM_MAXK;
__device__ __forceinline__ float rc_fill_row_small(float raw, const float* wk, int K, int A, int minmax, float scale_bound, float* frow,
                                                   float* terms, int lane) {
    const int n = A * K;
    for (int t0 = 0; t0 < n; t0 += 64) {
        const int t = t0 + lane, tc = t < n ? t : n - 1;          // every lane takes part in the shuffles
        const int s = tc / K, k = tc - s * K;
        const float mu = __shfl(raw, k, 64) + (float)minmax;
        const float sg = fmaxf(__shfl(raw, K + k, 64), scale_bound);
        const float a = fabsf((float)s - mu);
        const float term = phi_cdf((0.5f - a) / sg) - phi_cdf((-0.5f - a) / sg);
        if (t < n) terms[t] = term;
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    if (lane < A) {
        float pm = 0.f;
        for (int k = 0; k < K; ++k) pm = __fmaf_rn(terms[lane * K + k], wk[k], pm);
        frow[lane] = fminf(fmaxf(pm, 1.0f / 65536.0f), 1.0f);
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    return np_pairwise_sum(frow, A);
}

// The mixture of (image b, pixel hw, channel m) as gmm_cdf_wave_kernel loads it, then the row.
template <typename T>
__device__ __forceinline__ float rc_row(const hesic_gmm_desc& d, int b, int hw, int m, int minmax, const T* __restrict__ scales,
                                        const T* __restrict__ means, const float* __restrict__ weights, float* frow, int lane) {
    const int64_t sm = ((int64_t)b * d.HW + hw) * d.sm_pix_stride + m;
    float mu[GMM_MAXK], sg[GMM_MAXK], wk[GMM_MAXK];
    for (int k = 0; k < d.K; ++k) {
        mu[k] = elem<T>::ld(means + sm + d.m_c_off + k * d.M) + (float)minmax;
        sg[k] = fmaxf(elem<T>::ld(scales + sm + d.s_c_off + k * d.M), d.scale_bound);
        wk[k] = weights ? weights[(int64_t)b * d.K * d.M + k * d.M + m] : 1.f;
    }
    return rc_fill_row(mu, sg, wk, d.K, 2 * minmax + 1, frow, lane);
}

// quantised frequency of a row entry: the expression of the table kernels
__device__ __forceinline__ uint32_t rc_freq(float pm, float tot) { return (uint32_t)rintf(pm / tot * 65536.0f); }

template <typename T>
__global__ __launch_bounds__(256) void rc_ranges_kernel(const hesic_gmm_desc d, const T* __restrict__ scales, const T* __restrict__ means,
                                                        const float* __restrict__ weights, const void* __restrict__ yhat, int y_dtype,
                                                        const int32_t* __restrict__ meta, int32_t* __restrict__ triples) {
    __shared__ float buf[4][CDF_WAVE_MAX];
    __shared__ float tbuf[4][RC_TERMS];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    float* frow = buf[wave];
    const int64_t per_img = (int64_t)d.M * d.HW, total = per_img * d.B;
    for (int64_t i = blockIdx.x * 4ll + wave; i < total; i += (int64_t)gridDim.x * 4) {
        const int b = (int)(i / per_img);
        const int r = (int)(i - (int64_t)b * per_img);
        const int j = r / d.HW, hw = r - j * d.HW;
        const int32_t* mt = meta + (int64_t)b * (d.M + 2);
        const int n_ch = mt[0], minmax = mt[1];
        if (j >= n_ch || minmax < 1 || 2 * minmax + 1 > CDF_WAVE_MAX) continue;       // wave-uniform
        const int m = mt[2 + j];
        int32_t* out = triples + i * 3;
        if ((unsigned)m >= (unsigned)d.M) {                 // a damaged channel list: frequency 0, which the stream coder reports
            if (lane < 3) out[lane] = 0;
            continue;
        }
        const int A = 2 * minmax + 1;
        float tot;
        if (A <= RC_SMALL_A) {
            const int64_t sm = ((int64_t)b * d.HW + hw) * d.sm_pix_stride + m;
            float raw = 0.f, wk[GMM_MAXK];
            if (lane < 2 * d.K)
                raw = elem<T>::ld(lane < d.K ? means + sm + d.m_c_off + lane * d.M : scales + sm + d.s_c_off + (lane - d.K) * d.M);
            for (int k = 0; k < d.K; ++k) wk[k] = weights ? weights[(int64_t)b * d.K * d.M + k * d.M + m] : 1.f;
            tot = rc_fill_row_small(raw, wk, d.K, A, minmax, d.scale_bound, frow, tbuf[wave], lane);
        } else {
            tot = rc_row<T>(d, b, hw, m, minmax, scales, means, weights, frow, lane);
        }
        const int sym = (int)ld_any(yhat, ((int64_t)b * d.HW + hw) * d.M + m, y_dtype) + minmax;
        // cumulative counts are sums of integers below 2^24: the table kernels' fp32 running sums are these integer sums
        uint32_t lo = 0, fr = 0, all = 0;
        for (int s = lane; s < A; s += 64) {
            const uint32_t q = rc_freq(frow[s], tot);
            all += q;
            lo += s < sym ? q : 0u;
            fr += s == sym ? q : 0u;
        }
        lo = wave_sum_u32(lo); fr = wave_sum_u32(fr); all = wave_sum_u32(all);
        if (lane == 0) { out[0] = (int32_t)lo; out[1] = (int32_t)fr; out[2] = (int32_t)all; }
        __builtin_amdgcn_wave_barrier();          // the row buffer is rewritten by the next trip
    }
}

// hesic_rc_encoder_encode (csrc/host/hesic_host.cpp) per lane, over triples instead of table rows: stream t = (b, s) of both encoder
// kernels.  order == nullptr: the stream's triples in sequence (channel-major); else symbol i is channel i % nj of pixel order[i / nj].
__device__ __forceinline__ void rc_encode_stream(const int32_t* __restrict__ triples, const int32_t* __restrict__ meta, int t, int M, int HW, int cps,
                                                 int S, const int32_t* __restrict__ order, uint8_t* __restrict__ slots, int64_t cap,
                                                 int32_t* __restrict__ counts, int32_t* __restrict__ status) {
    const int b = t / S, s = t - b * S;
    int n_ch = meta[(int64_t)b * (M + 2)];
    n_ch = n_ch < 0 ? 0 : (n_ch > M ? M : n_ch);
    const int j0 = s * cps;
    if (j0 >= n_ch) { counts[t] = 0; return; }
    const int nj = n_ch - j0 < cps ? n_ch - j0 : cps;
    const int64_t n = (int64_t)nj * HW;
    const int32_t* tr = triples + ((int64_t)b * M + j0) * HW * 3;
    uint8_t* out = slots + (int64_t)t * cap;
    int64_t pos = 0;
    int bad = 0;
    uint64_t low = 0, range = ~0ull;
    for (int64_t i = 0; i < n && !bad; ++i) {
        int64_t e = i;
        if (order) {
            const int64_t p = i / nj;
            const int px = order[p];
            if ((unsigned)px >= (unsigned)HW) { bad = HESIC_CODEC_BAD_SYMBOL; break; }      // a damaged permutation: nothing to address
            e = (i - p * nj) * HW + px;
        }
        const uint32_t c = (uint32_t)tr[3 * e], f = (uint32_t)tr[3 * e + 1], tot = (uint32_t)tr[3 * e + 2];
        if (f == 0 || tot == 0 || (uint64_t)c + f > tot) { bad = HESIC_CODEC_BAD_SYMBOL; break; }
        range /= tot;
        low += (uint64_t)c * range;
        range *= (uint64_t)f;
        while ((low ^ (low + range)) < RC_TOP || (range < RC_BOT && ((range = (0 - low) & (RC_BOT - 1)), true))) {
            if (pos >= cap) { bad = HESIC_CODEC_OVERFLOW; break; }
            out[pos++] = (uint8_t)(low >> 56);
            low <<= 8;
            range <<= 8;
        }
    }
    if (!bad) {
        // flush: the top two bytes of low rounded up to a multiple of 2^48 (low <= v < low + range as range >= 2^48), trailing zeros dropped
        const uint64_t v = (low + (RC_BOT - 1)) & ~(RC_BOT - 1);
        const uint8_t b0 = (uint8_t)(v >> 56), b1 = (uint8_t)(v >> 48);
        const int nb = b1 ? 2 : (b0 ? 1 : 0);
        if (pos + nb > cap) bad = HESIC_CODEC_OVERFLOW;
        else {
            if (nb > 0) out[pos++] = b0;
            if (nb > 1) out[pos++] = b1;
        }
    }
    if (bad) atomicOr(status, bad);
    counts[t] = bad ? 0 : (int32_t)pos;
}

__global__ __launch_bounds__(64) void rc_encode_kernel(const int32_t* __restrict__ triples, const int32_t* __restrict__ meta, int B, int M, int HW,
                                                       int cps, int S, uint8_t* __restrict__ slots, int64_t cap, int32_t* __restrict__ counts,
                                                       int32_t* __restrict__ status) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= B * S) return;
    rc_encode_stream(triples, meta, t, M, HW, cps, S, nullptr, slots, cap, counts, status);
}

__global__ __launch_bounds__(64) void rc_encode_ordered_kernel(const int32_t* __restrict__ triples, const int32_t* __restrict__ meta, int B, int M,
                                                               int HW, int cps, int S, const int32_t* __restrict__ order,
                                                               uint8_t* __restrict__ slots, int64_t cap, int32_t* __restrict__ counts,
                                                               int32_t* __restrict__ status) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= B * S) return;
    rc_encode_stream(triples, meta, t, M, HW, cps, S, order, slots, cap, counts, status);
}

__global__ __launch_bounds__(256) void rc_compact_kernel(const uint8_t* __restrict__ slots, int64_t cap, const int32_t* __restrict__ counts,
                                                         const int64_t* __restrict__ offsets, uint8_t* __restrict__ out, int64_t out_bytes) {
    const int64_t t = blockIdx.x;
    int64_t n = counts[t];
    const int64_t off = offsets[t];
    if (n > cap) n = cap;
    if (off < 0 || off > out_bytes) return;
    if (off + n > out_bytes) n = out_bytes - off;
    const uint8_t* src = slots + t * cap;
    for (int64_t i = threadIdx.x; i < n; i += blockDim.x) out[off + i] = src[i];
}

// The coder state of one stream: what rc_decode_step_kernel keeps in device memory between the groups of a walk (4 x 8 bytes).
struct rc_coder {
    uint64_t low, range, code;
    int64_t pos;
};

__device__ __forceinline__ void rc_coder_begin(rc_coder& c, const uint8_t* __restrict__ in, int64_t len) {
    c.low = 0; c.range = ~0ull; c.code = 0; c.pos = 0;
    for (int i = 0; i < 8; ++i) { c.code = (c.code << 8) | (c.pos < len ? in[c.pos] : 0); ++c.pos; }
}

// One symbol of one stream, by the whole wave: the row of the symbol's mixture (raw: lane k < K its mean k, lane K + k its scale k, as
// loaded) in LDS, a wave scan to cumulative counts, the search by ballot / popcount, the state update with the coder's renormalisation.
// Returns the clamped symbol index; every byte read is index-checked against len.  The body of both decoder kernels.
__device__ __forceinline__ int rc_decode_symbol(float raw, const float* wk, int K, int A, int minmax, float scale_bound, float* frow, uint32_t* crow,
                                                float* terms, int lane, const uint8_t* __restrict__ in, int64_t len, rc_coder& c) {
    float tot;
    if (A <= RC_SMALL_A) {
        tot = rc_fill_row_small(raw, wk, K, A, minmax, scale_bound, frow, terms, lane);
    } else {
        float mu[GMM_MAXK], sg[GMM_MAXK];
        for (int k = 0; k < K; ++k) {
            mu[k] = __shfl(raw, k, 64) + (float)minmax;
            sg[k] = fmaxf(__shfl(raw, K + k, 64), scale_bound);
        }
        tot = rc_fill_row(mu, sg, wk, K, A, frow, lane);
    }
    uint32_t carry = 0;
    for (int s0 = 0; s0 < A; s0 += 64) {
        const int s = s0 + lane;
        uint32_t v = s < A ? rc_freq(frow[s], tot) : 0u;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const uint32_t u = (uint32_t)__shfl_up((int)v, o, 64);
            if (lane >= o) v += u;
        }
        v += carry;
        if (s < A) crow[s] = v;                      // c[s + 1]
        carry = (uint32_t)__shfl((int)v, 63, 64);
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    // hesic_rc_decoder_decode_grid's step; the guards on a zero total / zero step only act on states no valid stream reaches
    const uint64_t total = carry ? carry : 1u;
    uint64_t step = c.range / total;
    if (step == 0) step = 1;
    uint64_t v = (c.code - c.low) / step;
    if (v >= total) v = total - 1;
    // last index with c[idx] <= v: c[0] = 0 always counts, c[i] = crow[i - 1] for 1 <= i <= A - 1
    int idx = 0;
    for (int s0 = 0; s0 < A - 1; s0 += 64) {
        const int s = s0 + lane;
        idx += __popcll(__ballot(s < A - 1 && (uint64_t)crow[s] <= v));
    }
    if (idx > A - 1) idx = A - 1;
    const uint32_t c_lo = idx ? crow[idx - 1] : 0u, c_hi = crow[idx];
    c.low += (uint64_t)c_lo * step;
    c.range = step * (uint64_t)(c_hi - c_lo);
    // the coder's renormalisation; a valid state leaves it within 8 trips, the bound only ends a damaged one
    for (int it = 0; it < 16; ++it) {
        if (!((c.low ^ (c.low + c.range)) < RC_TOP || (c.range < RC_BOT && ((c.range = (0 - c.low) & (RC_BOT - 1)), true)))) break;
        c.code = (c.code << 8) | (c.pos < len ? in[c.pos] : 0);
        ++c.pos;
        c.low <<= 8;
        c.range <<= 8;
    }
    return idx;
}

template <typename T>
__global__ __launch_bounds__(256) void rc_decode_kernel(const hesic_gmm_desc d, const T* __restrict__ scales, const T* __restrict__ means,
                                                        const float* __restrict__ weights, const int32_t* __restrict__ meta, int cps, int S,
                                                        const uint8_t* __restrict__ bytes, int64_t n_bytes, const int64_t* __restrict__ offsets,
                                                        const int32_t* __restrict__ counts, void* __restrict__ yhat, int y_dtype) {
    __shared__ float buf[4][CDF_WAVE_MAX];
    __shared__ uint32_t cum[4][CDF_WAVE_MAX];
    __shared__ float tbuf[4][RC_TERMS];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    float* frow = buf[wave];
    uint32_t* crow = cum[wave];
    const int t = blockIdx.x * 4 + wave;
    if (t >= d.B * S) return;                       // everything below is wave-uniform: no block-level barrier follows
    const int b = t / S, s_idx = t - b * S;
    const int32_t* mt = meta + (int64_t)b * (d.M + 2);
    int n_ch = mt[0];
    const int minmax = mt[1];
    n_ch = n_ch < 0 ? 0 : (n_ch > d.M ? d.M : n_ch);
    const int j0 = s_idx * cps;
    if (j0 >= n_ch || minmax < 1 || 2 * minmax + 1 > CDF_WAVE_MAX) return;
    const int nj = n_ch - j0 < cps ? n_ch - j0 : cps;
    const int A = 2 * minmax + 1;
    // the stream's bytes: [off, off + len) clipped to the payload; a read at or past len yields 0 by the index check
    int64_t off = offsets[t], len = counts[t];
    if (off < 0 || off > n_bytes || len < 0) { off = 0; len = 0; }
    if (len > n_bytes - off) len = n_bytes - off;
    const uint8_t* in = bytes + off;
    rc_coder c;
    rc_coder_begin(c, in, len);
    // A stream is one serial chain of symbols, so what a symbol waits for is latency.  The 2 K parameters of a symbol are fetched by 2 K
    // lanes at once (lane k: mean k, lane K + k: scale k) ONE SYMBOL AHEAD, and handed round by shuffles: the loads of symbol i + 1 are
    // in flight while symbol i is evaluated (a run-time K loop of dependent loads per symbol cost more than the arithmetic).  The values
    // and the expressions they enter are those of rc_row.
    const int n_sym = nj * d.HW;
    auto fetch = [&](int i) -> float {
        if (i >= n_sym || lane >= 2 * d.K) return 0.f;
        const int jj = i / d.HW, hw = i - jj * d.HW;
        const int m = mt[2 + j0 + jj];
        if ((unsigned)m >= (unsigned)d.M) return 0.f;
        const int64_t sm = ((int64_t)b * d.HW + hw) * d.sm_pix_stride + m;
        const T* p = lane < d.K ? means + sm + d.m_c_off + lane * d.M : scales + sm + d.s_c_off + (lane - d.K) * d.M;
        return elem<T>::ld(p);
    };
    float nxt = fetch(0);
    float wk[GMM_MAXK];
    int cur_m = -1;
    for (int i = 0; i < n_sym; ++i) {
        const float raw = nxt;
        nxt = fetch(i + 1);
        const int jj = i / d.HW, hw = i - jj * d.HW;
        const int m = mt[2 + j0 + jj];
        if ((unsigned)m >= (unsigned)d.M) continue;          // a damaged channel list: nothing to address
        if (m != cur_m) {
            for (int k = 0; k < d.K; ++k) wk[k] = weights ? weights[(int64_t)b * d.K * d.M + k * d.M + m] : 1.f;
            cur_m = m;
        }
        const int idx = rc_decode_symbol(raw, wk, d.K, A, minmax, d.scale_bound, frow, crow, tbuf[wave], lane, in, len, c);
        if (lane == 0) st_any(yhat, ((int64_t)b * d.HW + hw) * d.M + m, y_dtype, (float)(idx - minmax));
        __builtin_amdgcn_wave_barrier();          // the row buffers are rewritten by the next symbol
    }
}

// rc_decode_kernel cut at the group boundaries of a HESIC+ wavefront walk (K = 1, fp32 (scale | mean) rows of the entropy-parameter net,
// row b * P + p for pixel p of this group in image b: d.HW = P).  One wave per stream (b, s): its coder state comes from / goes back to
// state[t] (first != 0: begun here from the stream's first 8 bytes), the P * nj symbols of the group are decoded pixel-major and written
// as symbol - minmax into row centre[p] of image b's padded latent map.  Loop counts follow from meta and P alone.
__global__ __launch_bounds__(256) void rc_decode_step_kernel(const hesic_gmm_desc d, const float* __restrict__ scales, const float* __restrict__ means,
                                                             const int32_t* __restrict__ meta, int cps, int S, const uint8_t* __restrict__ bytes,
                                                             int64_t n_bytes, const int64_t* __restrict__ offsets,
                                                             const int32_t* __restrict__ counts, uint64_t* __restrict__ state, int first,
                                                             const int32_t* __restrict__ centre, void* __restrict__ y_rows, int y_dtype,
                                                             int64_t rows_per_image) {
    __shared__ float buf[4][CDF_WAVE_MAX];
    __shared__ uint32_t cum[4][CDF_WAVE_MAX];
    __shared__ float tbuf[4][RC_SMALL_A];            // K = 1: one term per symbol
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    float* frow = buf[wave];
    uint32_t* crow = cum[wave];
    const int t = blockIdx.x * 4 + wave;
    if (t >= d.B * S) return;                       // wave-uniform from here on
    const int b = t / S, s_idx = t - b * S;
    const int32_t* mt = meta + (int64_t)b * (d.M + 2);
    int n_ch = mt[0];
    const int minmax = mt[1];
    n_ch = n_ch < 0 ? 0 : (n_ch > d.M ? d.M : n_ch);
    const int j0 = s_idx * cps;
    if (j0 >= n_ch || minmax < 1 || 2 * minmax + 1 > CDF_WAVE_MAX) return;
    const int nj = n_ch - j0 < cps ? n_ch - j0 : cps;
    const int A = 2 * minmax + 1;
    int64_t off = offsets[t], len = counts[t];
    if (off < 0 || off > n_bytes || len < 0) { off = 0; len = 0; }
    if (len > n_bytes - off) len = n_bytes - off;
    const uint8_t* in = bytes + off;
    uint64_t* sv = state + (int64_t)t * 4;
    rc_coder c;
    if (first) {
        rc_coder_begin(c, in, len);
    } else {
        c.low = sv[0]; c.range = sv[1]; c.code = sv[2]; c.pos = (int64_t)sv[3];
        if (c.pos < 0) c.pos = len;                  // not a position this kernel stored: read zeros
    }
    // parameters one symbol ahead, as in rc_decode_kernel: lane 0 the mean, lane 1 the scale
    auto fetch = [&](int p, int jj) -> float {
        if (p >= d.HW || lane >= 2) return 0.f;
        const int m = mt[2 + j0 + jj];
        if ((unsigned)m >= (unsigned)d.M) return 0.f;
        const int64_t sm = ((int64_t)b * d.HW + p) * d.sm_pix_stride + m;
        return lane == 0 ? means[sm + d.m_c_off] : scales[sm + d.s_c_off];
    };
    const float wk[1] = {1.f};
    float nxt = fetch(0, 0);
    for (int p = 0; p < d.HW; ++p) {
        const int row = centre[p];
        for (int jj = 0; jj < nj; ++jj) {
            const float raw = nxt;
            nxt = jj + 1 < nj ? fetch(p, jj + 1) : fetch(p + 1, 0);
            const int m = mt[2 + j0 + jj];
            if ((unsigned)m >= (unsigned)d.M) continue;      // a damaged channel list: nothing to address
            const int idx = rc_decode_symbol(raw, wk, 1, A, minmax, d.scale_bound, frow, crow, tbuf[wave], lane, in, len, c);
            if (lane == 0 && row >= 0 && row < rows_per_image)
                st_any(y_rows, ((int64_t)b * rows_per_image + row) * d.M + m, y_dtype, (float)(idx - minmax));
            __builtin_amdgcn_wave_barrier();          // the row buffers are rewritten by the next symbol
        }
    }
    if (lane == 0) { sv[0] = c.low; sv[1] = c.range; sv[2] = c.code; sv[3] = (uint64_t)c.pos; }
}

// The batch form of glue.hip's joint_step_kernel without its phase 1: for the P pixels of one wavefront group (centre / rows: their padded
// and raster rows) and the B images, in 16-byte chunks spread over the grid: the 5 x 5 crops of the padded maps -> crops[b * P + p][25][M],
// the hyper-decoder rows par[b][row] -> feat[b * P + p][0, c_par), view 2's extra rows ext[b][row] -> feat[..][e_off, +M).  A row outside
// its map reads as zeros.
struct JointGather {
    const unsigned char* y_rows; int es, M, Wp; int64_t rows_per_image;
    const int32_t* centre; const int32_t* rows; int B, P, HW;
    unsigned char* crops; const unsigned char* par; int c_par; const unsigned char* ext; int e_off; unsigned char* feat; int c_feat;
};
__global__ __launch_bounds__(256) void joint_gather_batch_kernel(const JointGather a) {
    const int rch = a.M * a.es / 16, pch = a.c_par * a.es / 16, fch = a.c_feat * a.es / 16, ech = a.ext ? rch : 0;
    const int per_row = 25 * rch + pch + ech;                          // chunks per (image, pixel)
    const int64_t total = (int64_t)a.B * a.P * per_row;
    for (int64_t i = blockIdx.x * 256ll + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        const int r = (int)(i / per_row), c = (int)(i - (int64_t)r * per_row);
        const int b = r / a.P, p = r - b * a.P;
        u32x4 v = u32x4{0u, 0u, 0u, 0u};
        if (c < 25 * rch) {
            const int t = c / rch, cc = c - t * rch;
            const int64_t src = (int64_t)a.centre[p] + (t / 5 - 2) * a.Wp + (t % 5 - 2);
            if (src >= 0 && src < a.rows_per_image) v = ((const u32x4*)(a.y_rows + ((int64_t)b * a.rows_per_image + src) * a.M * a.es))[cc];
            ((u32x4*)a.crops)[(int64_t)r * 25 * rch + c] = v;
        } else if (c < 25 * rch + pch) {
            const int cc = c - 25 * rch, row = a.rows[p];
            if ((unsigned)row < (unsigned)a.HW) v = ((const u32x4*)(a.par + ((int64_t)b * a.HW + row) * a.c_par * a.es))[cc];
            ((u32x4*)a.feat)[(int64_t)r * fch + cc] = v;
        } else {
            const int cc = c - 25 * rch - pch, row = a.rows[p];
            if ((unsigned)row < (unsigned)a.HW) v = ((const u32x4*)(a.ext + ((int64_t)b * a.HW + row) * a.M * a.es))[cc];
            ((u32x4*)a.feat)[(int64_t)r * fch + a.e_off * a.es / 16 + cc] = v;
        }
    }
}

int check_codec_gmm(const hesic_gmm_desc* d, const char* who) {
    HESIC_CHECK_ARG(d && d->B > 0 && d->HW > 0 && d->M > 0 && d->K >= 1 && d->K <= GMM_MAXK, "%s: bad geometry (K <= %d)", who, GMM_MAXK);
    HESIC_CHECK_ARG(d->dtype == HESIC_H16 || d->dtype == HESIC_F32, "%s: bad dtype", who);
    HESIC_CHECK_ARG((int64_t)d->B * d->M * d->HW < (1ll << 31) / 3, "%s: batch too large for 32-bit element indices", who);
    return 0;
}

}  // namespace

extern "C" int64_t hesic_rc_stream_cap(int64_t n_symbols) { return n_symbols < 0 ? 16 : 4 * n_symbols + 16; }

extern "C" int hesic_gmm_rc_ranges(const hesic_gmm_desc* d, const void* scales, const void* means, const float* weights, const void* y_hat,
                                   int y_dtype, const int32_t* meta, int32_t* triples, void* stream) {
    if (int e = check_codec_gmm(d, "gmm_rc_ranges")) return e;
    HESIC_CHECK_ARG(scales && means && y_hat && meta && triples, "gmm_rc_ranges: null pointer");
    HESIC_CHECK_ARG(weights || d->K == 1, "gmm_rc_ranges: weights required for K > 1");
    HESIC_CHECK_ARG(y_dtype == HESIC_H16 || y_dtype == HESIC_F32, "gmm_rc_ranges: bad y_hat dtype");
    const dim3 grid(grid_for((int64_t)d->B * d->M * d->HW, 4, 256 * 32));
    if (d->dtype == HESIC_H16)
        hipLaunchKernelGGL(rc_ranges_kernel<h16_t>, grid, dim3(256), 0, (hipStream_t)stream, *d, (const h16_t*)scales, (const h16_t*)means, weights,
                           y_hat, y_dtype, meta, triples);
    else
        hipLaunchKernelGGL(rc_ranges_kernel<float>, grid, dim3(256), 0, (hipStream_t)stream, *d, (const float*)scales, (const float*)means, weights,
                           y_hat, y_dtype, meta, triples);
    HESIC_LAUNCH_RETURN("gmm_rc_ranges");
}

extern "C" int hesic_rc_encode_streams(const int32_t* triples, const int32_t* meta, int B, int M, int HW, int channels_per_stream, uint8_t* slots,
                                       int64_t cap, int32_t* counts, int32_t* status, void* stream) {
    HESIC_CHECK_ARG(triples && meta && slots && counts && status, "rc_encode_streams: null pointer");
    HESIC_CHECK_ARG(B > 0 && M > 0 && HW > 0 && channels_per_stream >= 1 && channels_per_stream <= M, "rc_encode_streams: bad geometry");
    HESIC_CHECK_ARG((int64_t)B * M * HW < (1ll << 31) / 3, "rc_encode_streams: batch too large for 32-bit element indices");
    HESIC_CHECK_ARG(cap >= hesic_rc_stream_cap((int64_t)channels_per_stream * HW), "rc_encode_streams: slots of %lld bytes, a stream needs %lld",
                    (long long)cap, (long long)hesic_rc_stream_cap((int64_t)channels_per_stream * HW));
    const int S = (M + channels_per_stream - 1) / channels_per_stream;
    hipLaunchKernelGGL(rc_encode_kernel, dim3((B * S + 63) / 64), dim3(64), 0, (hipStream_t)stream, triples, meta, B, M, HW, channels_per_stream, S,
                       slots, cap, counts, status);
    HESIC_LAUNCH_RETURN("rc_encode_streams");
}

extern "C" int hesic_rc_compact_streams(const uint8_t* slots, int64_t cap, const int32_t* counts, const int64_t* offsets, int64_t n_streams,
                                        uint8_t* out, int64_t out_bytes, void* stream) {
    HESIC_CHECK_ARG(slots && counts && offsets && cap > 0 && n_streams > 0 && n_streams < (1ll << 31) && out_bytes >= 0 && (out || out_bytes == 0),
                    "rc_compact_streams: bad arguments");
    if (out_bytes == 0) return 0;
    hipLaunchKernelGGL(rc_compact_kernel, dim3((unsigned)n_streams), dim3(256), 0, (hipStream_t)stream, slots, cap, counts, offsets, out, out_bytes);
    HESIC_LAUNCH_RETURN("rc_compact_streams");
}

extern "C" int hesic_gmm_rc_decode(const hesic_gmm_desc* d, const void* scales, const void* means, const float* weights, const int32_t* meta,
                                   int channels_per_stream, const uint8_t* bytes, int64_t n_bytes, const int64_t* offsets, const int32_t* counts,
                                   void* y_hat, int y_dtype, void* stream) {
    if (int e = check_codec_gmm(d, "gmm_rc_decode")) return e;
    HESIC_CHECK_ARG(scales && means && meta && offsets && counts && y_hat && n_bytes >= 0 && (bytes || n_bytes == 0), "gmm_rc_decode: bad arguments");
    HESIC_CHECK_ARG(weights || d->K == 1, "gmm_rc_decode: weights required for K > 1");
    HESIC_CHECK_ARG(y_dtype == HESIC_H16 || y_dtype == HESIC_F32, "gmm_rc_decode: bad y_hat dtype");
    HESIC_CHECK_ARG(channels_per_stream >= 1 && channels_per_stream <= d->M, "gmm_rc_decode: bad channels_per_stream");
    const int S = (d->M + channels_per_stream - 1) / channels_per_stream;
    const int n = d->B * S;
    if (d->dtype == HESIC_H16)
        hipLaunchKernelGGL(rc_decode_kernel<h16_t>, dim3((n + 3) / 4), dim3(256), 0, (hipStream_t)stream, *d, (const h16_t*)scales, (const h16_t*)means,
                           weights, meta, channels_per_stream, S, bytes, n_bytes, offsets, counts, y_hat, y_dtype);
    else
        hipLaunchKernelGGL(rc_decode_kernel<float>, dim3((n + 3) / 4), dim3(256), 0, (hipStream_t)stream, *d, (const float*)scales, (const float*)means,
                           weights, meta, channels_per_stream, S, bytes, n_bytes, offsets, counts, y_hat, y_dtype);
    HESIC_LAUNCH_RETURN("gmm_rc_decode");
}

extern "C" int hesic_rc_encode_streams_ordered(const int32_t* triples, const int32_t* meta, int B, int M, int HW, int channels_per_stream,
                                               const int32_t* order, uint8_t* slots, int64_t cap, int32_t* counts, int32_t* status, void* stream) {
    HESIC_CHECK_ARG(triples && meta && order && slots && counts && status, "rc_encode_streams_ordered: null pointer");
    HESIC_CHECK_ARG(B > 0 && M > 0 && HW > 0 && channels_per_stream >= 1 && channels_per_stream <= M, "rc_encode_streams_ordered: bad geometry");
    HESIC_CHECK_ARG((int64_t)B * M * HW < (1ll << 31) / 3, "rc_encode_streams_ordered: batch too large for 32-bit element indices");
    HESIC_CHECK_ARG(cap >= hesic_rc_stream_cap((int64_t)channels_per_stream * HW), "rc_encode_streams_ordered: slots of %lld bytes, a stream needs %lld",
                    (long long)cap, (long long)hesic_rc_stream_cap((int64_t)channels_per_stream * HW));
    const int S = (M + channels_per_stream - 1) / channels_per_stream;
    hipLaunchKernelGGL(rc_encode_ordered_kernel, dim3((B * S + 63) / 64), dim3(64), 0, (hipStream_t)stream, triples, meta, B, M, HW,
                       channels_per_stream, S, order, slots, cap, counts, status);
    HESIC_LAUNCH_RETURN("rc_encode_streams_ordered");
}

extern "C" int hesic_joint_gather_batch(const void* y_rows, int dtype, int M, int Wp, int64_t rows_per_image, const int32_t* centre,
                                        const int32_t* rows, int group_offset, int P, int HW, int B, void* crops, const void* par, int c_par,
                                        const void* ext, int e_off, void* feat, int c_feat, void* stream) {
    HESIC_CHECK_ARG(y_rows && centre && rows && crops && par && feat, "joint_gather_batch: null pointer");
    HESIC_CHECK_ARG(dtype == HESIC_H16 || dtype == HESIC_F32, "joint_gather_batch: bad dtype");
    HESIC_CHECK_ARG(B > 0 && M > 0 && Wp > 4 && rows_per_image > 0 && HW > 0 && P > 0 && group_offset >= 0 && (int64_t)group_offset + P <= HW,
                    "joint_gather_batch: bad geometry (the group [offset, offset + P) must lie inside the HW pixels, P > 0)");
    const int es = dtype == HESIC_H16 ? 2 : 4;
    HESIC_CHECK_ARG(c_par > 0 && c_par <= c_feat && e_off >= 0 && (M * es) % 16 == 0 && (c_par * es) % 16 == 0 && (c_feat * es) % 16 == 0 &&
                        (e_off * es) % 16 == 0 && (!ext || e_off + M <= c_feat),
                    "joint_gather_batch: rows must be whole 16-byte chunks and the feature slices must fit");
    HESIC_CHECK_ARG((int64_t)B * P * (25 * M + c_feat) < (1ll << 31) && (int64_t)B * rows_per_image * M < (1ll << 40),
                    "joint_gather_batch: batch too large for 32-bit row indices");
    JointGather a;
    a.y_rows = (const unsigned char*)y_rows; a.es = es; a.M = M; a.Wp = Wp; a.rows_per_image = rows_per_image;
    a.centre = centre + group_offset; a.rows = rows + group_offset; a.B = B; a.P = P; a.HW = HW;
    a.crops = (unsigned char*)crops; a.par = (const unsigned char*)par; a.c_par = c_par; a.ext = (const unsigned char*)ext; a.e_off = e_off;
    a.feat = (unsigned char*)feat; a.c_feat = c_feat;
    const int64_t chunks = (int64_t)B * P * ((25 * M + c_par + (ext ? M : 0)) * es / 16);
    hipLaunchKernelGGL(joint_gather_batch_kernel, dim3(grid_for(chunks, 256, 256 * 4)), dim3(256), 0, (hipStream_t)stream, a);
    HESIC_LAUNCH_RETURN("joint_gather_batch");
}

extern "C" int hesic_gmm_rc_decode_step(const hesic_gmm_desc* d, const float* scales, const float* means, const int32_t* meta, int channels_per_stream,
                                        const uint8_t* bytes, int64_t n_bytes, const int64_t* offsets, const int32_t* counts, uint64_t* state,
                                        int first, const int32_t* centre, int group_offset, int n_pixels, void* y_rows, int y_dtype,
                                        int64_t rows_per_image, void* stream) {
    if (int e = check_codec_gmm(d, "gmm_rc_decode_step")) return e;
    HESIC_CHECK_ARG(d->K == 1 && d->dtype == HESIC_F32, "gmm_rc_decode_step: K = 1 and fp32 (scale, mean) rows only");
    HESIC_CHECK_ARG(scales && means && meta && offsets && counts && state && centre && y_rows && n_bytes >= 0 && (bytes || n_bytes == 0),
                    "gmm_rc_decode_step: bad arguments");
    HESIC_CHECK_ARG(y_dtype == HESIC_H16 || y_dtype == HESIC_F32, "gmm_rc_decode_step: bad y_rows dtype");
    HESIC_CHECK_ARG(channels_per_stream >= 1 && channels_per_stream <= d->M, "gmm_rc_decode_step: bad channels_per_stream");
    HESIC_CHECK_ARG(rows_per_image > 0 && n_pixels > 0 && group_offset >= 0 && (int64_t)group_offset + d->HW <= n_pixels,
                    "gmm_rc_decode_step: the group [offset, offset + P) must lie inside the n_pixels of the map");
    const int S = (d->M + channels_per_stream - 1) / channels_per_stream;
    const int n = d->B * S;
    hipLaunchKernelGGL(rc_decode_step_kernel, dim3((n + 3) / 4), dim3(256), 0, (hipStream_t)stream, *d, scales, means, meta, channels_per_stream, S,
                       bytes, n_bytes, offsets, counts, state, first, centre + group_offset, y_rows, y_dtype, rows_per_image);
    HESIC_LAUNCH_RETURN("gmm_rc_decode_step");
}

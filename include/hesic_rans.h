/*
 * hesic_rans.h -- C ABI of the device rANS coder for batches of independent streams in libhesic_hip.so / libhesic_hip_f16.so
 * (hesic_amd/csrc/rans.hip): the z strings of HSIC / HSICJoint.compress_batch / decompress_batch(z_coder="device").  Every stream
 * is, byte for byte, what the host coder writes (hesic_rans_encoder_push / _flush, hesic_rans_decoder_decode of
 * hesic_amd/csrc/host/hesic_host.cpp): a 64-bit state renormalised in 32-bit words, 16-bit frequencies, symbols outside a row's
 * support as the escape bin followed by 4-bit raw nibbles (one count nibble, then the data nibbles of `raw`, lowest first), and the two
 * state words of the flush in front.
 *
 * Conventions as in hesic_hip.h: DEVICE pointers, element counts, `stream` a hipStream_t, asynchronous; return 0 or a hipError_t
 * (> 0) or HESIC_EINVAL (-1), with hesic_last_error() describing the failure.  No atomics; two runs give identical bytes.
 *
 * tables   cdfs (ncdf, cdf_stride) int32 quantised CDFs, sizes (ncdf) int32 entries used per row (2 <= sizes[r] <= cdf_stride, the last
 *          bin is the escape bin), offsets (ncdf) int32 the symbol value of a row's entry 0 -- EntropyModel's _quantized_cdf,
 *          _cdf_length, _offset.  cdf_stride <= HESIC_RANS_MAX_ROW.
 * streams  n_streams streams of n symbols each, n = C * P.  Symbol i = (c, p), c = i / P, p = i % P, of stream b lies at element
 *          b * sb + c * sc + p * sp of `symbols` (and of z_hat / symbols_out): (sb, sc, sp) = (n, P, 1) is a contiguous (B, C, P)
 *          array, (n, 1, C) a channels-last one, read and written in place.
 * indexes  the table row of symbol i of stream b: NULL means row c = i / P (the bottleneck's channel-major runs); otherwise int32,
 *          entry b * index_stride + i (index_stride 0: one array of n entries shared by the batch, n: one per stream).
 * dequant  medians != NULL: z_hat element = (float)symbol + medians[row], rounded once to z_dtype (HESIC_F32 or HESIC_H16) -- what
 *          EntropyModel._dequantize(symbols, medians).to(dtype) yields -- with the symbols' strides.  medians NULL: no such output.
 * status   (n_streams) int32, written (not OR-ed) by the kernel that walks the stream: 0 or a sum of the bits below.  A stream with
 *          a non-zero status has count 0 (encoder) / unspecified symbols (decoder); nothing is read or written outside the arguments.
 */
#ifndef HESIC_RANS_H
#define HESIC_RANS_H

#include <stddef.h>
#include <stdint.h>

#include "hesic_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define HESIC_RANS_MAX_ROW 512      /* a row lives in the registers of one wave: at most 8 entries per lane */
enum {
    HESIC_RANS_OVERFLOW = 1,        /* encoder: the stream did not fit its slot */
    HESIC_RANS_BAD_TABLE = 2,       /* a row index outside [0, ncdf), a row size outside [2, cdf_stride] or a zero frequency */
    HESIC_RANS_BAD_ESCAPE = 4,      /* decoder: an escape claims more than 8 data nibbles (no int32 symbol needs them) */
    HESIC_RANS_BAD_STREAM = 8       /* decoder: a stream shorter than 8 bytes, not whole 32-bit words, misaligned or outside the payload */
};

/* bytes of one stream's slot: 8 per symbol + 16 (a symbol costs at most 16 bits modelled, or 52 bits as an escape; 8 bytes flush) */
int64_t hesic_rans_slot_bytes(int64_t n);
/* bytes of the encoder's workspace (the itemised symbols: 9 bytes each) */
int64_t hesic_rans_encode_ws_bytes(int64_t n_streams, int64_t n);
/* Two launches.  (1) one lane per symbol of the batch: v = symbol - offsets[row], the escape decision and raw exactly as
 * hesic_rans_encoder_push (odd raw below the support, even at or above), the modelled (start, freq) and the nibble count into ws,
 * and z_hat if medians != NULL.  (2) one wave per stream: the items walked backwards, every emitted 32-bit word written downwards
 * from the end of the stream's slot, then the two state words: stream b is the LAST counts[b] bytes of slots[b * slot_bytes .. +
 * slot_bytes).  slot_bytes >= hesic_rans_slot_bytes(n) and a multiple of 4; a stream that still would not fit gets
 * HESIC_RANS_OVERFLOW.  ws: ws_bytes >= hesic_rans_encode_ws_bytes(n_streams, n), 8-byte aligned. */
int hesic_rans_encode(const int32_t* symbols, int64_t sb, int64_t sc, int64_t sp, int n_streams, int64_t n, int64_t P,
                      const int32_t* indexes, int64_t index_stride, const int32_t* cdfs, int ncdf, int cdf_stride, const int32_t* sizes,
                      const int32_t* offsets, void* ws, int64_t ws_bytes, uint8_t* slots, int64_t slot_bytes, int32_t* counts,
                      int32_t* status, const float* medians, void* z_hat, int z_dtype, void* stream);
/* out[out_offsets[t] .. + counts[t]) = the stream at the END of slot t; out_offsets (n_streams) int64 = exclusive scan of counts;
 * copies are clipped to out_bytes */
int hesic_rans_compact(const uint8_t* slots, int64_t slot_bytes, const int32_t* counts, const int64_t* out_offsets, int n_streams,
                       uint8_t* out, int64_t out_bytes, void* stream);
/* One wave per stream: stream b is data[data_offsets[b] .. + counts[b]) inside data[0 .. n_bytes) (data 4-byte aligned); a word
 * past a stream's end reads as 0, as the host decoder's.  The symbol search (largest s with cdf[s] <= slot) is a ballot + popcount over
 * the row held in registers, reloaded only when the row index changes.  symbols_out (may be NULL) and z_hat (with medians; may be
 * NULL) are written with the strides above; at least one of them is required. */
int hesic_rans_decode(const uint8_t* data, int64_t n_bytes, const int64_t* data_offsets, const int32_t* counts, int n_streams, int64_t n,
                      int64_t P, const int32_t* indexes, int64_t index_stride, const int32_t* cdfs, int ncdf, int cdf_stride,
                      const int32_t* sizes, const int32_t* offsets, int32_t* symbols_out, int64_t sb, int64_t sc, int64_t sp,
                      const float* medians, void* z_hat, int z_dtype, int32_t* status, void* stream);

#ifdef __cplusplus
}
#endif
#endif

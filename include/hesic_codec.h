/*
 * hesic_codec.h -- C ABI of the device-resident range coder for the HESIC latents in libhesic_hip.so / libhesic_hip_f16.so
 * (hesic_amd/csrc/codec.hip): batched HSIC.compress_batch / decompress_batch.  No table and no symbol leaves the device; only
 * the coded bytes do.
 *
 * Conventions as in hesic_hip.h: DEVICE pointers, element counts, `stream` a hipStream_t, asynchronous; return 0 or a hipError_t
 * (> 0) or HESIC_EINVAL (-1), with hesic_last_error() describing the failure.  scales / means / weights and the descriptor are
 * those of hesic_gmm_cdf (d->dtype: storage of scales and means); all launches serve the d->B images of a batch at once.
 *
 * meta    (B, M + 2) int32, per image of ONE view: [n_coded, minmax, channel_0 .. channel_{n_coded-1}, unused ...] -- the coded
 *         (flagged) channels in ascending order and the alphabet 2 * minmax + 1 <= HESIC_CODEC_MAX_ALPHABET of that image.
 * y_hat   (B, M, H, W) channels-last (pixel stride M) rounded latents, y_dtype HESIC_F32 or HESIC_H16.
 * stream  (b, s), s < S = ceil(M / channels_per_stream): the symbols y_hat + minmax of the coded channels
 *         [s * cps, min((s + 1) * cps, n_coded)) of image b, channel-major, then rows, then columns; streams beyond the image's
 *         coded channels are empty.  Flat stream index t = b * S + s.
 * A stream is coded by the state machine of the host range coder (hesic_rc_encoder_encode: 64-bit low / range, 2^56 / 2^48,
 * the same renormalisation) and ends with the top two bytes of low rounded up to a multiple of 2^48, trailing zero bytes
 * dropped; a decoder reads zeros past the end of a stream.
 */
#ifndef HESIC_CODEC_H
#define HESIC_CODEC_H

#include <stddef.h>
#include <stdint.h>

#include "hesic_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define HESIC_CODEC_MAX_ALPHABET 1024   /* one table row in LDS per wave, as the wave table kernel of hesic_gmm_cdf */
enum { HESIC_CODEC_OVERFLOW = 1, HESIC_CODEC_BAD_SYMBOL = 2 };   /* bits of the encoder's status word */

/* bytes of one stream's slot: 4 per symbol + 16 */
int64_t hesic_rc_stream_cap(int64_t n_symbols);
/* triples (B, M, HW, 3) int32: for listed channel j < n_coded and pixel hw of image b, {c[s], c[s+1] - c[s], c[A]} of the coded symbol
 * s = y_hat + minmax in the table row hesic_gmm_cdf forms for that element (bit for bit); a symbol outside the alphabet yields
 * frequency 0.  Rows j >= n_coded are not written. */
int hesic_gmm_rc_ranges(const hesic_gmm_desc* d, const void* scales, const void* means, const float* weights, const void* y_hat,
                        int y_dtype, const int32_t* meta, int32_t* triples, void* stream);
/* One lane per stream: slots (B * S, cap) uint8, counts (B * S) int32 bytes written per stream (0 for empty streams), status (1) int32
 * zeroed by the caller and OR-ed with HESIC_CODEC_OVERFLOW (a stream did not fit its slot; it stops, nothing is written past the slot)
 * or HESIC_CODEC_BAD_SYMBOL (a triple with zero frequency).  cap >= hesic_rc_stream_cap(channels_per_stream * HW). */
int hesic_rc_encode_streams(const int32_t* triples, const int32_t* meta, int B, int M, int HW, int channels_per_stream, uint8_t* slots,
                            int64_t cap, int32_t* counts, int32_t* status, void* stream);
/* out[offsets[t] .. + counts[t]) = slot t; offsets (n_streams) int64 = exclusive scan of counts; copies are clipped to out_bytes */
int hesic_rc_compact_streams(const uint8_t* slots, int64_t cap, const int32_t* counts, const int64_t* offsets, int64_t n_streams,
                             uint8_t* out, int64_t out_bytes, void* stream);
/* One wave per stream: decodes stream t from bytes[offsets[t] .. + counts[t]) (clipped to n_bytes; reads past a stream's end yield 0)
 * and writes symbol - minmax into the coded channels of y_hat; the caller zero-fills y_hat first (unflagged channels).  The number
 * of symbols per stream follows from meta alone; a damaged payload yields wrong latents, never a longer loop or an address
 * outside the arguments. */
int hesic_gmm_rc_decode(const hesic_gmm_desc* d, const void* scales, const void* means, const float* weights, const int32_t* meta,
                        int channels_per_stream, const uint8_t* bytes, int64_t n_bytes, const int64_t* offsets, const int32_t* counts,
                        void* y_hat, int y_dtype, void* stream);

#ifdef __cplusplus
}
#endif
#endif

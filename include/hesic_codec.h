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
 *
 * HESIC+ streams (HSICJoint.compress_batch / decompress_batch; the "ordered" encoder, the batched group gather and the step decoder
 * below).  Same cut into streams of channels_per_stream coded channels, same coder, same termination; what differs is the ORDER of
 * the symbols, because the table row of a HESIC+ latent depends on latents decoded before it (5 x 5 mask-'A' context).  The pixels
 * of an (H/16, W/16) latent map are walked group by group of HSICJoint._wavefronts: t = w + 3 h ascending, raster index h * W/16 + w
 * ascending inside a group (all pixels of a group depend on earlier groups only).  Stream (b, s) carries, for each pixel in that
 * order, the symbols y_hat + minmax of the stream's channels in ascending order (pixel-major: with channels_per_stream = M this is
 * the symbol sequence of the per-pair HSICJoint.compress(order="wavefront")).  The table row of a symbol is the row hesic_gmm_cdf
 * forms for K = 1, weights = NULL from the fp32 (scale | mean) output rows of the entropy-parameter net.  Alphabets are limited to
 * HESIC_CODEC_MAX_ALPHABET as above.
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


/* ---- HESIC+ (wavefront order) */
/* hesic_rc_encode_streams with a pixel permutation: order (HW) int32, the raster index of the i-th pixel in coding order; symbol i
 * of stream (b, s) is the triple of channel j0 + i % nj of pixel order[i / nj] (j0 = s * cps, nj the stream's channel count).  The
 * triples are hesic_gmm_rc_ranges' over the whole-map (scale, mean).  Same slots, counts, status bits and cap as above; an order
 * entry outside [0, HW) sets HESIC_CODEC_BAD_SYMBOL. */
int hesic_rc_encode_streams_ordered(const int32_t* triples, const int32_t* meta, int B, int M, int HW, int channels_per_stream,
                                    const int32_t* order, uint8_t* slots, int64_t cap, int32_t* counts, int32_t* status, void* stream);
/* One wavefront group of a batch: pixels [group_offset, group_offset + P) of the coding order, B images.  y_rows: the B padded
 * latent maps, (B, rows_per_image, M) rows of `dtype`, rows_per_image = (H/16 + 4) * Wp, Wp = W/16 + 4; centre / rows (HW) int32:
 * per pixel in coding order its row in the padded map and its raster row.  Writes, image-major (row b * P + p):
 *   crops (B * P, 25, M)   the 5 x 5 neighbourhood of the pixel (rows outside the map read as zeros),
 *   feat  (B * P, c_feat)  [0, c_par) <- par (B, HW, c_par) row, and with ext != NULL [e_off, e_off + M) <- ext (B, HW, M) row.
 * M, c_par, c_feat and e_off must be whole 16-byte chunks of `dtype`. */
int hesic_joint_gather_batch(const void* y_rows, int dtype, int M, int Wp, int64_t rows_per_image, const int32_t* centre,
                             const int32_t* rows, int group_offset, int P, int HW, int B, void* crops, const void* par, int c_par,
                             const void* ext, int e_off, void* feat, int c_feat, void* stream);
/* hesic_gmm_rc_decode cut at group boundaries.  d: B images, HW = P pixels of THIS group, K = 1, dtype HESIC_F32; scales / means
 * address row b * P + p of the entropy-parameter net's output through d (pixel stride, channel offsets).  One wave per stream:
 * state (B * S, 4) uint64 {low, range, code, byte position} is loaded (first == 0) or begun from the stream's first 8 bytes
 * (first != 0), the P * nj symbols of the group are decoded pixel-major, symbol - minmax is written into row centre[group_offset + p]
 * of image b in y_rows ((B, rows_per_image, M) of y_dtype; rows outside [0, rows_per_image) are skipped), and the state is stored.
 * bytes / n_bytes / offsets / counts as hesic_gmm_rc_decode.  Loop counts follow from meta and P alone; a damaged payload yields
 * wrong latents, never a longer loop or an address outside the arguments. */
int hesic_gmm_rc_decode_step(const hesic_gmm_desc* d, const float* scales, const float* means, const int32_t* meta, int channels_per_stream,
                             const uint8_t* bytes, int64_t n_bytes, const int64_t* offsets, const int32_t* counts, uint64_t* state,
                             int first, const int32_t* centre, int group_offset, int n_pixels, void* y_rows, int y_dtype,
                             int64_t rows_per_image, void* stream);

#ifdef __cplusplus
}
#endif
#endif

/* hesic_homonet_items.h -- the item form of hesic_homonet_prepare (hesic_homography_prep.h, which includes this header): HomographyNet's
 * inputs of a batch straight from STORED uint8 images, every item at its own address with its own size, in one launch.  It feeds the net
 * from a device-resident folder (pair_cache.DevicePairCache.homonet_batch, ``python -m hesic_amd.homography_train --cache device|stream``):
 * the net only ever sees the S x S frame, so pairs of different sizes share a batch.  Exported by both libraries (libhesic_hip.so,
 * libhesic_hip_f16.so); an addition to HESIC_ABI_VERSION 2.  Conventions as in hesic_homography_prep.h.  No atomics, no shared memory.   */
#ifndef HESIC_HOMONET_ITEMS_H
#define HESIC_HOMONET_ITEMS_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

typedef struct {
    const uint8_t* left;    /* stored left view: (rows, pitch_px, 3) uint8 RGB, dense */
    const uint8_t* right;   /* stored right view, same geometry */
    int32_t pitch_px, rows; /* stored image */
    int32_t x0, y0;         /* crop origin inside the stored image */
    int32_t cw, ch;         /* crop size: the frame that is resized to S x S */
    int32_t wx, wy;         /* window origin in the S x S frame */
} hesic_homonet_item;       /* 48 bytes */

/* items: B descriptors in DEVICE memory (8-byte aligned).  The outputs are exactly those of hesic_homonet_prepare -- grey1, grey2
 * (B, 1, S, S), patch1, patch2 (B, 1, P, P), corners (B, 4, 2): fp32, dense, every element written -- and so is the arithmetic, applied to
 * the crop view[y0 : y0 + ch, x0 : x0 + cw] of each view as if that crop were the whole image: per item scale_y = (float)ch / (float)S and
 * scale_x = (float)cw / (float)S by IEEE division, the axis rule of hesic_homography_prep.h with n = ch resp. cw -- so the taps are clamped
 * to the CROP's last row and column, not the stored image's --, the same resampling, rounding, normalisation and grey.  Item b's outputs
 * are bit for bit those of hesic_homonet_prepare on a HESIC_PREP_U8 (1, 3, ch, cw) view of that crop with xy = (wx, wy), whatever the
 * other items of the batch are.
 *
 * Memory contract.  Apart from the B descriptors, the kernel reads only bytes of the two crop rectangles of an item -- row y0 + i, bytes
 * [3 (x0), 3 (x0 + cw)) of that row, for 0 <= i < ch --, never the rest of the stored image and nothing before or behind it; it writes the
 * five outputs and nothing else.  A crop may therefore end at the last byte of an allocation.  Source addresses are formed in 64 bits.
 *
 * The CALLER guarantees per item, since the entry cannot read device memory: left, right not null; 0 <= x0, x0 + cw <= pitch_px; 0 <= y0,
 * y0 + ch <= rows; cw, ch >= 1; 0 <= wx, wy <= S - P (functional.check_homonet_items does this on the host).  A window outside that range
 * cannot write out of bounds, as in hesic_homonet_prepare; a crop outside its image reads out of bounds.  The entry checks the pointers
 * and their alignment (items 8 bytes, outputs 4), 1 <= B <= 65535, 1 <= P <= S <= 16384, std != 0, mean and std not NaN.
 *
 * One launch of ceil(S * S / 256) x B x 2 blocks of 256 threads, one grey element per thread; blockIdx.y is the item, whose descriptor the
 * block reads once.  The three channels of a tap are adjacent bytes and the two taps of a row adjacent pixels: a thread fetches each of its
 * two rows as one 4-byte and one 2-byte load at byte alignment (the pair of columns is shifted left by one at the crop's last column, so
 * the six bytes stay inside the crop; a crop one pixel wide is read as its three bytes), 4 loads instead of the strided form's 12.
 *
 * Measured (profiles/homography_cache_bench.json; one box, warm, median of seven, variants alternating, graph replays): B = 8 whole
 * 512 x 512 images -> 256 x 256, P = 128: 13.6 us, against 13.3 us for hesic_homonet_prepare on the same images stacked and 4.15 us for a
 * device copy of the 17.8 MB moved (3.28 x the copy; the strided form 3.21 x).  The item form is NOT faster: both execute about 280 vector
 * instructions per thread (nine resp. eleven IEEE divisions are about a third of them) and that is the bound, not the loads -- what the fewer
 * loads and the cheaper addresses save, the two divisions for the per-item scales and the unpacking of the taps spend again.              */
int hesic_homonet_prepare_items(const hesic_homonet_item* items, int B, int S, int P, float mean, float std, float* grey1, float* grey2,
                                float* patch1, float* patch2, float* corners, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* HESIC_HOMONET_ITEMS_H */

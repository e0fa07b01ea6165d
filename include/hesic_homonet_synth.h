/* hesic_homonet_synth.h -- synthetic-warp pairs for HomographyNet's supervised training, straight from STORED uint8 images: per item the
 * grey frame of ONE view (as hesic_homonet_prepare_items makes it), a known perspective warp of that frame, the two windows and the corner
 * offsets that are the label.  It finishes what the reference's ``udh/udh/dataset.py`` (``SyntheticDataset``) leaves commented out:
 * ``h = get_perspective_transform(corners, corners + delta); img_b = warp_perspective(img_a, inverse(h), (S, S))``.  It feeds
 * pair_cache.DevicePairCache.homonet_synth_batch, ``python -m hesic_amd.homography_train --supervision synthetic`` and ``python -m
 * hesic_amd.homography_eval``.  Exported by both libraries (libhesic_hip.so, libhesic_hip_f16.so); an addition to HESIC_ABI_VERSION 2;
 * hesic_hip.h does not include it.  Conventions as in hesic_homonet_items.h.  No atomics, no shared memory, no host synchronisation.      */
#ifndef HESIC_HOMONET_SYNTH_H
#define HESIC_HOMONET_SYNTH_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

typedef struct {
    const uint8_t* view;      /* stored view: (rows, pitch_px, 3) uint8 RGB, dense */
    int32_t pitch_px, rows;   /* stored image */
    int32_t x0, y0, cw, ch;   /* crop that is resized to S x S */
    int32_t wx, wy;           /* window origin in the S x S frame */
    int32_t delta[8];         /* corner offsets (x, y) x 4, in the order of `corners` */
} hesic_homonet_synth_item;   /* 72 bytes */

/* items: B descriptors in DEVICE memory (8-byte aligned).  Outputs, dense, every element written:
 *
 *   grey_a  (B,1,S,S) fp32   the resized, quantised, normalised grey frame of the crop: the bits of hesic_homonet_prepare_items' grey1 for
 *                            the same stored view, crop and window (the same device functions, csrc/homonet_prep_dev.h)
 *   patch_a (B,1,P,P) fp32   grey_a[wy : wy + P, wx : wx + P]
 *   corners (B,4,2)   fp32   [[wx, wy], [wx+P, wy], [wx+P, wy+P], [wx, wy+P]], as in hesic_homography_prep.h
 *   delta   (B,4,2)   fp32   the descriptor's integers as floats: the label
 *   h       (B,9)     fp64   DLT(corners -> corners + delta), h[8] = 1, by csrc/dlt.h's dlt4; the corners are ABSOLUTE frame coordinates
 *   grey_b  (B,1,S,S) fp32   grey_b(p) = bilinear(grey_a, h p), zeros outside the frame: warp_perspective(grey_a, inverse(h), (S, S))
 *                            without the inversion pair.  align_corners has the meaning of hesic_warp_desc's.
 *   patch_b (B,1,P,P) fp32   grey_b[wy : wy + P, wx : wx + P]
 *
 * so homography.photometric_loss(delta, grey_a, patch_b, corners) -- which maps the window's own coordinates by DLT(corners - corners[0] ->
 * corners + delta), the same map behind a translation -- is zero up to rounding at the true delta.
 *
 * The arithmetic of grey_b, from the STORED h (the nine fp64 words above) on; every operation is an IEEE fp64 operation rounded on its own
 * (no contraction), divisions are IEEE divisions, x and y are the destination pixel's integer coordinates:
 *
 *   X = (h[0] * x + h[1] * y) + h[2];   Y = (h[3] * x + h[4] * y) + h[5];   Z = (h[6] * x + h[7] * y) + h[8]
 *   u = X / Z;   v = Y / Z
 *   sx = u, sy = v                          under align_corners = 1
 *   sx = u * k - 0.5, sy = v * k - 0.5      under align_corners = 0, with k = (double)S / (double)(S - 1)
 *   fx = floor(sx), fy = floor(sy);   wx1 = sx - fx, wx0 = 1.0 - wx1;   wy1 = sy - fy, wy0 = 1.0 - wy1
 *   acc = +0.0, then in THIS order, each term only where its tap (row, column) lies inside [0, S - 1]^2:
 *     acc = acc + grey_a[fy    ][fx    ] * (wx0 * wy0)
 *     acc = acc + grey_a[fy    ][fx + 1] * (wx1 * wy0)
 *     acc = acc + grey_a[fy + 1][fx    ] * (wx0 * wy1)
 *     acc = acc + grey_a[fy + 1][fx + 1] * (wx1 * wy1)
 *   grey_b = (float)acc                     the one rounding to fp32
 *
 * The taps are the fp32 values of grey_a, widened exactly.  A coordinate that is not finite (Z == 0) has no tap inside and gives 0.
 *
 * Form.  THREE launches on `stream`, in order: (1) one thread per item writes corners, delta and h (the DLT's 8 x 9 system lives in
 * scratch memory; inside launch (2) it would give every wave of that kernel the scratch and the registers of its one DLT thread);
 * (2) ceil(S * S / 256) x B blocks of 256 threads, one element of grey_a per thread -- the thread map of hesic_homonet_prepare_items with one
 * view; (3) the same grid, one element of grey_b per thread, reading h and the four taps back from grey_a.  The alternative, ONE launch
 * that recomputes every tap from the stored bytes, was not built: the item kernel is bound by its vector instruction count (about 280 per
 * thread, hesic_homonet_items.h), a recomputed tap costs that again, so grey_b would cost four times the first view on top of its own fp64
 * coordinates, where the read-back is four loads of a frame that launch (2) has just left in L2 (B = 16, S = 256: 4 MiB).  The bits are
 * the same either way, the device functions being the same; the price is two launch boundaries.
 *
 * Measured (profiles/homonet_synth_bench.json; one box, warm, median of seven, variants alternating, graph replays): B = 16 whole
 * 512 x 512 images -> 256 x 256, P = 128: 31.7 us, against 19.1 us for hesic_homonet_prepare_items on the same pairs (both views) and
 * 4.08 us for a device copy of the 27.3 MB moved (7.8 x the copy, 1.66 x the item entry).
 *
 * The bits of an item's outputs depend on its descriptor and its crop's bytes alone: not on the batch, its position in it, or the run.
 *
 * Memory contract.  That of hesic_homonet_items.h: apart from the B descriptors, and from h and grey_a, its own outputs that launch (3)
 * reads back, the entry reads only bytes of an item's crop rectangle -- row y0 + i, bytes [3 (x0), 3 (x0 + cw)) of that row, 0 <= i < ch --;
 * it writes the seven outputs and nothing else.  A crop may end at the last byte of an allocation.  Addresses are formed in 64 bits.
 *
 * The CALLER guarantees per item: view not null; 0 <= x0, x0 + cw <= pitch_px; 0 <= y0, y0 + ch <= rows; cw, ch >= 1; 0 <= wx, wy <= S - P;
 * the quadrilateral corners + delta strictly convex (functional.check_homonet_synth_items does this on the host, homography.draw_deltas
 * draws such deltas).  For a configuration dlt4 reports singular, the item's h, grey_b and patch_b are written as NaN; nothing is read or
 * written out of bounds.  The entry checks the pointers and their alignment (items and h 8 bytes, the other outputs 4), 1 <= B <= 65535,
 * 1 <= P <= S <= 16384, std != 0, mean and std not NaN; align_corners is read as zero / non-zero.                                          */
int hesic_homonet_synth_items(const hesic_homonet_synth_item* items, int B, int S, int P, float mean, float std, int align_corners,
                              float* grey_a, float* patch_a, float* corners, float* delta, double* h, float* grey_b, float* patch_b,
                              void* stream);

#ifdef __cplusplus
}
#endif
#endif /* HESIC_HOMONET_SYNTH_H */

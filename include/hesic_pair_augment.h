/* hesic_pair_augment.h -- hesic_pair_batch_gather (hesic_pair_batch.h) with stereo-aware augmentation per item: a horizontal flip, a vertical
 * flip and an exchange of the two views, each carried through to the homography that travels with the pixels.  Same descriptors, same
 * outputs, still one launch.  Exported by both libraries (libhesic_hip.so, libhesic_hip_f16.so); an addition to HESIC_ABI_VERSION 2.  The
 * entry is declared here and not in hesic_pair_batch.h, whose list of entries stays what it is; hesic_hip.h does not include this header.
 *
 * Conventions as in hesic_hip.h: DEVICE pointers, `stream` a hipStream_t, asynchronous; return 0 or a hipError_t (> 0) or HESIC_EINVAL (-1),
 * with hesic_last_error() describing the failure.  No atomics, no LDS, no shared state: the same inputs give the same bits.               */
#ifndef HESIC_PAIR_AUGMENT_H
#define HESIC_PAIR_AUGMENT_H
#include "hesic_pair_batch.h"
#ifdef __cplusplus
extern "C" {
#endif

/* hesic_pair_item.reserved as this entry reads it: any combination of these bits.  The entry cannot read the descriptors (they are in
 * device memory), so it CANNOT refuse other bits: it ignores them.  The caller refuses them (functional.pair_batch_gather_aug does). */
#define HESIC_PAIR_HFLIP 1 /* both views mirrored left-right  */
#define HESIC_PAIR_VFLIP 2 /* both views mirrored top-bottom  */
#define HESIC_PAIR_SWAP 4  /* x1 from the right view, x2 from the left view */

/* Arguments, caller's guarantees, alignment and shape limits exactly as hesic_pair_batch_gather; hesic_pair_item keeps its layout (48 bytes).
 * Every element of the three outputs is written.  Per item b with f = items[b].reserved:
 *
 * Pixels.  A is the right view if f & SWAP, else the left view; B is the other one.
 *   r' = ph - 1 - r if f & VFLIP, else r;   q' = pw - 1 - q if f & HFLIP, else q
 *   x1[b, c, r, q] = (float)A[y0 + r', x0 + q', c] / 255.0f   (one IEEE division, as hesic_pair_batch_gather);  x2 likewise from B.
 *
 * Matrix, for h_index >= 0 (with h_index = -1 h_out[b] is the identity whatever the flags).  In fp64, every product, sum and difference
 * rounded on its own (no fused multiply-add).  It starts from R, the re-based matrix BEFORE its division exactly as hesic_pair_batch.h
 * forms it (G0 = H0 - hx * H2; G1 = H1 - hy * H2; G2 = H2; R[:,0] = G[:,0]; R[:,1] = G[:,1]; R[:,2] = (G[:,0] * hx + G[:,1] * hy) + G[:,2]).
 * The steps run in this order, each only when its flag is set:
 *   HFLIP, with a = (double)(pw - 1)      [R <- F R F, F = [[-1, 0, a], [0, 1, 0], [0, 0, 1]], its own inverse]
 *     S0j = a * R2j - R0j,  S1j = R1j,  S2j = R2j                 for j = 0..2
 *     Ti0 = -Si0,  Ti1 = Si1,  Ti2 = a * Si0 + Si2                for i = 0..2
 *     R <- T
 *   VFLIP, with c = (double)(ph - 1)      [the same on row 1 and column 1]
 *     S0j = R0j,  S1j = c * R2j - R1j,  S2j = R2j                 for j = 0..2
 *     Ti0 = Si0,  Ti1 = -Si1,  Ti2 = c * Si1 + Si2                for i = 0..2
 *     R <- T
 *   SWAP: R <- adj(R), each entry one difference of two products, with m = R   [the inverse up to the determinant, which the
 *     U00 = m11 * m22 - m12 * m21,  U01 = m02 * m21 - m01 * m22,  U02 = m01 * m12 - m02 * m11       normalisation below removes]
 *     U10 = m12 * m20 - m10 * m22,  U11 = m00 * m22 - m02 * m20,  U12 = m02 * m10 - m00 * m12
 *     U20 = m10 * m21 - m11 * m20,  U21 = m01 * m20 - m00 * m21,  U22 = m00 * m11 - m01 * m10
 *     R <- U
 *   h_out[b][i][j] = (float)(R[i][j] / R[2][2])
 * With f = 0 for every item the three outputs are the bits of hesic_pair_batch_gather.
 *
 * Memory: nothing is read outside [view, view + rows * pitch_px * 3) of an item's two views, the descriptors and the named table rows --
 * under HFLIP too, where a row's FIRST output thread reads the crop's last columns and its last thread the first; nothing is written
 * outside the three outputs.  pw need not be a multiple of 4: with HFLIP the partial group of a row lies at the row's end in the output
 * and at the crop's first columns in the source.
 * One launch of (B * ceil(ph * ceil(pw / 4) / 256)) x 2 blocks of 256 threads, the shape of hesic_pair_batch_gather: a thread owns four
 * consecutive OUTPUT pixels of one row (16 bytes into each of the three channel planes, 16-byte stores when pw % 4 == 0 and x1, x2 are
 * 16-byte aligned), reads the 12 source bytes they come from -- contiguous under every flag -- and reverses the four pixels in registers
 * under HFLIP; blockIdx.y is the OUTPUT (0: x1, 1: x2); the first thread of an item's first x1 block also writes its matrix.            */
int hesic_pair_batch_gather_aug(const hesic_pair_item* items, const double* h_table, int B, int ph, int pw, float* x1, float* x2, float* h_out,
                                void* stream);

#ifdef __cplusplus
}
#endif
#endif /* HESIC_PAIR_AUGMENT_H */

/* hesic_pair_batch.h -- a training batch of stereo crops gathered from uint8 images that live on the device, in one launch: what the loader
 * does per item on the host (compressai/datasets/utils.py:140-160; here compressai.datasets.ImageFolder.__getitem__: crop both views at one
 * offset, ToTensor, re-base the sidecar homography to the crop).  Exported by both libraries (libhesic_hip.so, libhesic_hip_f16.so); an
 * addition to HESIC_ABI_VERSION 2.  hesic_hip.h does not include this header.
 *
 * Conventions as in hesic_hip.h: DEVICE pointers, `stream` a hipStream_t, asynchronous; return 0 or a hipError_t (> 0) or HESIC_EINVAL (-1),
 * with hesic_last_error() describing the failure.  No atomics, no shared state: the same inputs give the same bits.                          */
#ifndef HESIC_PAIR_BATCH_H
#define HESIC_PAIR_BATCH_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

typedef struct {
    const uint8_t* left;    /* stored left view: (rows, pitch_px, 3) uint8 RGB, dense */
    const uint8_t* right;   /* stored right view, same geometry */
    int32_t pitch_px, rows; /* stored image: pixels per row, rows */
    int32_t x0, y0;         /* crop origin inside the STORED image */
    int32_t hx, hy;         /* crop origin in the FULL image: the translation H is re-based by */
    int32_t h_index;        /* row of h_table, or -1: no matrix for this item */
    int32_t reserved;       /* 0 (hesic_pair_augment.h's entry reads its flip / swap bits here) */
} hesic_pair_item;          /* 48 bytes */

/* items: B descriptors in DEVICE memory (8-byte aligned).  The stored image and the full image differ when the caller uploads only the crop
 * (x0 = y0 = 0, pitch_px = pw, rows = ph, hx / hy the crop's origin in the file): the pixels come from (x0, y0), the matrix moves by (hx, hy).
 * The CALLER guarantees, per item, 0 <= x0, x0 + pw <= pitch_px, 0 <= y0, y0 + ph <= rows and h_index in [-1, N): the entry cannot read the
 * descriptors.  Every element of the three outputs is written:
 *   x1, x2 (B, 3, ph, pw) fp32 dense   x[b, c, r, q] = (float)byte / 255.0f  (IEEE division: torchvision's ToTensor, bit for bit) with
 *                                      byte = view[((y0 + r) * pitch_px + (x0 + q)) * 3 + c]
 *   h_out  (B, 3, 3) fp32              T(-t) H T(t) / [2,2] with t = (hx, hy) and H = h_table[h_index] (fp64 (N, 9) row-major; may be NULL
 *                                      when every h_index is -1); the identity where h_index is -1.  In fp64, every operation rounded on its
 *                                      own (no fused multiply-add), with H0, H1, H2 the rows of H:
 *                                        G0 = H0 - hx * H2;  G1 = H1 - hy * H2;  G2 = H2
 *                                        R[:,0] = G[:,0];  R[:,1] = G[:,1];  R[:,2] = (G[:,0] * hx + G[:,1] * hy) + G[:,2]
 *                                        h_out = (float)(R / R[2][2])
 * Memory: nothing is read outside [view, view + rows * pitch_px * 3) of an item's two views, the descriptors and the named table rows;
 * nothing is written outside the three outputs.  x0 * 3 may have any alignment; pw need not be a multiple of 4 (16-byte stores are used
 * when it is and x1, x2 are 16-byte aligned, 4-byte stores otherwise).
 * B, ph, pw >= 1 and B * 3 * ph * pw <= INT32_MAX.  One launch of (B * ceil(ph * ceil(pw / 4) / 256)) x 2 blocks of 256 threads: a thread
 * owns four consecutive pixels of one crop row (12 source bytes, 16 bytes into each of the three channel planes), blockIdx.y is the view;
 * the first thread of an item's first left-view block also writes its matrix.                                                              */
int hesic_pair_batch_gather(const hesic_pair_item* items, const double* h_table, int B, int ph, int pw, float* x1, float* x2, float* h_out,
                            void* stream);

#ifdef __cplusplus
}
#endif
#endif /* HESIC_PAIR_BATCH_H */

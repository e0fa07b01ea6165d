/* hesic_homography_prep.h -- a stereo pair on the device becomes HomographyNet's inputs in one launch: the step the `_real` scripts' loader
 * does per item on the host (compressai/datasets/utils.py:161-186; here compressai.datasets.ImageFolder._homonet_inputs): both views
 * resized to S x S (cv2.resize INTER_LINEAR in its float form: half-pixel centres, no anti-aliasing), quantised to grey levels, ToTensor,
 * Normalize, averaged to grey, one P x P window cut from each with its corner coordinates.  Exported by both libraries (libhesic_hip.so,
 * libhesic_hip_f16.so); an addition to HESIC_ABI_VERSION 2.  hesic_hip.h does not include this header.
 *
 * Conventions as in hesic_hip.h: DEVICE pointers, element strides, `stream` a hipStream_t, asynchronous; return 0 or a hipError_t (> 0) or
 * HESIC_EINVAL (-1), with hesic_last_error() describing the failure.  No atomics, no shared memory: the same inputs give the same bits.
 *
 * The same step for a batch whose views are STORED uint8 images, each at its own address and of its own size (a device-resident folder):
 * hesic_homonet_prepare_items in hesic_homonet_items.h, included at the end of this header -- one kernel source, the same device functions
 * per axis, tap and level, the same bits.                                                                                                */
#ifndef HESIC_HOMOGRAPHY_PREP_H
#define HESIC_HOMOGRAPHY_PREP_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

/* element type of x1 / x2 */
#define HESIC_PREP_U8 0  /* bytes: the level of a sample is the byte                                                                     */
#define HESIC_PREP_F32 1 /* fp32 in [0, 1]: the level is rint(255 * v) clamped to [0, 255] (exact for v = u / 255); NaN is out of contract */

/* x1, x2 (B, 3, H, W) of `dtype` with element strides xs1[4] / xs2[4] (HOST arrays) = (batch, channel, row, column), each >= 0 (NCHW, channels-last, a
 * crop view of a larger tensor; the two views may differ in strides).  xy (B, 2) int32: the window origin (x, y) of item b, 0 <= x, y <=
 * S - P (the CALLER checks the range: the kernel writes a window element only where it lies inside the S x S frame, so a value outside
 * the range cannot write out of bounds but leaves part of the window unwritten).  All outputs are fp32, dense, and every element is
 * written:
 *   grey1, grey2   (B, 1, S, S)   the normalised grey frames
 *   patch1, patch2 (B, 1, P, P)   grey[:, :, y:y+P, x:x+P]
 *   corners        (B, 4, 2)      [[x, y], [x+P, y], [x+P, y+P], [x, y+P]]
 * The arithmetic, in fp32, every operation rounded on its own (no fused multiply-add).  Per axis of length n, for output index d:
 *   scale = (float)n / (float)S;  s = max(scale * (d + 0.5f) - 0.5f, 0);  i0 = min((int)s, n - 1);  i1 = min(i0 + 1, n - 1);
 *   l1 = s - i0;  l0 = 1 - l1
 * per channel, with a, b the levels at (y0, x0), (y0, x1) and c, d those at (y1, x0), (y1, x1):
 *   v = hy0 * (wx0 * a + wx1 * b) + hy1 * (wx0 * c + wx1 * d);  r = clamp(rint(v), 0, 255)      (ties to even)
 * and  grey = ((r0 / 255 - mean) / std + (r1 / 255 - mean) / std + (r2 / 255 - mean) / std) / 3   with IEEE division, summed left to right.
 * 1 <= P <= S; std != 0.  One launch of ceil(S * S / 256) x B x 2 blocks of 256 threads, one grey element per thread.                     */
int hesic_homonet_prepare(const void* x1, const int64_t* xs1, const void* x2, const int64_t* xs2, const int32_t* xy, int B, int H, int W, int S,
                          int P, float mean, float std, int dtype, float* grey1, float* grey2, float* patch1, float* patch2, float* corners,
                          void* stream);

#ifdef __cplusplus
}
#endif
#include "hesic_homonet_items.h"
#endif /* HESIC_HOMOGRAPHY_PREP_H */

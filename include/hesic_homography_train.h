/* hesic_homography_train.h -- gradients through the geometry in front of the stereo path: the photometric loss that trains HomographyNet
 * (ywz/mywork/model.py:18-45) with its backward to the corner deltas, the gradient of warp_perspective with respect to its matrix, and the
 * adjoint of the 4-point DLT (hesic_perspective_transform / hesic_h_from_delta of hesic_hip.h).  Exported by both libraries
 * (libhesic_hip.so, libhesic_hip_f16.so); an addition to HESIC_ABI_VERSION 2.  Includes hesic_hip.h for hesic_warp_desc; hesic_hip.h does
 * not include this header.
 *
 * Every reduction here is two launches -- per-block fp64 partials in a caller-provided workspace, then a finishing launch that adds them in
 * a fixed order -- with no atomics and no host read: the same inputs give the same bits in every run.                                   */
#ifndef HESIC_HOMOGRAPHY_TRAIN_H
#define HESIC_HOMOGRAPHY_TRAIN_H
#include <stdint.h>
#include "hesic_hip.h"
#ifdef __cplusplus
extern "C" {
#endif

/* `partials` of the three image-sized entry points below holds B * HESIC_HTRAIN_MAX_BLOCKS * HESIC_HTRAIN_PARTIAL_WIDTH fp64 values (every
 * entry that is read is written first).                                                                                                  */
#define HESIC_HTRAIN_MAX_BLOCKS 64
#define HESIC_HTRAIN_PARTIAL_WIDTH 9

/* loss = mean | bilinear(img_a, h p) - patch_b(p) | over B x C x Ho x Wo, zeros outside the image, with
 *     c0 = corners - corners[:,0];  h = DLT(c0 -> corners + delta)   (h22 = 1; fp64 from the fp32 inputs on)
 * i.e. F.l1_loss(kornia.warp_perspective(img_a, inverse(h), patch_b.shape[-2:]), patch_b) without the inversion pair.
 * `d`: B, C, H, W of img_a with its strides ss_*; Ho, Wo of patch_b with its strides ds_*; align_corners as in hesic_warp_desc; both images
 * fp32 (src_dtype = dst_dtype = HESIC_F32); m_is_dst_to_src is ignored.  corners, delta: (B,4,2) fp32 contiguous.  Outputs: h (B,9) fp64 --
 * hesic_photometric_backward reads it -- and loss, one fp32.  Three launches: DLT (one thread per pair), sample + |diff| partials, finish. */
int hesic_photometric_forward(const hesic_warp_desc* d, const float* img_a, const float* patch_b, const float* corners, const float* delta,
                              double* h, double* partials, float* loss, void* stream);

/* d_delta (B,4,2) fp32 = grad_loss[0] * d loss / d delta.  Per pixel the taps are recomputed; with sign(0) = 0 and an out-of-image tap
 * counted as 0 (grid_sample's zero-padding gradient) the eight free entries of h get their per-block partials, and the finishing launch
 * (one thread per pair, fp64) scales them by grad_loss[0] / (B C Ho Wo), read from device memory, and applies the DLT adjoint.            */
int hesic_photometric_backward(const hesic_warp_desc* d, const float* img_a, const float* patch_b, const float* corners, const float* delta,
                               const double* h, const float* grad_loss, double* partials, float* d_delta, void* stream);

/* The gradient of hesic_warp_perspective_forward with respect to its matrix: dM (B,9) fp32 from d_dst (dst_dtype, strides ds_*) and src
 * (src_dtype, strides ss_*).  With m_is_dst_to_src = 0 the kernel inverts M as the forward does and dM = -M^-T dA M^-T for the gradient dA
 * of the destination -> source matrix A = M^-1; with m_is_dst_to_src = 1, dM = dA.                                                      */
int hesic_warp_perspective_backward_m(const hesic_warp_desc* d, const void* src, const void* d_dst, const float* M, double* partials,
                                      float* dM, void* stream);

/* Adjoint of hesic_perspective_transform: d_src, d_dst (B,4,2) fp32 (either may be null) from dH (B,9) fp32 (dH[8] is ignored: h22 = 1). */
int hesic_perspective_transform_backward(const float* src, const float* dst, const float* dH, float* d_src, float* d_dst, int B,
                                         void* stream);

/* Adjoint of hesic_h_from_delta with respect to delta: through h_adjust, the 3x3 inverse and the DLT.                                    */
int hesic_h_from_delta_backward(const float* corners, const float* delta, float ratio_a, float ratio_b, int subtract_origin,
                                const float* dH, float* d_delta, int B, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* HESIC_HOMOGRAPHY_TRAIN_H */

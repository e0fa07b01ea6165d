/*
 * hesic_stereo_h.h -- C ABI of the stereo homography estimator in libhesic_hip.so / libhesic_hip_f16.so
 * (hesic_amd/csrc/stereo_h.hip): the GPU form of the reference loader's get_H (compressai/datasets/utils.py:30-66:
 * SURF keypoints, 2-NN brute-force matching with the 0.7 ratio test, findHomography(RANSAC, 5.0)).
 *
 * Conventions as in hesic_hip.h: DEVICE pointers, element counts and strides, `stream` a hipStream_t, asynchronous; return 0 or a
 * hipError_t (> 0) or HESIC_EINVAL (-1), with hesic_last_error() describing the failure.  The kernels do not depend on the library's
 * 16-bit storage format.
 *
 * A batch is B same-size pairs; images are numbered n = 0..2B-1 with view 1 (left) of pair b at n = b and view 2 (right) at n = B + b.
 * Per-image arrays:
 *   I      (2B, H+1, W+1) int32        integral image of the grey level
 *   det    (2B, hesic_stereo_h_det_elems(H, W)) fp32   Hessian responses of the 20 layers (4 octaves x 5), each (H/step) x (W/step)
 *   kp     (2B, max_kp, 4) fp32        keypoints [x, y, size, response], the first n_kp[n] valid, in generation order
 *   desc   (2B, max_kp, 64) fp32       U-SURF descriptors; nrm (2B, max_kp) their squared norms
 *          (2B, max_kp, dim) fp32      with the _ex entry points: dim = 64 or 128 (extended), upright or oriented
 *   ori    (2B, max_kp, 2) fp32        keypoint directions [cos, sin] (x right, y down); (1, 0) is upright
 * Per-pair arrays:
 *   matches (B, max_kp, 2) int32       [query in view 1, train in view 2], the first n_match[b] valid, in query order
 *   H_out (B, 9) fp32 (left -> right pixels, h33 = 1; zeros when invalid), valid / inliers / best (B) int32,
 *   inlier_mask (B, max_kp) uint8 over the matches
 * ws: one workspace of hesic_stereo_h_ws_bytes(B, H, W, max_kp, n_hyp) bytes shared by the stages of one batch.
 */
#ifndef HESIC_STEREO_H_H
#define HESIC_STEREO_H_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define HESIC_STEREO_H_MAX_KEYPOINTS 4096   /* the RANSAC stage stages every match (16 bytes) in 64 KB of LDS */

int64_t hesic_stereo_h_det_elems(int H, int W);
size_t hesic_stereo_h_ws_bytes(int B, int H, int W, int max_kp, int n_hyp);
/* grey (cvtColor BGR2GRAY of the RGB data, as the reference's SURF sees it) + integral image of N (3, H, W) images with element strides
   (sb, sc, sy, sx); is_f32 = 0: uint8, 1: fp32 in [0, 1] quantised as rint(clamp(x, 0, 1) * 255) */
int hesic_stereo_h_integral(const void* img, int is_f32, int64_t sb, int64_t sc, int64_t sy, int64_t sx, int N, int H, int W, int32_t* I,
                            void* stream);
/* Fast-Hessian responses (OpenCV SURF's box filters, det = Dxx Dyy - 0.81 Dxy^2) of every layer of N images */
int hesic_stereo_h_hessian(const int32_t* I, int N, int H, int W, float* det, void* stream);
/* 3x3x3 NMS above hessianThreshold = 100, quadratic sub-pixel / sub-scale fit, the strongest max_kp of each of the 2B images */
int hesic_stereo_h_keypoints(const float* det, int B, int H, int W, int max_kp, int n_hyp, void* ws, size_t ws_bytes, float* kp,
                             int32_t* n_kp, void* stream);
/* upright 64-d SURF descriptors of the first n_kp[n] keypoints of each of N images */
int hesic_stereo_h_describe(const int32_t* I, const float* kp, const int32_t* n_kp, int N, int H, int W, int max_kp, float* desc, float* nrm,
                            void* stream);
/* 2-NN of every view-1 descriptor over view 2 (squared L2 on the matrix cores), ratio test d1^2 < 0.49 d2^2, compacted in query order */
int hesic_stereo_h_match(const float* desc, const float* nrm, const int32_t* n_kp, int B, int H, int W, int max_kp, int n_hyp, void* ws,
                         size_t ws_bytes, int32_t* matches, int32_t* n_match, void* stream);
/* dominant direction of the first n_kp[n] keypoints of each of N images (OpenCV SURF's orientation: 109 Haar samples of size
   4 s in a radius of 6 s, the longest summed response over 60-degree windows in steps of 5 degrees); (1, 0) where no window has a
   non-zero sum.  max_kp <= HESIC_STEREO_H_MAX_KEYPOINTS */
int hesic_stereo_h_orient(const int32_t* I, const float* kp, const int32_t* n_kp, int N, int H, int W, int max_kp, float* ori, void* stream);
/* SURF descriptors of dim = 64 or 128 (extended: each sum split by the sign of the other response) components, in the frame of ori
   (NULL: upright; ori = (1, 0) everywhere with dim = 64 gives hesic_stereo_h_describe's bits) */
int hesic_stereo_h_describe_ex(const int32_t* I, const float* kp, const float* ori, const int32_t* n_kp, int N, int H, int W, int max_kp,
                               int dim, float* desc, float* nrm, void* stream);
/* hesic_stereo_h_match on descriptors of dim = 64 or 128 components (dim = 64 gives hesic_stereo_h_match's result) */
int hesic_stereo_h_match_ex(const float* desc, const float* nrm, const int32_t* n_kp, int B, int H, int W, int max_kp, int n_hyp, int dim,
                            void* ws, size_t ws_bytes, int32_t* matches, int32_t* n_match, void* stream);
/* RANSAC (n_hyp hypotheses from a counter hash of (seed, pair_ids[b], hypothesis, draw), reprojection error <= 5 px), best
   hypothesis, inlier mask, least-squares DLT + 10 Levenberg-Marquardt steps over its inliers */
int hesic_stereo_h_ransac(const float* kp, const int32_t* matches, const int32_t* n_match, int B, int H, int W, int max_kp, int n_hyp,
                          uint32_t seed, const uint32_t* pair_ids, void* ws, size_t ws_bytes, float* H_out, int32_t* valid, int32_t* inliers,
                          int32_t* best, uint8_t* inlier_mask, void* stream);

#ifdef __cplusplus
}
#endif

#endif

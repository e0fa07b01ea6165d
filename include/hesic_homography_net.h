/* hesic_homography_net.h -- what HomographyNet (ywz/mywork/model.py:73-101) needs to TRAIN beside the conv kernels of hesic_hip.h: the backward
 * of MaxPool2d(2,2), the flatten + Dropout pair of `fc` in both directions, and a small-batch Linear layer over the fp32 master weight
 * (forward, data gradient, weight / bias gradient).  Exported by both libraries (libhesic_hip.so, libhesic_hip_f16.so); an addition to
 * HESIC_ABI_VERSION 2.  hesic_hip.h does not include this header.
 *
 * No kernel here uses atomics and every sum has a fixed order: the same inputs give the same bits in every run.  `dtype` (HESIC_F32 /
 * HESIC_H16) is the storage type T of the ACTIVATIONS and their gradients; weights, biases and their gradients are always fp32.          */
#ifndef HESIC_HOMOGRAPHY_NET_H
#define HESIC_HOMOGRAPHY_NET_H
#include <stddef.h>
#include <stdint.h>
#include "hesic_hip.h"
#ifdef __cplusplus
extern "C" {
#endif

/* Backward of hesic_maxpool2_forward.  x (B,H,W,C), gy (B,H/2,W/2,C), gx (B,H,W,C), all NHWC of type T, C % (16 / sizeof(T)) == 0.  The
 * argmax is recomputed from x: the window is scanned (0,0), (0,1), (1,0), (1,1) and a later element replaces the maximum only if it is
 * strictly greater (torch's rule; a window of equal values sends its gradient to (0,0)).  EVERY element of gx is written: zero for the
 * non-maxima and for the last row / column of an odd H / W, which the forward ignores.                                                  */
int hesic_maxpool2_backward(const void* x, const void* gy, void* gx, int B, int H, int W, int C, int dtype, void* stream);

/* y (B, F = C*HW) row-major of type T from the NHWC map x (B, HW, C): the reference's NCHW flatten order j = c*HW + p, with inverted
 * dropout applied on the way.  Needs C % 4 == 0 when HW > 1, and F % 4 == 0.
 *     word(b, j) = Philox4x32-10(counter = (q lo, q hi, step, site), key = (seed lo, seed hi))[(b*F + j) & 3],  q = (b*F + j) >> 2
 *     y[b, j]    = word >= thr ? x * scale (one fp32 product, stored in T) : +0
 * thr = llrint(p * 2^32) clamped to [0, 2^32 - 1]; scale = 1.0f / (1.0f - (float)p).  thr = 0, scale = 1 is the plain permutation.  The
 * mask is a function of the logical index alone; the backward regenerates it (gx (B, HW, C) from gy (B, F)), nothing is stored.          */
int hesic_flatten_dropout_forward(const void* x, void* y, int B, int HW, int C, uint32_t thr, float scale, uint64_t seed, uint32_t step,
                                  uint32_t site, int dtype, void* stream);
int hesic_flatten_dropout_backward(const void* gy, void* gx, int B, int HW, int C, uint32_t thr, float scale, uint64_t seed, uint32_t step,
                                   uint32_t site, int dtype, void* stream);

/* y = act(x W^T + bias) for few rows: x (B, In) of type T, W (Out, In) fp32 in nn.Linear's layout (read once, no packed copy), bias (Out)
 * fp32 or null, fp32 accumulation.  1 <= B <= HESIC_LINEAR_MAX_ROWS, In % 4 == 0, any Out >= 1.  A row's result does not depend on B.     */
#define HESIC_LINEAR_MAX_ROWS 64

/* The forward splits In over blocks: fp32 partial sums go to `ws` (hesic_linear_forward_ws_bytes(B, In, Out) bytes, every entry that is
 * read is written first) and a finishing launch adds the slices in ascending order, then the bias, and applies act (HESIC_ACT_NONE or
 * HESIC_ACT_RELU).  y (B, Out) of type T.                                                                                                */
size_t hesic_linear_forward_ws_bytes(int B, int In, int Out);
int hesic_linear_forward(const void* x, const float* W, const float* bias, void* y, int B, int In, int Out, int act, int dtype, void* ws,
                         size_t ws_bytes, void* stream);

/* gx[b,i] = sum_o gy[b,o] W[o,i].  gy (B, Out) and gx (B, In) of type T.  One launch; the contraction is split over the four waves of a
 * block only (summed in wave order), so no workspace.                                                                                   */
int hesic_linear_dgrad(const void* gy, const float* W, void* gx, int B, int In, int Out, int dtype, void* stream);

/* dW[o,i] = sum_b gy[b,o] x[b,i] (b ascending) and, unless db is null, db[o] = sum_b gy[b,o].  accumulate != 0 adds into dW / db in place,
 * accumulate == 0 overwrites them.  dW is touched once per call.                                                                         */
int hesic_linear_wgrad(const void* x, const void* gy, float* dW, float* db, int B, int In, int Out, int accumulate, int dtype, void* stream);

/* Order-fixed forms of two conv gradients whose usual kernels end in float atomics (last bits that change from run to run): per-block
 * partial sums over pixel ranges that depend on the sizes alone, in `ws`, added in block order by a second launch.  `ws` holds
 * HESIC_DET_MAX_BLOCKS * n floats, n = the number of outputs (every entry that is read is written first).  accumulate as in hesic_linear_wgrad.
 *   hesic_bias_grad:       db[c] (+)= sum_p gy[p, c] over the P rows of an NHWC gradient of type T; C divides 256.
 *   hesic_narrow_in_wgrad: dW (Cout, Cin, 3, 3) (+)= the weight gradient of a 3x3, stride 1, padding 1 conv with Cin = 2 input channels; x
 *                          (B, Cin, H, W) fp32 contiguous, gy (B, H, W, Cout) NHWC of type T; Cout divides 256.                            */
#define HESIC_DET_MAX_BLOCKS 256
int hesic_bias_grad(const void* gy, float* db, float* ws, int64_t P, int C, int accumulate, int dtype, void* stream);
int hesic_narrow_in_wgrad(const float* x, const void* gy, float* dW, float* ws, int B, int Cin, int H, int W, int Cout, int accumulate,
                          int dtype, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* HESIC_HOMOGRAPHY_NET_H */

/* hesic_en_train.h -- the stage-2 (enhancement net) training step's own kernels: the criterion of ywz/mywork/newtrain6_real.py:82-88 for both
 * views in one call, its gradient written straight into the map the 32 -> 3 output layer's backward consumes, and the data-gradient weights of
 * every 3x3 conv of a flat parameter buffer in one launch.  Exported by both libraries (libhesic_hip.so, libhesic_hip_f16.so); an addition to
 * HESIC_ABI_VERSION 2.  hesic_hip.h does not include this header.
 *
 * Conventions as in hesic_hip.h: DEVICE pointers, `stream` a hipStream_t, asynchronous; return 0 or a hipError_t (> 0) or HESIC_EINVAL (-1),
 * with hesic_last_error() describing the failure.  No atomics, no memset, no host synchronisation: capturable in a graph, and the same
 * inputs give the same bits, eagerly and in a replay.                                                                                    */
#ifndef HESIC_EN_TRAIN_H
#define HESIC_EN_TRAIN_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

/* Bytes of workspace hesic_en_loss needs for B pairs of H x W images; -1 (with a message) for arguments hesic_en_loss would refuse. */
int64_t hesic_en_loss_ws_bytes(int B, int H, int W);

/* out[4] fp64, every element WRITTEN: {sse1, sse2, mse_loss, loss} with sse_v = sum((a_v - b_v)^2) over the dense fp32 planar (B,3,H,W)
 * operands of view v, mse_loss = sse1 / n + sse2 / n, n = B * 3 * H * W, loss = lambda_255sq * mse_loss (the caller passes lambda * 255^2).
 * Per element d = a - b in fp32, widened to fp64, squared and accumulated in fp64: every term is exact and non-negative.
 * Launch 1: the 3 * H * W elements of every (view, image) are cut into a number of blocks that depends only on H * W (4096 elements a
 * block, at most 64), each of which writes one fp64 partial to `ws`.  Launch 2: one wave per view adds that view's B * blocks partials in
 * index order.  Operands that are 16-byte aligned image by image are read with 16-byte loads, others with 4-byte loads by the same lanes in
 * the same order: the bits do not depend on the alignment.  A NaN operand makes the sums of its view (and mse_loss, loss) NaN.
 * B, H, W >= 1, B <= 2^20, H * W < 2^31; operands 4-byte aligned; out and ws 8-byte aligned, ws_bytes >= hesic_en_loss_ws_bytes(B, H, W). */
int hesic_en_loss(const float* a1, const float* b1, const float* a2, const float* b2, int B, int H, int W, double lambda_255sq, double* out,
                  void* ws, int64_t ws_bytes, void* stream);

/* The gradient of that loss w.r.t. a1 and a2, one launch: g_v (B,H,W,32) NHWC in the library's 16-bit format, channel c < 3 of pixel (y, x) of
 * image i = round16(s * (a_v[i][c][y][x] - b_v[i][c][y][x])) -- a subtract, then a multiply, in fp32, then one round to nearest even (no
 * saturation: a NaN operand gives a NaN in exactly that element) -- and channels 3..31 WRITTEN as zero.  s = (float)(2 * lambda_255sq / n),
 * computed in double and rounded once; with `seed` not NULL, s is multiplied in fp32 by seed[0] (the gradient of the caller's own scalar
 * w.r.t. the loss; NULL = backward() on the unscaled loss).  g1, g2 16-byte aligned.  B, H, W >= 1, H * W < 2^31.                       */
int hesic_en_loss_grad(const float* a1, const float* b1, const float* a2, const float* b2, int B, int H, int W, double lambda_255sq,
                       const float* seed, void* g1, void* g2, void* stream);

/* One conv layer of hesic_c32_mirror_weights: offsets in floats from `src` / `dst`.                                                       */
typedef struct {
    int64_t src;       /* (cout, cin, 3, 3) fp32 */
    int64_t dst;       /* (cin, cout_pad, 3, 3) fp32 */
    int32_t cout, cin; /* 1..32 each */
    int32_t cout_pad;  /* cout <= cout_pad <= 32: rows cout..cout_pad-1 of every input channel are written as zero */
    int32_t reserved;
} hesic_mirror_entry;

/* dst[e.dst + ((ci * cout_pad + co) * 3 + ky) * 3 + kx] = co < cout ? src[e.src + ((co * cin + ci) * 3 + 2 - ky) * 3 + 2 - kx] : 0 for every
 * entry e of the DEVICE table: the weight of the data-gradient conv (input and output channels exchanged, taps mirrored), a pure permutation
 * with zero padding.  An entry whose dimensions are out of range, or whose source / destination does not lie inside src_numel / dst_numel
 * floats, is skipped as a whole (nothing outside the two buffers is ever touched).  1 <= n_layers <= capacity (the entries `table` holds).   */
int hesic_c32_mirror_weights(const float* src, int64_t src_numel, float* dst, int64_t dst_numel, const hesic_mirror_entry* table, int n_layers,
                             int capacity, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* HESIC_EN_TRAIN_H */

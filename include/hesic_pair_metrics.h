/* hesic_pair_metrics.h -- the rate-distortion sums of a batch PER PAIR: what the reference's evaluation gets by running at
 * --test-batch-size 1 (ywz/mywork/test3real.py:3,90-122: bits, MSE and PSNR per pair, then averaged), for a whole batch in two launches.
 * Exported by both libraries (libhesic_hip.so, libhesic_hip_f16.so); an addition to HESIC_ABI_VERSION 2.  hesic_hip.h does not include
 * this header.
 *
 * Conventions as in hesic_hip.h: DEVICE pointers, `stream` a hipStream_t, asynchronous; return 0 or a hipError_t (> 0) or HESIC_EINVAL (-1),
 * with hesic_last_error() describing the failure.  No atomics, no memset, no host synchronisation: capturable in a graph, and the same
 * inputs give the same bits.                                                                                                            */
#ifndef HESIC_PAIR_METRICS_H
#define HESIC_PAIR_METRICS_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define HESIC_PAIR_METRICS_MAX_LIK 8

/* Bytes of workspace hesic_pair_metrics needs for B pairs, n_lik likelihood maps of numel[i] elements each (the whole batch) and H x W
 * images; -1 (with a message) for arguments hesic_pair_metrics would refuse.  numel may be NULL when n_lik is 0.                        */
int64_t hesic_pair_metrics_ws_bytes(int B, int n_lik, const int64_t* numel, int H, int W);

/* out (B, n_lik + 4) fp64, row-major, every element WRITTEN (not added to; no zero-fill needed):
 *   out[b][i], i < n_lik   sum(log2(lik[i][e])) over image b's slice e in [b * per_i, (b + 1) * per_i), per_i = numel[i] / B: the maps
 *                          are fp32 with the batch outermost (dense NCHW or channels-last).  Per term log2f in fp32, widened to fp64,
 *                          accumulated in fp64 (the arithmetic of hesic_sum_log2).  16-byte loads are used for an image whose slice
 *                          starts on a 16-byte boundary and 4-byte loads otherwise; the order of the additions is the same in both.
 *   out[b][n_lik + s]      s = 0, 1: sum((a_s - b_s)^2) over the C x H x W window of image b of the pair (a[s], b[s]).  Operands of
 *                          dtype HESIC_F32 / HESIC_H16 with four element strides (batch, channel, row, column) each: a cropped view of
 *                          a padded reconstruction is described by its strides, and nothing outside the window is read.  Per pixel an
 *                          fp32 fmaf chain over the channels (restarted every 8), widened to fp64 (the arithmetic of hesic_sum_sq_diff).
 *   out[b][n_lik + 2 + s]  the same sum over the 8-bit images a decoder writes: sum((q(a_s) - q(b_s))^2) with
 *                          q(v) = rintf(fminf(fmaxf(v, 0), 1) * 255.f), and q(NaN) = NaN.  An integer, exact in fp64.
 * A NaN in image b's operands makes row b's two sums of that pair NaN and touches no other row.
 * Launch 1: every (image, column) is cut into a number of blocks that depends only on that image's element / pixel count (never on B),
 * each of which reduces its share (wave_sum_d, then four waves in order) and writes one fp64 partial per sum to `ws`.  Launch 2: one
 * wave per (image, column) adds its partials in index order.  Hence a pair's row is the same bits in every batch, at every position.
 * B >= 1, 0 <= n_lik <= 8, numel[i] > 0 and numel[i] % B == 0, C, H, W >= 1, H * W < 2^31; ws 8-byte aligned with
 * ws_bytes >= hesic_pair_metrics_ws_bytes(...).  a, b: two pointers each; a_dtype, b_dtype: two ints each; a_strides, b_strides: 2 x 4.  */
int hesic_pair_metrics(int B, int n_lik, const float* const* lik, const int64_t* numel, const void* const* a, const int* a_dtype,
                       const int64_t* a_strides, const void* const* b, const int* b_dtype, const int64_t* b_strides, int C, int H, int W,
                       double* out, void* ws, int64_t ws_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* HESIC_PAIR_METRICS_H */

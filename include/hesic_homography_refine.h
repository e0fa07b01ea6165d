/* hesic_homography_refine.h -- photometric refinement of a stereo pair's homography: Gauss-Newton with Levenberg-Marquardt damping on the
 * grey image residual, coarse to fine, started from a matrix the caller already has (functional.homography_refine,
 * homography.refine_h_matrix).  Exported by both libraries (libhesic_hip.so, libhesic_hip_f16.so); an addition to HESIC_ABI_VERSION 3.
 *
 * Notation.  H (`h`, fp32, row-major 3x3 per pair) is the h_matrix of HSIC.forward: it maps a pixel of x1 to a pixel of x2.  A = H^-1 scaled
 * to a22 = 1 maps a destination pixel p = (x, y) to its source position w(p) = (X/Z, Y/Z); its eight free entries are the unknowns.  Pixel
 * coordinates follow align_corners = 1 (the legacy half-pixel sampling is not implemented).
 *
 * Conventions of hesic_homography_train.h: device pointers, a stream argument, caller-provided workspaces, no host read, no atomics; every
 * reduction adds in a fixed order (per thread in pixel order, a wave by xor shuffles, the four waves and then the blocks in index order), so
 * equal inputs give equal bits in every run and a pair gives the same bits at any position of a batch.  All arithmetic is fp64 from the fp32
 * pixels on, without fused multiply-adds.  Every workspace entry that is read is written first.                                            */
#ifndef HESIC_HOMOGRAPHY_REFINE_H
#define HESIC_HOMOGRAPHY_REFINE_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define HESIC_HREFINE_MAX_LEVELS 6   /* pyramid levels a call can use                                                                    */
#define HESIC_HREFINE_MIN_SIDE 16    /* levels are built while min(H_l, W_l) >= 16; smaller images are refused                          */
#define HESIC_HREFINE_MAX_BLOCKS 64  /* blocks per pair of the normal-equation launch                                                  */
#define HESIC_HREFINE_SUMS 46        /* 36 upper-triangle sums of w J^T J (row-major, i <= j), 8 of w J^T r, sum w r^2, valid count     */
#define HESIC_HREFINE_STATE 80       /* fp64 words of per-pair state                                                                    */
#define HESIC_HREFINE_INFO 8         /* fp64 words of per-pair report: cost_before, cost_after, accepted, rejected, valid_share,
                                        levels_used, refined (0 / 1), 0                                                                 */

/* Levels actually used for an H x W image: min(levels, available), level l + 1 being (H_l / 2, W_l / 2) (a trailing odd row or column is
 * dropped) while min(H_l, W_l) >= HESIC_HREFINE_MIN_SIDE.  0 for an image below that side, -1 for levels outside [1, MAX_LEVELS].  Host.  */
int hesic_hrefine_levels(int H, int W, int levels);

/* Blocks per pair of the normal-equation launch on an Hl x Wl level: one per 256 pixels, at most HESIC_HREFINE_MAX_BLOCKS.  Host.         */
int hesic_hrefine_blocks(int Hl, int Wl);

/* fp32 elements of the grey pyramid of both views: per used level l, [view 0 | view 1] x [B][H_l][W_l], levels in ascending order.  Host. */
int64_t hesic_hrefine_pyramid_elems(int B, int H, int W, int levels);

/* Bytes of the workspace of hesic_homography_refine: the pyramid, B * MAX_BLOCKS * SUMS fp64 partials, B * STATE fp64 of state and the
 * per-block pixel ranges of x2's levels.  Host.                                                                                          */
int64_t hesic_homography_refine_ws_bytes(int B, int H, int W, int levels);

/* The grey pyramid of both views of the batch in ONE launch.  x1, x2: fp32 (B, C, H, W), C in {1, 3}, element strides s1[4], s2[4] (any
 * non-negative strides: the codec passes un-padded views).  Level 0 is the unweighted channel mean, level l + 1 the 2 x 2 mean of the ROUNDED
 * level l; each is computed in fp64 and rounded once to fp32.  `levels` is the number actually used (hesic_hrefine_levels).               */
int hesic_hrefine_pyramid(const float* x1, const int64_t* s1, const float* x2, const int64_t* s2, int B, int C, int H, int W, int levels,
                          float* pyr, void* stream);

/* The normal equations of one candidate per pair on level `level` of `pyr` (B, H, W, levels as it was built): A of pair b is the nine fp64 at
 * A + b * a_stride, in that level's coordinates.  For destination pixel p: the bilinear sample v of I1 at w(p) from the cell (x0, y0) =
 * floor(w) with taps a b / c d; the cell gradient gx = (b-a)(1-fy) + (d-c)fy, gy = (c-a)(1-fx) + (d-b)fx; valid iff all four taps lie inside
 * I1; r = v - I2(p); J = [gx x, gx y, gx, gy x, gy y, gy, -(gx u + gy v_) x, -(gx u + gy v_) y] / Z with (u, v_) = w(p) (every division by Z
 * is a multiplication by the one reciprocal 1 / Z); weight 1, or with huber = delta > 0, min(1, delta / |r|).  Block j of pair b writes its
 * HESIC_HREFINE_SUMS sums at partials[(b * nblk + j) * SUMS], nblk = hesic_hrefine_blocks(H_l, W_l).  One launch, grid nblk x B.         */
int hesic_hrefine_normal_eq(const float* pyr, int B, int H, int W, int levels, int level, const double* A, int64_t a_stride, double huber,
                            double* partials, void* stream);

/* The whole refinement.  x1, x2 as above; h (B, 9) fp32 contiguous; h_out (B, 9) fp32; info (B, HESIC_HREFINE_INFO) fp64; ws of
 * hesic_homography_refine_ws_bytes.  Per level, coarse to fine, `iters` + 1 candidates are evaluated (one normal-equation launch and one
 * update launch each; the update's decision and solve are one thread per pair):
 *   cost = sum w r^2 / n_valid (0 without a valid pixel).  A candidate is accepted iff it is the level's first, or cost < cost_best and
 *   n_valid >= min_overlap H_l W_l; on accept it becomes the best, its sums are kept and lambda <- max(lambda / 10, 1e-9), otherwise
 *   lambda <- min(10 lambda, 1e6).  Then (J^T J + lambda diag(J^T J)) delta = -J^T r is solved from the best's sums with partial pivoting and
 *   the next candidate is best + delta; a singular or non-finite solve counts as one more rejection and the candidate equals the best.
 *   lambda starts at 1e-3 on every level; a level whose first candidate has no valid pixel does nothing, and neither does a level on which
 *   x2 has no contrast (largest pixel == smallest: such a view says nothing about geometry, and descent would only drag x1's window
 *   towards the parts of x1 nearest that constant; one launch after the pyramid marks those levels).  Between levels A_l = T^-1 A T,
 *   renormalised to a22 = 1, T = [[s,0,(s-1)/2],[0,s,(s-1)/2],[0,0,1]], s = 2^l.
 * `accepted` / `rejected` count the candidates after each level's first.  cost_before is level 0's cost of the INPUT matrix (one extra pass
 * when the walk starts above level 0).  h_out is inverse(A_best) scaled to [2][2] = 1 only if a candidate was accepted and level 0's final
 * cost is below cost_before; otherwise h_out is h, bit for bit, and cost_after = cost_before: never worse than the input by its own measure.
 * iters = 0 evaluates and reports, and returns h.  4 + sum over levels of (1 + 2 (iters + 1)) launches (+ 2 when levels > 1); nothing a
 * stream capture refuses.                                                                                                              */
int hesic_homography_refine(const float* x1, const int64_t* s1, const float* x2, const int64_t* s2, int B, int C, int H, int W,
                            const float* h, int levels, int iters, double huber, double min_overlap, void* ws, int64_t ws_bytes,
                            float* h_out, double* info, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* HESIC_HOMOGRAPHY_REFINE_H */

/* hesic_train_ctl.h -- device-resident step controls of the training step: the global L2 norm of a flat gradient buffer, gradient clipping,
 * the non-finite guard and a learning rate read from device memory, so that a step recorded into a HIP graph still obeys decisions a host
 * would otherwise make between two launches.  Exported by both libraries (libhesic_hip.so, libhesic_hip_f16.so); an addition to
 * HESIC_ABI_VERSION 2.  Includes hesic_hip.h for hesic_adam_chunk; hesic_hip.h does not include this header.                            */
#ifndef HESIC_TRAIN_CTL_H
#define HESIC_TRAIN_CTL_H
#include <stdint.h>
#include "hesic_hip.h"
#ifdef __cplusplus
extern "C" {
#endif

/* The control block: HESIC_TRAIN_CTL_FLOATS fp32 values in device memory, one block per optimiser group.
 * Inputs, written by the host (a device fill) outside any graph:                                                                        */
#define HESIC_TRAIN_CTL_LR 0             /* the learning rate hesic_adam_step_ctl uses                                                   */
#define HESIC_TRAIN_CTL_MAX_NORM 1       /* clip the gradient to this global L2 norm; <= 0: do not clip                                  */
#define HESIC_TRAIN_CTL_SKIP_NONFINITE 2 /* 0 / 1: a non-finite norm turns the step into a no-op                                         */
/* Outputs, written by the second launch of hesic_grad_norm_ctl:                                                                         */
#define HESIC_TRAIN_CTL_GRAD_NORM 3      /* the L2 norm of the buffer (the fp64 sum of squares, one square root, rounded once to fp32)   */
#define HESIC_TRAIN_CTL_CLIP_COEF 4      /* min(1, max_norm / (grad_norm + 1e-6)) in fp32 (torch.nn.utils.clip_grad_norm_); 1 without clipping */
#define HESIC_TRAIN_CTL_APPLIED 5        /* 1: hesic_adam_step_ctl updates; 0: it changes nothing                                        */
#define HESIC_TRAIN_CTL_SKIPPED 6        /* running count of calls that ended with applied == 0 (the host zeroes it once)                */
#define HESIC_TRAIN_CTL_FLOATS 8         /* size of the block (entry 7 is reserved, zero)                                                */

/* `partials` of hesic_grad_norm_ctl holds this many fp64 values (one per block of the first launch)                                     */
#define HESIC_GRAD_NORM_MAX_BLOCKS 1024

/* The L2 norm of the `numel` fp32 values at `g` (any 4-byte aligned address) and the step decision, in two launches, no host read:
 *   1. min(HESIC_GRAD_NORM_MAX_BLOCKS, ceil(numel / 4096)) blocks square and sum in fp64 from the first product (a finite fp32 buffer can
 *      never give a non-finite sum) and leave one fp64 partial each in `partials` (every entry that is read is written first);
 *   2. one block adds the partials in a fixed order and writes grad_norm, clip_coef, applied = !(skip_nonfinite && the sum is not finite)
 *      -- ANDed with the `applied` of `also_require`, another group's control block that this entry point ran on earlier in the stream
 *      (may be null) -- and skipped += 1 - applied.
 * No atomics, no completion counter: the same buffer gives the same bits in every run, eagerly and in a graph replay, on every rank.     */
int hesic_grad_norm_ctl(const float* g, int64_t numel, double* partials, float* ctl, const float* also_require, void* stream);

/* hesic_adam_step with the decisions of `ctl` (filled by hesic_grad_norm_ctl earlier in the stream): the learning rate is ctl[LR]
 * (chunk->lr is ignored), every gradient value enters as the fp32 product g * ctl[CLIP_COEF] rounded once (the gradient buffers are not
 * written), and with ctl[APPLIED] == 0 nothing changes: neither p, m, v nor the step counters.  With clip_coef == 1 and the same learning
 * rate the results equal hesic_adam_step's bit for bit.                                                                                 */
int hesic_adam_step_ctl(const hesic_adam_chunk* chunk_host, const float* ctl, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* HESIC_TRAIN_CTL_H */

/* hesic_dropout_state.h -- the dropout masks of hesic_homography_net.h (hesic_flatten_dropout_*) with (seed, step) in DEVICE memory, so that a
 * captured HIP graph draws a new mask at every replay (train.GraphedHomographyTrainer).  Exported by both libraries (libhesic_hip.so,
 * libhesic_hip_f16.so); an addition to HESIC_ABI_VERSION 2.  The kernels are those of hesic_homography_net.h (homography_net.hip): one
 * body per kernel, parametrised on where the key words and the step come from.                                                          */
#ifndef HESIC_DROPOUT_STATE_H
#define HESIC_DROPOUT_STATE_H
#include <stddef.h>
#include <stdint.h>
#include "hesic_hip.h"
#ifdef __cplusplus
extern "C" {
#endif

/* The state is sixteen bytes of device memory, uint32 {seed lo, seed hi, step, reserved}.  hesic_dropout_state_take (one tiny launch, one
 * lane, plain loads and stores, no atomics) copies the four words of `state` into `taken`, another 16-byte device buffer, and then sets
 * state.step = (step + 1) & 0xFFFFFFFF: "use the current step for both sites, then increment", what homography.Net does to its host counter.
 * The _state entries are hesic_flatten_dropout_forward / _backward with `seed, step` replaced by `taken` (read, never written; null is
 * refused), under the same argument checks; for equal (seed, step) they produce the by-value entries' bits.                            */
int hesic_dropout_state_take(void* state, void* taken, void* stream);
int hesic_flatten_dropout_forward_state(const void* x, void* y, int B, int HW, int C, uint32_t thr, float scale, const void* taken,
                                        uint32_t site, int dtype, void* stream);
int hesic_flatten_dropout_backward_state(const void* gy, void* gx, int B, int HW, int C, uint32_t thr, float scale, const void* taken,
                                         uint32_t site, int dtype, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* HESIC_DROPOUT_STATE_H */

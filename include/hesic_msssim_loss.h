/* hesic_msssim_loss.h -- MS-SSIM as a training loss: the backward of hesic_ssim_scale (include/hesic_hip.h, which includes this header).
 * Exported by both libraries (libhesic_hip.so, libhesic_hip_f16.so); an addition to HESIC_ABI_VERSION 2.                              */
#ifndef HESIC_MSSSIM_LOSS_H
#define HESIC_MSSSIM_LOSS_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

/* MS-SSIM as a training loss: the gradient of  L = sum_n grad_out[n] * MS[n]  with respect to x at ONE scale (y is the target, a constant).
 * A backward is n_scales launches walking from the last scale to the first: `x` / `y` are that scale's images (the originals on scale 0, the
 * hesic_avgpool2_pad outputs below; fp32, element strides (b, c, row, col) like hesic_ssim_scale), `sums` the forward's [n_scales][B*C][2]
 * fp64 sums, `counts[s]` the valid positions of scale s and `weights[s]` its exponent (host arrays of n_scales <= 5 entries), `grad_out` B
 * fp64 values on the device.  The gain of the scale -- grad_out[b] / C * w_s * MS_c / v_s / count_s, 0 where any scale's mean is <= 0 (the
 * relu of the definition) -- is formed on the device from `sums`: no host read.  `coarse_grad`: the gradient this entry point wrote for scale
 * + 1 (contiguous, the pooled size), null exactly on the last scale; a pixel receives 0.25 x its pool cell's gradient in the same launch.
 * `grad_x`: contiguous fp32 (B, C, H, W); a gather -- every element is written exactly once, no atomics, nothing to zero beforehand.      */
int hesic_ssim_scale_backward(const float* x, const int64_t x_strides[4], const float* y, const int64_t y_strides[4], int B, int C, int H,
                              int W, float data_range, const double* sums, const int64_t* counts, const double* weights, int n_scales,
                              int scale, const double* grad_out, const float* coarse_grad, float* grad_x, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* HESIC_MSSSIM_LOSS_H */

// The row arithmetic of the real bit-stream's cumulative-frequency tables, shared by the table kernels (entropy.hip) and the
// device range coder (codec.hip).  Encoder and decoder only meet if every one of them evaluates the SAME expressions: there is one
// definition, and it lives here.  Changing any of it moves the tables (models.TABLE_KERNEL_VERSION).
#pragma once
#include "common.h"

namespace {

__device__ __forceinline__ float phi_cdf(float x) { return 0.5f * erfcf(-0.70710678118654752440f * x); }

constexpr int GMM_MAXK = 8;
// alphabets up to this many symbols are handled one WAVE per row (the row lives in LDS)
constexpr int CDF_WAVE_MAX = 1024;

// numpy's float32 pairwise summation order (np.sum of a contiguous row)
__device__ float np_pairwise_sum(const float* a, int n) {
    if (n < 8) {
        float r = 0.f;
        for (int i = 0; i < n; ++i) r += a[i];
        return r;
    }
    if (n <= 128) {
        float r[8];
        for (int j = 0; j < 8; ++j) r[j] = a[j];
        int i = 8;
        for (; i < n - (n % 8); i += 8)
            for (int j = 0; j < 8; ++j) r[j] += a[i + j];
        float res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]));
        for (; i < n; ++i) res += a[i];
        return res;
    }
    int n2 = n / 2;
    n2 -= n2 % 8;
    return np_pairwise_sum(a, n2) + np_pairwise_sum(a + n2, n - n2);
}

// clipped pmf of symbol s under the row's mixture: ONE definition for every kernel that forms a table row (their tables must agree bit
// for bit: an encoder may take one and a decoder the other only if both evaluate the same expression)
template <int DUMMY = 0>
__device__ __forceinline__ float cdf_pm(int s, const float* mu, const float* sg, const float* wk, int K) {
    float pm = 0.f;
    for (int k = 0; k < K; ++k) {
        const float a = fabsf((float)s - mu[k]);
        pm += (phi_cdf((0.5f - a) / sg[k]) - phi_cdf((-0.5f - a) / sg[k])) * wk[k];
    }
    return fminf(fmaxf(pm, 1.0f / 65536.0f), 1.0f);
}

}  // namespace

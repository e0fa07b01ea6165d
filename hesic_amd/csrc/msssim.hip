// MS-SSIM on the device: the second quality metric the reference reports next to PSNR (ywz/mywork/test3real.py:107-109,
// newtrain6_real.py:90-91: pytorch_msssim.ms_ssim(x_hat, x, data_range=1, size_average=False)).  pytorch_msssim is third party and
// absent; the published algorithm (Wang, Simoncelli, Bovik 2003, as that package implements it) is restated in
// oracle/hesic_oracle.py::ms_ssim and here:
//   per scale, per image and channel: an 11-tap normalised Gaussian (sigma 1.5) applied separably WITHOUT padding to x, y, x^2, y^2, xy;
//   cs = (2 s_xy + C2) / (s_x^2 + s_y^2 + C2), ssim = (2 mu_x mu_y + C1) / (mu_x^2 + mu_y^2 + C1) * cs, summed over the valid positions;
//   between scales a 2 x 2 average pool (zero padding of odd sides, divisor 4).
// HBM-bound by construction (two fp32 images read once per scale: 12.6 MB at 512 x 512 x 3 x 2 views x 8 pairs); a block owns a 32 x 32
// tile of valid positions: the 42 x 42 input patches of x and y go to LDS once, the horizontal pass leaves five 42 x 32 maps in LDS, the
// vertical pass + the two ratios run per output pixel, the block's partial sums leave through ONE pair of fp64 atomics.
#include "common.h"

namespace {

constexpr int WIN = 11, HALO = WIN - 1, TS = 32, PS = TS + HALO;      // tile of valid outputs, patch side

struct SsimArgs {
    const float* x; const float* y;
    int64_t xs[4], ys[4];          // element strides (b, c, row, col) of the two images
    int B, C, H, W, Ho, Wo, tiles_x, tiles_y;
    float win[WIN];
    float C1, C2;
    double* sums;                  // [B * C][2]: sum of ssim, sum of cs over the valid positions
};

__global__ __launch_bounds__(256) void ssim_scale_kernel(const SsimArgs a) {
    __shared__ float px[PS][PS + 1], py[PS][PS + 1];
    __shared__ float hq[5][PS][TS + 1];
    __shared__ double red[4][2];
    const int tid = threadIdx.x;
    int t = blockIdx.x;
    const int tx = t % a.tiles_x; t /= a.tiles_x;
    const int ty = t % a.tiles_y; t /= a.tiles_y;
    const int c = t % a.C, b = t / a.C;
    const int oy0 = ty * TS, ox0 = tx * TS;
    const float* xb = a.x + b * a.xs[0] + c * a.xs[1];
    const float* yb = a.y + b * a.ys[0] + c * a.ys[1];
    for (int i = tid; i < PS * PS; i += 256) {
        const int r = i / PS, q = i % PS, iy = oy0 + r, ix = ox0 + q;
        const bool ok = iy < a.H && ix < a.W;
        px[r][q] = ok ? xb[iy * a.xs[2] + ix * a.xs[3]] : 0.f;
        py[r][q] = ok ? yb[iy * a.ys[2] + ix * a.ys[3]] : 0.f;
    }
    __syncthreads();
    for (int i = tid; i < PS * TS; i += 256) {            // horizontal pass: rows of the patch x the tile's 32 columns
        const int r = i / TS, q = i % TS;
        float sx = 0.f, sy = 0.f, sxx = 0.f, syy = 0.f, sxy = 0.f;
#pragma unroll
        for (int k = 0; k < WIN; ++k) {
            const float w = a.win[k], u = px[r][q + k], v = py[r][q + k];
            sx += w * u; sy += w * v; sxx += w * (u * u); syy += w * (v * v); sxy += w * (u * v);
        }
        hq[0][r][q] = sx; hq[1][r][q] = sy; hq[2][r][q] = sxx; hq[3][r][q] = syy; hq[4][r][q] = sxy;
    }
    __syncthreads();
    double acc_s = 0.0, acc_c = 0.0;
    for (int i = tid; i < TS * TS; i += 256) {
        const int r = i / TS, q = i % TS;
        if (oy0 + r >= a.Ho || ox0 + q >= a.Wo) continue;
        float m[5] = {0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int k = 0; k < WIN; ++k) {
            const float w = a.win[k];
#pragma unroll
            for (int j = 0; j < 5; ++j) m[j] += w * hq[j][r + k][q];
        }
        const float mxx = m[0] * m[0], myy = m[1] * m[1], mxy = m[0] * m[1];
        const float vx = m[2] - mxx, vy = m[3] - myy, cxy = m[4] - mxy;
        const float cs = (2.f * cxy + a.C2) / (vx + vy + a.C2);
        const float ss = (2.f * mxy + a.C1) / (mxx + myy + a.C1) * cs;
        acc_s += (double)ss; acc_c += (double)cs;
    }
    acc_s = wave_sum_d(acc_s); acc_c = wave_sum_d(acc_c);
    if ((tid & 63) == 0) { red[tid >> 6][0] = acc_s; red[tid >> 6][1] = acc_c; }
    __syncthreads();
    if (tid == 0) {
        atomicAdd(a.sums + (int64_t)(b * a.C + c) * 2, red[0][0] + red[1][0] + red[2][0] + red[3][0]);
        atomicAdd(a.sums + (int64_t)(b * a.C + c) * 2 + 1, red[0][1] + red[1][1] + red[2][1] + red[3][1]);
    }
}

// F.avg_pool2d(x, 2, padding = (H % 2, W % 2)) of pytorch_msssim: zero padding on both sides of an odd side, divisor always 4;
// output (H + 2 ph - 2) / 2 + 1.  Planar fp32 out (contiguous); one thread per output value.
__global__ void avgpool2_kernel(const float* __restrict__ x, int64_t sb, int64_t sc, int64_t sy, int64_t sx, float* __restrict__ y,
                                int B, int C, int H, int W, int Ho, int Wo, int ph, int pw) {
    const int64_t n = (int64_t)B * C * Ho * Wo;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const int ox = i % Wo;
        int64_t r = i / Wo;
        const int oy = r % Ho; r /= Ho;
        const int c = r % C, b = r / C;
        const float* p = x + b * sb + c * sc;
        float s = 0.f;
#pragma unroll
        for (int dy = 0; dy < 2; ++dy)
#pragma unroll
            for (int dx = 0; dx < 2; ++dx) {
                const int iy = 2 * oy + dy - ph, ix = 2 * ox + dx - pw;
                if (iy >= 0 && iy < H && ix >= 0 && ix < W) s += p[iy * sy + ix * sx];
            }
        y[i] = 0.25f * s;
    }
}

// ------------------------------------------------------------------------------------------------ backward (MS-SSIM as a training loss)
// d(sum_n grad_out[n] MS[n]) / dx of ONE scale, as a gather: a block owns a 32 x 32 tile of GRADIENT pixels q.  A pixel sees the valid
// positions p in [q - 10, q], so the block needs the three coefficient maps
//     a_xy = gain * dv/dExy, a_xx = gain * dv/dExx, a_mu = gain * dv/dmu_x       (v = cs on scales 1-4, ssim on scale 5; 0 outside the valid region)
// on the 42 x 42 positions from q0 - 10 on, and those need the 52 x 52 input patch from q0 - 10 on.  The window means are RECOMPUTED in LDS
// with the forward's arithmetic (same taps, same order of summation) instead of being stored by the forward: a
// launch then reads x and y once (+ halo) and the pooled gradient, and writes the gradient -- 4 + 4 + 1 + 4 bytes per pixel -- where stored
// maps would add 12 bytes per pixel to the forward and 12 to the backward.
//     dL/dx(q) = (G^T a_mu)(q) + 2 x(q) (G^T a_xx)(q) + y(q) (G^T a_xy)(q) + 0.25 * gc[pool cell of q]
// LDS (65,316 B of the 64 KiB a block may declare statically, two blocks per CU of 160 KiB): the two 52 x 52 patches, reused for the three
// 42 x 42 coefficient maps once every thread holds the x(q), y(q) of its four pixels; the five 52 x 42 row-filtered maps, reused for the three
// 42 x 32 row-filtered coefficient maps.  Every gradient element is written exactly once: no atomics, no zero-fill.
constexpr int BT = 32, BA = BT + HALO, BP = BA + HALO;      // gradient tile, coefficient-map side, input patch side

struct SsimBwdArgs {
    const float* x; const float* y;      // x: the differentiated image, y: the target (this scale's images)
    int64_t xs[4], ys[4];
    const float* gc;                     // gradient of the next coarser scale (contiguous, Hc x Wc) or null on the last scale
    float* gx;                           // out: contiguous (B, C, H, W)
    const double* sums;                  // [n_scales][B * C][2] of the forward (ssim, cs)
    const double* grad_out;              // [B]
    double inv_count[5], weight[5];
    int scale, n_scales;
    int B, C, H, W, Ho, Wo, Hc, Wc, tiles_x, tiles_y;
    float win[WIN];
    float C1, C2;
};

__global__ __launch_bounds__(256) void ssim_scale_backward_kernel(const SsimBwdArgs a) {
    __shared__ float patch[2 * BP * BP];          // px | py, later the coefficient maps A[3][BA][BA]
    __shared__ float rows[5 * BP * BA];           // hq[5][BP][BA], later T[3][BA][BT]
    __shared__ float gain_s;
    float (*px)[BP] = reinterpret_cast<float (*)[BP]>(patch);
    float (*py)[BP] = reinterpret_cast<float (*)[BP]>(patch + BP * BP);
    float (*A)[BA][BA] = reinterpret_cast<float (*)[BA][BA]>(patch);
    float (*hq)[BP][BA] = reinterpret_cast<float (*)[BP][BA]>(rows);
    float (*T)[BA][BT] = reinterpret_cast<float (*)[BA][BT]>(rows);
    static_assert(3 * BA * BA <= 2 * BP * BP && 3 * BA * BT <= 5 * BP * BA, "aliased LDS regions");
    const int tid = threadIdx.x;
    int t = blockIdx.x;
    const int tx = t % a.tiles_x; t /= a.tiles_x;
    const int ty = t % a.tiles_y; t /= a.tiles_y;
    const int c = t % a.C, b = t / a.C;
    const int qy0 = ty * BT, qx0 = tx * BT;
    if (tid == 0) {
        // gain = grad_out[b] / C * w_s * MS_c / v_s / count_s, MS_c = prod_t v_t^w_t; any v_t <= 0 clamps the product and every gradient to 0
        double ms = 1.0, vs = 1.0;
        bool live = true;
        for (int s = 0; s < a.n_scales; ++s) {
            const double v = a.sums[((int64_t)s * a.B * a.C + b * a.C + c) * 2 + (s == a.n_scales - 1 ? 0 : 1)] * a.inv_count[s];
            if (!(v > 0.0)) { live = false; break; }
            ms *= pow(v, a.weight[s]);
            if (s == a.scale) vs = v;
        }
        gain_s = live ? (float)(a.grad_out[b] / a.C * a.weight[a.scale] * ms / vs * a.inv_count[a.scale]) : 0.f;
    }
    const float* xb = a.x + b * a.xs[0] + c * a.xs[1];
    const float* yb = a.y + b * a.ys[0] + c * a.ys[1];
    for (int i = tid; i < BP * BP; i += 256) {
        const int r = i / BP, q = i % BP, iy = qy0 - HALO + r, ix = qx0 - HALO + q;
        const bool ok = iy >= 0 && iy < a.H && ix >= 0 && ix < a.W;
        px[r][q] = ok ? xb[iy * a.xs[2] + ix * a.xs[3]] : 0.f;
        py[r][q] = ok ? yb[iy * a.ys[2] + ix * a.ys[3]] : 0.f;
    }
    __syncthreads();
    float xq[4], yq[4];                                   // this thread's four gradient pixels: tile position (tid / 32 + 8 j, tid % 32)
#pragma unroll
    for (int j = 0; j < 4; ++j) { xq[j] = px[HALO + (tid >> 5) + 8 * j][HALO + (tid & 31)]; yq[j] = py[HALO + (tid >> 5) + 8 * j][HALO + (tid & 31)]; }
    for (int i = tid; i < BP * BA; i += 256) {            // horizontal pass: rows of the patch x the 42 columns of positions
        const int r = i / BA, q = i % BA;
        float sx = 0.f, sy = 0.f, sxx = 0.f, syy = 0.f, sxy = 0.f;
#pragma unroll
        for (int k = 0; k < WIN; ++k) {
            const float w = a.win[k], u = px[r][q + k], v = py[r][q + k];
            sx += w * u; sy += w * v; sxx += w * (u * u); syy += w * (v * v); sxy += w * (u * v);
        }
        hq[0][r][q] = sx; hq[1][r][q] = sy; hq[2][r][q] = sxx; hq[3][r][q] = syy; hq[4][r][q] = sxy;
    }
    __syncthreads();                                      // the patches are dead from here on (xq / yq are in registers)
    const float gain = gain_s;
    const bool last = a.scale == a.n_scales - 1;
    for (int i = tid; i < BA * BA; i += 256) {            // vertical pass + coefficients at position p = q0 - 10 + (r, q)
        const int r = i / BA, q = i % BA, py_ = qy0 - HALO + r, px_ = qx0 - HALO + q;
        float a_mu = 0.f, a_xx = 0.f, a_xy = 0.f;
        if (py_ >= 0 && py_ < a.Ho && px_ >= 0 && px_ < a.Wo) {
            float m[5] = {0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int k = 0; k < WIN; ++k) {
                const float w = a.win[k];
#pragma unroll
                for (int j = 0; j < 5; ++j) m[j] += w * hq[j][r + k][q];
            }
            const float mxx = m[0] * m[0], myy = m[1] * m[1], mxy = m[0] * m[1];
            const float vx = m[2] - mxx, vy = m[3] - myy, cxy = m[4] - mxy;
            const float iD2 = 1.f / (vx + vy + a.C2);
            const float cs = (2.f * cxy + a.C2) * iD2;
            a_xy = 2.f * iD2; a_xx = -cs * iD2; a_mu = 2.f * iD2 * (cs * m[0] - m[1]);
            if (last) {
                const float iD1 = 1.f / (mxx + myy + a.C1), l = (2.f * mxy + a.C1) * iD1;
                a_xy *= l; a_xx *= l; a_mu = a_mu * l + cs * (2.f * m[1] - 2.f * m[0] * l) * iD1;
            }
            a_xy *= gain; a_xx *= gain; a_mu *= gain;
        }
        A[0][r][q] = a_mu; A[1][r][q] = a_xx; A[2][r][q] = a_xy;
    }
    __syncthreads();                                      // hq is dead
    for (int i = tid; i < BA * BT; i += 256) {            // transposed window along the row: T(r, qc) = sum_k w[k] A(r, qc + 10 - k)
        const int r = i / BT, q = i % BT;
        float s0 = 0.f, s1 = 0.f, s2 = 0.f;
#pragma unroll
        for (int k = 0; k < WIN; ++k) {
            const float w = a.win[k];
            s0 += w * A[0][r][q + HALO - k]; s1 += w * A[1][r][q + HALO - k]; s2 += w * A[2][r][q + HALO - k];
        }
        T[0][r][q] = s0; T[1][r][q] = s1; T[2][r][q] = s2;
    }
    __syncthreads();
    const int ph = a.H % 2, pw = a.W % 2;
    float* gb = a.gx + ((int64_t)b * a.C + c) * a.H * a.W;
    const float* gcb = a.gc ? a.gc + ((int64_t)b * a.C + c) * a.Hc * a.Wc : nullptr;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int r = (tid >> 5) + 8 * j, q = tid & 31, iy = qy0 + r, ix = qx0 + q;
        if (iy >= a.H || ix >= a.W) continue;
        float s0 = 0.f, s1 = 0.f, s2 = 0.f;
#pragma unroll
        for (int k = 0; k < WIN; ++k) {
            const float w = a.win[k];
            s0 += w * T[0][r + HALO - k][q]; s1 += w * T[1][r + HALO - k][q]; s2 += w * T[2][r + HALO - k][q];
        }
        float g = s0 + 2.f * xq[j] * s1 + yq[j] * s2;
        if (gcb) g += 0.25f * gcb[(int64_t)((iy + ph) >> 1) * a.Wc + ((ix + pw) >> 1)];
        gb[(int64_t)iy * a.W + ix] = g;
    }
}

}  // namespace

extern "C" int hesic_ssim_scale(const float* x, const int64_t x_strides[4], const float* y, const int64_t y_strides[4], int B, int C, int H,
                                int W, float data_range, double* sums, void* stream) {
    HESIC_CHECK_ARG(x && y && x_strides && y_strides && sums && B > 0 && C > 0, "ssim_scale: bad arguments");
    HESIC_CHECK_ARG(H >= WIN && W >= WIN, "ssim_scale: image side %d x %d smaller than the %d-tap window", H, W, WIN);
    SsimArgs a;
    a.x = x; a.y = y;
    for (int i = 0; i < 4; ++i) { a.xs[i] = x_strides[i]; a.ys[i] = y_strides[i]; }
    a.B = B; a.C = C; a.H = H; a.W = W; a.Ho = H - HALO; a.Wo = W - HALO;
    a.tiles_x = (a.Wo + TS - 1) / TS; a.tiles_y = (a.Ho + TS - 1) / TS;
    float g[WIN], sum = 0.f;                                       // pytorch_msssim._fspecial_gauss_1d in fp32
    for (int i = 0; i < WIN; ++i) { const float co = (float)(i - WIN / 2); g[i] = expf(-(co * co) / (2.f * 1.5f * 1.5f)); sum += g[i]; }
    for (int i = 0; i < WIN; ++i) a.win[i] = g[i] / sum;
    a.C1 = (0.01f * data_range) * (0.01f * data_range); a.C2 = (0.03f * data_range) * (0.03f * data_range);
    a.sums = sums;
    const int64_t blocks = (int64_t)B * C * a.tiles_x * a.tiles_y;
    HESIC_CHECK_ARG(blocks < (1ll << 31), "ssim_scale: bad grid");
    hipLaunchKernelGGL(ssim_scale_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, a);
    HESIC_LAUNCH_RETURN("ssim_scale");
}

extern "C" int hesic_avgpool2_pad(const float* x, const int64_t x_strides[4], float* y, int B, int C, int H, int W, void* stream) {
    HESIC_CHECK_ARG(x && x_strides && y && B > 0 && C > 0 && H > 1 && W > 1, "avgpool2_pad: bad arguments");
    const int ph = H % 2, pw = W % 2, Ho = (H + 2 * ph - 2) / 2 + 1, Wo = (W + 2 * pw - 2) / 2 + 1;
    hipLaunchKernelGGL(avgpool2_kernel, dim3(grid_for((int64_t)B * C * Ho * Wo, 256)), dim3(256), 0, (hipStream_t)stream, x, x_strides[0],
                       x_strides[1], x_strides[2], x_strides[3], y, B, C, H, W, Ho, Wo, ph, pw);
    HESIC_LAUNCH_RETURN("avgpool2_pad");
}

extern "C" int hesic_ssim_scale_backward(const float* x, const int64_t x_strides[4], const float* y, const int64_t y_strides[4], int B, int C,
                                         int H, int W, float data_range, const double* sums, const int64_t* counts, const double* weights,
                                         int n_scales, int scale, const double* grad_out, const float* coarse_grad, float* grad_x,
                                         void* stream) {
    HESIC_CHECK_ARG(x && y && x_strides && y_strides && sums && counts && weights && grad_out && grad_x && B > 0 && C > 0,
                    "ssim_scale_backward: bad arguments");
    HESIC_CHECK_ARG(H >= WIN && W >= WIN, "ssim_scale_backward: image side %d x %d smaller than the %d-tap window", H, W, WIN);
    HESIC_CHECK_ARG(n_scales >= 1 && n_scales <= 5 && scale >= 0 && scale < n_scales, "ssim_scale_backward: scale %d of %d (at most 5)", scale,
                    n_scales);
    HESIC_CHECK_ARG((coarse_grad != nullptr) == (scale < n_scales - 1), "ssim_scale_backward: every scale but the last takes the coarser gradient");
    HESIC_CHECK_ARG(counts[scale] == (int64_t)(H - HALO) * (W - HALO), "ssim_scale_backward: counts[%d] is not (H - 10) * (W - 10)", scale);
    SsimBwdArgs a;
    a.x = x; a.y = y; a.gc = coarse_grad; a.gx = grad_x; a.sums = sums; a.grad_out = grad_out;
    for (int i = 0; i < 4; ++i) { a.xs[i] = x_strides[i]; a.ys[i] = y_strides[i]; }
    for (int i = 0; i < 5; ++i) {
        HESIC_CHECK_ARG(i >= n_scales || counts[i] > 0, "ssim_scale_backward: counts[%d] <= 0", i);
        a.inv_count[i] = i < n_scales ? 1.0 / (double)counts[i] : 0.0;
        a.weight[i] = i < n_scales ? weights[i] : 0.0;
    }
    a.scale = scale; a.n_scales = n_scales;
    a.B = B; a.C = C; a.H = H; a.W = W; a.Ho = H - HALO; a.Wo = W - HALO;
    a.Hc = (H + 2 * (H % 2) - 2) / 2 + 1; a.Wc = (W + 2 * (W % 2) - 2) / 2 + 1;      // hesic_avgpool2_pad's output size
    a.tiles_x = (W + BT - 1) / BT; a.tiles_y = (H + BT - 1) / BT;
    float g[WIN], sum = 0.f;                                       // the forward's window
    for (int i = 0; i < WIN; ++i) { const float co = (float)(i - WIN / 2); g[i] = expf(-(co * co) / (2.f * 1.5f * 1.5f)); sum += g[i]; }
    for (int i = 0; i < WIN; ++i) a.win[i] = g[i] / sum;
    a.C1 = (0.01f * data_range) * (0.01f * data_range); a.C2 = (0.03f * data_range) * (0.03f * data_range);
    const int64_t blocks = (int64_t)B * C * a.tiles_x * a.tiles_y;
    HESIC_CHECK_ARG(blocks < (1ll << 31), "ssim_scale_backward: bad grid");
    hipLaunchKernelGGL(ssim_scale_backward_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, a);
    HESIC_LAUNCH_RETURN("ssim_scale_backward");
}

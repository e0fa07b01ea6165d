// Gradients through the geometry in front of the stereo path (include/hesic_homography_train.h): the photometric loss that trains
// HomographyNet (ywz/mywork/model.py:18-45; the training program is udh/udh/QHtrain.py:88-132) with its backward to the corner deltas, the
// gradient of warp_perspective with respect to its matrix, and the adjoint of the 4-point DLT.
//
// One per-pixel kernel serves the three image-sized passes.  A thread maps its destination pixel p = (ox, oy, 1) through the destination ->
// source matrix A (fp64: X, Y, Z = A p), samples the four taps with warp.hip's zero padding (cell and weights from the fp64 coordinate), and
//   PHOTO_FWD: adds |patch_b_hat - patch_b| over the channels;
//   PHOTO_BWD: g_c = sign(patch_b_hat - patch_b);  WARP_BWD: g_c = d_dst_c;  then
//       dI/dsx = wy0 (I01 - I00) + wy1 (I11 - I10),  dI/dsy = wx0 (I10 - I00) + wx1 (I11 - I01)     (out-of-image taps are 0)
//       dsx/dA0j = k pj / Z,  dsx/dA2j = -k x pj / Z  with x = X / Z and k = W / (W - 1) under align_corners = 0 (1 otherwise); y alike.
// A block leaves one fp64 partial per matrix entry in the workspace; a finishing launch adds the partials in a fixed order (one thread per
// pair) and applies what follows the matrix: the mean, the upstream gradient and the DLT adjoint, or -M^-T dA M^-T.  No atomics.
#include "common.h"
#include "dlt.h"
#include "../../include/hesic_homography_train.h"

namespace {

constexpr int NV = HESIC_HTRAIN_PARTIAL_WIDTH;
enum { PHOTO_FWD = 0, PHOTO_BWD = 1, WARP_BWD = 2 };

struct GArgs {
    hesic_warp_desc d;
    const void* src;         // the sampled image
    const void* other;       // PHOTO_*: patch_b (fp32); WARP_BWD: d_dst
    const float* M;          // WARP_BWD: the caller's matrix
    const double* h;         // PHOTO_*: the DLT's h (B,9), destination -> source
    double* partials;        // [B][gridDim.x][NV] (PHOTO_FWD: [B][gridDim.x])
};

template <int MODE>
__global__ __launch_bounds__(256) void coord_kernel(const GArgs a) {
    const hesic_warp_desc& d = a.d;
    __shared__ double iv[9];
    __shared__ double red[4][NV];
    const int b = blockIdx.y;
    if (threadIdx.x == 0) {
        if (MODE == WARP_BWD) {
            double m[9];
            for (int j = 0; j < 9; ++j) m[j] = a.M[b * 9 + j];
            if (d.m_is_dst_to_src)
                for (int j = 0; j < 9; ++j) iv[j] = m[j];
            else
                inv3(m, iv);
        } else {
            for (int j = 0; j < 9; ++j) iv[j] = a.h[b * 9 + j];
        }
    }
    __syncthreads();
    const double kx = d.align_corners ? 1.0 : d.W / (double)(d.W - 1), ky = d.align_corners ? 1.0 : d.H / (double)(d.H - 1);
    constexpr int NA = MODE == PHOTO_FWD ? 1 : NV;
    double acc[NA];
#pragma unroll
    for (int k = 0; k < NA; ++k) acc[k] = 0.0;
    const int64_t total = (int64_t)d.Ho * d.Wo;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int ox = i % d.Wo, oy = i / d.Wo;
        const double X = iv[0] * ox + iv[1] * oy + iv[2], Y = iv[3] * ox + iv[4] * oy + iv[5], Z = iv[6] * ox + iv[7] * oy + iv[8];
        const double rz = 1.0 / Z;
        const double x = X * rz, y = Y * rz;
        // the cell and the weights come from the fp64 coordinate: bilinear interpolation has a kink at every integer coordinate, and a
        // coordinate rounded to fp32 first (warp.hip's forward, where the value is continuous) can land in the neighbouring cell, whose
        // slope is another -- one such pixel in 128 x 128 moves the gradient by several 1e-5 of its size
        const double sxd = d.align_corners ? x : x * kx - 0.5, syd = d.align_corners ? y : y * ky - 0.5;
        const double fxd = floor(sxd), fyd = floor(syd);
        const float fx0 = (float)fxd, fy0 = (float)fyd;
        const float wx1 = (float)(sxd - fxd), wy1 = (float)(syd - fyd), wx0 = 1.f - wx1, wy0 = 1.f - wy1;
        const bool big = !(isfinite(fx0) && isfinite(fy0)) || fabsf(fx0) > 1e8f || fabsf(fy0) > 1e8f;
        const int x0 = big ? -10 : (int)fx0, y0 = big ? -10 : (int)fy0;
        const bool vx0 = x0 >= 0 && x0 < d.W, vx1 = x0 + 1 >= 0 && x0 + 1 < d.W;
        const bool vy0 = y0 >= 0 && y0 < d.H, vy1 = y0 + 1 >= 0 && y0 + 1 < d.H;
        const int64_t sb = b * d.ss_b + y0 * d.ss_y + x0 * d.ss_x;
        const int64_t db = b * d.ds_b + oy * d.ds_y + ox * d.ds_x;
        float gix = 0.f, giy = 0.f;
        for (int c = 0; c < d.C; ++c) {
            const int64_t s = sb + c * d.ss_c;
            const float i00 = vy0 && vx0 ? ld_any(a.src, s, d.src_dtype) : 0.f;
            const float i01 = vy0 && vx1 ? ld_any(a.src, s + d.ss_x, d.src_dtype) : 0.f;
            const float i10 = vy1 && vx0 ? ld_any(a.src, s + d.ss_y, d.src_dtype) : 0.f;
            const float i11 = vy1 && vx1 ? ld_any(a.src, s + d.ss_y + d.ss_x, d.src_dtype) : 0.f;
            float g;
            if constexpr (MODE == WARP_BWD) {
                g = ld_any(a.other, db + c * d.ds_c, d.dst_dtype);
            } else {
                float v = 0.f;                               // the forward warp's sum: invalid taps contribute no term
                if (vy0 && vx0) v += i00 * (wx0 * wy0);
                if (vy0 && vx1) v += i01 * (wx1 * wy0);
                if (vy1 && vx0) v += i10 * (wx0 * wy1);
                if (vy1 && vx1) v += i11 * (wx1 * wy1);
                const float diff = v - ((const float*)a.other)[db + c * d.ds_c];
                g = (float)(diff > 0.f) - (float)(diff < 0.f);
                if constexpr (MODE == PHOTO_FWD) acc[0] += (double)fabsf(diff);
            }
            if constexpr (MODE != PHOTO_FWD) {
                gix += g * (wy0 * (i01 - i00) + wy1 * (i11 - i10));
                giy += g * (wx0 * (i10 - i00) + wx1 * (i11 - i01));
            }
        }
        if constexpr (MODE != PHOTO_FWD) {
            if (!big) {
                const double gx = (double)gix * kx, gy = (double)giy * ky;
                const double t0 = gx * rz, t1 = gy * rz, t2 = -(gx * x + gy * y) * rz;
                acc[0] += t0 * ox; acc[1] += t0 * oy; acc[2] += t0;
                acc[3] += t1 * ox; acc[4] += t1 * oy; acc[5] += t1;
                acc[6] += t2 * ox; acc[7] += t2 * oy; acc[8] += t2;
            }
        }
    }
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
#pragma unroll
    for (int k = 0; k < NA; ++k) {
        const double s = wave_sum_d(acc[k]);
        if (lane == 0) red[wave][k] = s;
    }
    __syncthreads();
    if (threadIdx.x < NA)
        a.partials[((int64_t)b * gridDim.x + blockIdx.x) * NA + threadIdx.x] =
            ((red[0][threadIdx.x] + red[1][threadIdx.x]) + red[2][threadIdx.x]) + red[3][threadIdx.x];
}

// Gaussian elimination with partial pivoting on an augmented 8x9 system (the DLT's own elimination, for the adjoint's transposed system)
__device__ bool solve8(double A[8][9], double x[8]) {
    for (int c = 0; c < 8; ++c) {
        int piv = c;
        for (int r = c + 1; r < 8; ++r)
            if (fabs(A[r][c]) > fabs(A[piv][c])) piv = r;
        if (fabs(A[piv][c]) < 1e-300) return false;
        if (piv != c)
            for (int k = 0; k < 9; ++k) { const double t = A[c][k]; A[c][k] = A[piv][k]; A[piv][k] = t; }
        const double inv = 1.0 / A[c][c];
        for (int r = c + 1; r < 8; ++r) {
            const double f = A[r][c] * inv;
            for (int k = c; k < 9; ++k) A[r][k] -= f * A[c][k];
        }
    }
    for (int c = 7; c >= 0; --c) {
        double s = A[c][8];
        for (int k = c + 1; k < 8; ++k) s -= A[c][k] * x[k];
        x[c] = s / A[c][c];
    }
    return true;
}

// The DLT solves A h = rhs (rows [x y 1 0 0 0 -xu -yu | u], [0 0 0 x y 1 -xv -yv | v]).  With the gradient g of h[0..7]:
//   lambda = A^-T g,  d rhs = lambda,  dA = -lambda h^T,  and onto the points
//   du_i = lambda_2i (1 + h6 x + h7 y)                               dv_i = lambda_2i+1 (1 + h6 x + h7 y)
//   dx_i = -lambda_2i (h0 - h6 u) - lambda_2i+1 (h3 - h6 v)           dy_i = -lambda_2i (h1 - h7 u) - lambda_2i+1 (h4 - h7 v)
__device__ bool dlt4_adjoint(const double sx[4], const double sy[4], const double dx[4], const double dy[4], const double h[9],
                             const double g[8], double gsx[4], double gsy[4], double gdx[4], double gdy[4]) {
    double T[8][9], lam[8];
    for (int i = 0; i < 4; ++i) {
        const double x = sx[i], y = sy[i], u = dx[i], v = dy[i];
        const double r0[8] = {x, y, 1, 0, 0, 0, -x * u, -y * u}, r1[8] = {0, 0, 0, x, y, 1, -x * v, -y * v};
        for (int k = 0; k < 8; ++k) { T[k][2 * i] = r0[k]; T[k][2 * i + 1] = r1[k]; }      // transposed
    }
    for (int k = 0; k < 8; ++k) T[k][8] = g[k];
    if (!solve8(T, lam)) return false;
    for (int i = 0; i < 4; ++i) {
        const double x = sx[i], y = sy[i], u = dx[i], v = dy[i], l0 = lam[2 * i], l1 = lam[2 * i + 1];
        const double w = 1.0 + h[6] * x + h[7] * y;
        gdx[i] = l0 * w; gdy[i] = l1 * w;
        gsx[i] = -l0 * (h[0] - h[6] * u) - l1 * (h[3] - h[6] * v);
        gsy[i] = -l0 * (h[1] - h[7] * u) - l1 * (h[4] - h[7] * v);
    }
    return true;
}

// -m^T g m^T: the gradient of a matrix from the gradient g of its inverse m
__device__ void inverse_adjoint(const double m[9], const double g[9], double o[9]) {
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) {
            double s = 0.0;
            for (int k = 0; k < 3; ++k)
                for (int l = 0; l < 3; ++l) s += m[3 * k + i] * g[3 * k + l] * m[3 * j + l];
            o[3 * i + j] = -s;
        }
}

// the photometric loss's point sets (fp64 from the fp32 inputs on): src = corners - corners[0], dst = corners + delta
__device__ void photo_points(const float* corners, const float* delta, int b, double sx[4], double sy[4], double dx[4], double dy[4]) {
    const double x0 = corners[b * 8], y0 = corners[b * 8 + 1];
    for (int i = 0; i < 4; ++i) {
        const double cx = corners[b * 8 + 2 * i], cy = corners[b * 8 + 2 * i + 1];
        sx[i] = cx - x0; sy[i] = cy - y0;
        dx[i] = cx + (double)delta[b * 8 + 2 * i]; dy[i] = cy + (double)delta[b * 8 + 2 * i + 1];
    }
}

__global__ void photo_dlt_kernel(const float* __restrict__ corners, const float* __restrict__ delta, double* __restrict__ h, int B) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    double sx[4], sy[4], dx[4], dy[4], hh[9];
    photo_points(corners, delta, b, sx, sy, dx, dy);
    if (!dlt4(sx, sy, dx, dy, hh))
        for (int k = 0; k < 9; ++k) hh[k] = NAN;
    for (int k = 0; k < 9; ++k) h[b * 9 + k] = hh[k];
}

// one block: the n partials in a fixed order (thread t takes t, t + 256, ...; then the wave and block sums), loss = sum / count
__global__ __launch_bounds__(256) void photo_loss_finish_kernel(const double* __restrict__ partials, int n, double count, float* __restrict__ loss) {
    __shared__ double red[4];
    double s = 0.0;
    for (int i = threadIdx.x; i < n; i += 256) s += partials[i];
    s = wave_sum_d(s);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) loss[0] = (float)((((red[0] + red[1]) + red[2]) + red[3]) / count);
}

__global__ void photo_bwd_finish_kernel(const double* __restrict__ partials, int nblk, double count, const float* __restrict__ grad_loss,
                                        const float* __restrict__ corners, const float* __restrict__ delta, const double* __restrict__ h,
                                        float* __restrict__ d_delta, int B) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    const double scale = (double)grad_loss[0] / count;
    double g[8], hh[9], sx[4], sy[4], dx[4], dy[4], gsx[4], gsy[4], gdx[4], gdy[4];
    for (int k = 0; k < 8; ++k) {
        double s = 0.0;
        for (int j = 0; j < nblk; ++j) s += partials[((int64_t)b * nblk + j) * NV + k];
        g[k] = s * scale;
    }
    for (int k = 0; k < 9; ++k) hh[k] = h[b * 9 + k];
    photo_points(corners, delta, b, sx, sy, dx, dy);
    const bool ok = dlt4_adjoint(sx, sy, dx, dy, hh, g, gsx, gsy, gdx, gdy);
    for (int i = 0; i < 4; ++i) {
        d_delta[b * 8 + 2 * i] = ok ? (float)gdx[i] : NAN;
        d_delta[b * 8 + 2 * i + 1] = ok ? (float)gdy[i] : NAN;
    }
}

__global__ void warp_m_finish_kernel(const double* __restrict__ partials, int nblk, const float* __restrict__ M, int m_is_dst_to_src,
                                     float* __restrict__ dM, int B) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    double g[9], o[9];
    for (int k = 0; k < 9; ++k) {
        double s = 0.0;
        for (int j = 0; j < nblk; ++j) s += partials[((int64_t)b * nblk + j) * NV + k];
        g[k] = s;
    }
    if (m_is_dst_to_src) {
        for (int k = 0; k < 9; ++k) o[k] = g[k];
    } else {
        double m[9], mi[9];
        for (int k = 0; k < 9; ++k) m[k] = M[b * 9 + k];
        inv3(m, mi);
        inverse_adjoint(mi, g, o);
    }
    for (int k = 0; k < 9; ++k) dM[b * 9 + k] = (float)o[k];
}

__global__ void perspective_transform_bwd_kernel(const float* __restrict__ src, const float* __restrict__ dst, const float* __restrict__ dH,
                                                 float* __restrict__ d_src, float* __restrict__ d_dst, int B) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    double sx[4], sy[4], dx[4], dy[4], h[9], g[8], gsx[4], gsy[4], gdx[4], gdy[4];
    for (int i = 0; i < 4; ++i) {
        sx[i] = src[b * 8 + 2 * i]; sy[i] = src[b * 8 + 2 * i + 1];
        dx[i] = dst[b * 8 + 2 * i]; dy[i] = dst[b * 8 + 2 * i + 1];
    }
    for (int k = 0; k < 8; ++k) g[k] = dH[b * 9 + k];
    const bool ok = dlt4(sx, sy, dx, dy, h) && dlt4_adjoint(sx, sy, dx, dy, h, g, gsx, gsy, gdx, gdy);
    for (int i = 0; i < 4; ++i) {
        if (d_src) { d_src[b * 8 + 2 * i] = ok ? (float)gsx[i] : NAN; d_src[b * 8 + 2 * i + 1] = ok ? (float)gsy[i] : NAN; }
        if (d_dst) { d_dst[b * 8 + 2 * i] = ok ? (float)gdx[i] : NAN; d_dst[b * 8 + 2 * i + 1] = ok ? (float)gdy[i] : NAN; }
    }
}

__global__ void h_from_delta_bwd_kernel(const float* __restrict__ corners, const float* __restrict__ delta, float ra, float rb,
                                        int subtract_origin, const float* __restrict__ dH, float* __restrict__ d_delta, int B) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    double sx[4], sy[4], dx[4], dy[4], h[9], hi[9], ghi[9], gh[9], gsx[4], gsy[4], gdx[4], gdy[4];
    const float x0 = subtract_origin ? corners[b * 8] : 0.f, y0 = subtract_origin ? corners[b * 8 + 1] : 0.f;
    for (int i = 0; i < 4; ++i) {       // the forward's points (fp32 sums, hesic_h_from_delta)
        const float cx = corners[b * 8 + 2 * i] - x0, cy = corners[b * 8 + 2 * i + 1] - y0;
        sx[i] = cx; sy[i] = cy;
        dx[i] = cx + delta[b * 8 + 2 * i]; dy[i] = cy + delta[b * 8 + 2 * i + 1];
    }
    bool ok = dlt4(sx, sy, dx, dy, h);
    if (ok) {
        inv3(h, hi);
        // h_adjust scales entry (r, c) of the inverse by rs[r] * cs[c], rs = (a, b, 1), cs = (1/a, 1/b, 1)
        const double rs[3] = {ra, rb, 1.0}, cs[3] = {1.0 / ra, 1.0 / rb, 1.0};
        for (int r = 0; r < 3; ++r)
            for (int c = 0; c < 3; ++c) ghi[3 * r + c] = (double)dH[b * 9 + 3 * r + c] * rs[r] * cs[c];
        inverse_adjoint(hi, ghi, gh);
        ok = dlt4_adjoint(sx, sy, dx, dy, h, gh, gsx, gsy, gdx, gdy);
    }
    for (int i = 0; i < 4; ++i) {
        d_delta[b * 8 + 2 * i] = ok ? (float)gdx[i] : NAN;
        d_delta[b * 8 + 2 * i + 1] = ok ? (float)gdy[i] : NAN;
    }
}

int check(const hesic_warp_desc* d, const char* who) {
    HESIC_CHECK_ARG(d && d->B > 0 && d->B < 65536 && d->C > 0 && d->H > 1 && d->W > 1 && d->Ho > 0 && d->Wo > 0, "%s: bad geometry", who);
    return 0;
}

// blocks per image: 256 pixels per block pass, at most HESIC_HTRAIN_MAX_BLOCKS (the rest is a grid-stride loop)
int blocks_for(const hesic_warp_desc* d) { return grid_for((int64_t)d->Ho * d->Wo, 256, HESIC_HTRAIN_MAX_BLOCKS); }

}  // namespace

extern "C" int hesic_photometric_forward(const hesic_warp_desc* d, const float* img_a, const float* patch_b, const float* corners,
                                         const float* delta, double* h, double* partials, float* loss, void* stream) {
    if (int e = check(d, "photometric_forward")) return e;
    HESIC_CHECK_ARG(img_a && patch_b && corners && delta && h && partials && loss, "photometric_forward: null pointer");
    HESIC_CHECK_ARG(d->src_dtype == HESIC_F32 && d->dst_dtype == HESIC_F32, "photometric_forward: fp32 images only");
    const int nblk = blocks_for(d);
    hipLaunchKernelGGL(photo_dlt_kernel, dim3((d->B + 63) / 64), dim3(64), 0, (hipStream_t)stream, corners, delta, h, d->B);
    GArgs a; a.d = *d; a.src = img_a; a.other = patch_b; a.M = nullptr; a.h = h; a.partials = partials;
    hipLaunchKernelGGL(coord_kernel<PHOTO_FWD>, dim3(nblk, d->B), dim3(256), 0, (hipStream_t)stream, a);
    hipLaunchKernelGGL(photo_loss_finish_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, (const double*)partials, nblk * d->B,
                       (double)d->B * d->C * d->Ho * d->Wo, loss);
    HESIC_LAUNCH_RETURN("photometric_forward");
}

extern "C" int hesic_photometric_backward(const hesic_warp_desc* d, const float* img_a, const float* patch_b, const float* corners,
                                          const float* delta, const double* h, const float* grad_loss, double* partials, float* d_delta,
                                          void* stream) {
    if (int e = check(d, "photometric_backward")) return e;
    HESIC_CHECK_ARG(img_a && patch_b && corners && delta && h && grad_loss && partials && d_delta, "photometric_backward: null pointer");
    HESIC_CHECK_ARG(d->src_dtype == HESIC_F32 && d->dst_dtype == HESIC_F32, "photometric_backward: fp32 images only");
    const int nblk = blocks_for(d);
    GArgs a; a.d = *d; a.src = img_a; a.other = patch_b; a.M = nullptr; a.h = h; a.partials = partials;
    hipLaunchKernelGGL(coord_kernel<PHOTO_BWD>, dim3(nblk, d->B), dim3(256), 0, (hipStream_t)stream, a);
    hipLaunchKernelGGL(photo_bwd_finish_kernel, dim3((d->B + 63) / 64), dim3(64), 0, (hipStream_t)stream, (const double*)partials, nblk,
                       (double)d->B * d->C * d->Ho * d->Wo, grad_loss, corners, delta, h, d_delta, d->B);
    HESIC_LAUNCH_RETURN("photometric_backward");
}

extern "C" int hesic_warp_perspective_backward_m(const hesic_warp_desc* d, const void* src, const void* d_dst, const float* M,
                                                 double* partials, float* dM, void* stream) {
    if (int e = check(d, "warp_perspective_backward_m")) return e;
    HESIC_CHECK_ARG(src && d_dst && M && partials && dM, "warp_perspective_backward_m: null pointer");
    HESIC_CHECK_ARG((d->src_dtype == HESIC_F32 || d->src_dtype == HESIC_H16) && (d->dst_dtype == HESIC_F32 || d->dst_dtype == HESIC_H16),
                    "warp_perspective_backward_m: bad dtype");
    const int nblk = blocks_for(d);
    GArgs a; a.d = *d; a.src = src; a.other = d_dst; a.M = M; a.h = nullptr; a.partials = partials;
    hipLaunchKernelGGL(coord_kernel<WARP_BWD>, dim3(nblk, d->B), dim3(256), 0, (hipStream_t)stream, a);
    hipLaunchKernelGGL(warp_m_finish_kernel, dim3((d->B + 63) / 64), dim3(64), 0, (hipStream_t)stream, (const double*)partials, nblk, M,
                       d->m_is_dst_to_src, dM, d->B);
    HESIC_LAUNCH_RETURN("warp_perspective_backward_m");
}

extern "C" int hesic_perspective_transform_backward(const float* src, const float* dst, const float* dH, float* d_src, float* d_dst, int B,
                                                    void* stream) {
    HESIC_CHECK_ARG(src && dst && dH && (d_src || d_dst) && B > 0, "perspective_transform_backward: bad arguments");
    hipLaunchKernelGGL(perspective_transform_bwd_kernel, dim3((B + 63) / 64), dim3(64), 0, (hipStream_t)stream, src, dst, dH, d_src, d_dst, B);
    HESIC_LAUNCH_RETURN("perspective_transform_backward");
}

extern "C" int hesic_h_from_delta_backward(const float* corners, const float* delta, float ratio_a, float ratio_b, int subtract_origin,
                                           const float* dH, float* d_delta, int B, void* stream) {
    HESIC_CHECK_ARG(corners && delta && dH && d_delta && B > 0 && ratio_a > 0.f && ratio_b > 0.f, "h_from_delta_backward: bad arguments");
    hipLaunchKernelGGL(h_from_delta_bwd_kernel, dim3((B + 63) / 64), dim3(64), 0, (hipStream_t)stream, corners, delta, ratio_a, ratio_b,
                       subtract_origin, dH, d_delta, B);
    HESIC_LAUNCH_RETURN("h_from_delta_backward");
}

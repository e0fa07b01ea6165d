// Photometric refinement of a stereo homography (include/hesic_homography_refine.h): a grey pyramid of both views, the normal equations of a
// candidate on one level, and the Levenberg-Marquardt walk over them, coarse to fine.
//
// The image-sized work is the normal-equation launch: a thread maps its destination pixels through the candidate A (fp64: X, Y, Z = A p),
// takes the bilinear sample and the cell gradient of I1 there, and adds the 46 sums of w J^T J (upper triangle), w J^T r, w r^2 and the
// valid count into registers; a wave reduces by xor shuffles, the four waves through LDS, and the block leaves its 46 fp64 partials in the
// workspace.  Everything after it -- adding the blocks in index order, accepting or rejecting, the damped 8 x 8 solve, the level transitions
// -- is one block per pair (thread k adds column k; thread 0 does the rest).  No atomics, no host read, no fused multiply-adds: the numpy
// restatement (tests/homography_refine_ref.py) performs the same fp64 operations.
#include "common.h"
#pragma clang fp contract(off)      // before dlt.h: its 3x3 inverse is part of the restated arithmetic
#include "dlt.h"
#include "../../include/hesic_homography_refine.h"

namespace {

constexpr int NS = HESIC_HREFINE_SUMS, NSTATE = HESIC_HREFINE_STATE, MAXL = HESIC_HREFINE_MAX_LEVELS;
// per-pair state (fp64 words)
enum { S_BEST = 0, S_CAND = 9, S_KEPT = 18, S_LAMBDA = 64, S_COST_BEST = 65, S_COST_FIRST = 66, S_ACCEPTED = 67, S_REJECTED = 68,
       S_VALID_SHARE = 69, S_FIRST = 70, S_ALIVE = 71, S_HAVE_FIRST = 72, S_FLAT = 73 /* one word per level: I2 has no contrast there */ };
static_assert(S_FLAT + MAXL <= NSTATE && S_KEPT + NS == S_LAMBDA, "state layout");

struct PyrGeom {
    int B, nlev;
    int h[MAXL], w[MAXL];
    int64_t off[MAXL];          // first element of level l: view v of pair b starts at off[l] + (v * B + b) * h[l] * w[l]
    int64_t total;
};

bool pyr_geom(int B, int H, int W, int levels, PyrGeom* g) {
    if (B <= 0 || levels < 1 || levels > MAXL) return false;
    g->B = B; g->nlev = 0; g->total = 0;
    while (g->nlev < levels && H >= HESIC_HREFINE_MIN_SIDE && W >= HESIC_HREFINE_MIN_SIDE) {
        g->h[g->nlev] = H; g->w[g->nlev] = W; g->off[g->nlev] = g->total;
        g->total += 2 * (int64_t)B * H * W;
        ++g->nlev;
        H /= 2; W /= 2;
    }
    for (int l = g->nlev; l < MAXL; ++l) { g->h[l] = g->w[l] = 0; g->off[l] = 0; }
    return true;
}

// ------------------------------------------------------------------------------------------------------------------------------- pyramid
struct PyrArgs {
    PyrGeom g;
    const float* src[2];
    int64_t s[2][4];
    int C;
    float* pyr;
};

// the value of level L at (y, x), recomputed from the input: every level is the fp64 mean of the four ROUNDED values below it
template <int L>
__device__ float pyr_val(const float* p, int64_t sc, int64_t sy, int64_t sx, int C, int y, int x) {
    if constexpr (L == 0) {
        const float* q = p + y * sy + x * sx;
        if (C == 1) return q[0];
        return (float)((((double)q[0] + (double)q[sc]) + (double)q[2 * sc]) / 3.0);
    } else {
        const double a = pyr_val<L - 1>(p, sc, sy, sx, C, 2 * y, 2 * x), b = pyr_val<L - 1>(p, sc, sy, sx, C, 2 * y, 2 * x + 1);
        const double c = pyr_val<L - 1>(p, sc, sy, sx, C, 2 * y + 1, 2 * x), d = pyr_val<L - 1>(p, sc, sy, sx, C, 2 * y + 1, 2 * x + 1);
        return (float)((((a + b) + c) + d) * 0.25);
    }
}

// one thread per level-0 pixel of a view: it writes that pixel and every coarser pixel whose top-left corner it is
__global__ __launch_bounds__(256) void pyramid_kernel(const PyrArgs a) {
    const PyrGeom& g = a.g;
    const int v = blockIdx.y & 1, b = blockIdx.y >> 1;
    const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    if (i >= (int64_t)g.h[0] * g.w[0]) return;
    const int x = i % g.w[0], y = i / g.w[0];
    const float* p = a.src[v] + b * a.s[v][0];
    const int64_t sc = a.s[v][1], sy = a.s[v][2], sx = a.s[v][3];
    a.pyr[g.off[0] + ((int64_t)v * g.B + b) * g.h[0] * g.w[0] + i] = pyr_val<0>(p, sc, sy, sx, a.C, y, x);
    for (int l = 1; l < g.nlev; ++l) {
        if ((y | x) & ((1 << l) - 1)) break;
        const int yl = y >> l, xl = x >> l;
        if (yl >= g.h[l] || xl >= g.w[l]) break;
        float r;
        switch (l) {
            case 1: r = pyr_val<1>(p, sc, sy, sx, a.C, yl, xl); break;
            case 2: r = pyr_val<2>(p, sc, sy, sx, a.C, yl, xl); break;
            case 3: r = pyr_val<3>(p, sc, sy, sx, a.C, yl, xl); break;
            case 4: r = pyr_val<4>(p, sc, sy, sx, a.C, yl, xl); break;
            default: r = pyr_val<5>(p, sc, sy, sx, a.C, yl, xl); break;
        }
        a.pyr[g.off[l] + (((int64_t)v * g.B + b) * g.h[l] + yl) * g.w[l] + xl] = r;
    }
}
static_assert(MAXL == 6, "pyramid_kernel's switch covers levels 1..5");

// ---------------------------------------------------------------------------------------------------------------------- normal equations
__global__ __launch_bounds__(256) void normal_eq_kernel(const float* __restrict__ I1, const float* __restrict__ I2, int Hl, int Wl,
                                                        const double* __restrict__ A, int64_t a_stride, double huber,
                                                        double* __restrict__ partials) {
    __shared__ double red[4][NS];
    const int b = blockIdx.y;
    I1 += (int64_t)b * Hl * Wl;
    I2 += (int64_t)b * Hl * Wl;
    double m[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) m[k] = A[b * a_stride + k];
    double acc[NS];
#pragma unroll
    for (int k = 0; k < NS; ++k) acc[k] = 0.0;
    const int total = Hl * Wl;
    const double xmax = (double)(Wl - 2), ymax = (double)(Hl - 2);
    for (int i = blockIdx.x * 256 + threadIdx.x; i < total; i += gridDim.x * 256) {
        const double x = (double)(i % Wl), y = (double)(i / Wl);
        const double X = (m[0] * x + m[1] * y) + m[2], Y = (m[3] * x + m[4] * y) + m[5], Z = (m[6] * x + m[7] * y) + m[8];
        const double iz = 1.0 / Z;                                                      // the one division by Z
        const double u = X * iz, v_ = Y * iz;
        const double fx0 = floor(u), fy0 = floor(v_);
        if (!(fx0 >= 0.0 && fy0 >= 0.0 && fx0 <= xmax && fy0 <= ymax)) continue;       // a NaN coordinate compares false: invalid
        const int x0 = (int)fx0, y0 = (int)fy0;                                        // in [0, Wl - 2] x [0, Hl - 2]: the four taps are inside
        const double fx = u - fx0, fy = v_ - fy0;
        const float* q = I1 + y0 * Wl + x0;
        const double ta = q[0], tb = q[1], tc = q[Wl], td = q[Wl + 1];
        const double gx = (tb - ta) * (1.0 - fy) + (td - tc) * fy;
        const double gy = (tc - ta) * (1.0 - fx) + (td - tb) * fx;
        const double val = (ta * (1.0 - fx) + tb * fx) * (1.0 - fy) + (tc * (1.0 - fx) + td * fx) * fy;
        const double r = val - (double)I2[i];
        const double t0 = gx * iz, t1 = gy * iz, t2 = -(gx * u + gy * v_) * iz;
        const double J[8] = {t0 * x, t0 * y, t0, t1 * x, t1 * y, t1, t2 * x, t2 * y};
        const double w = huber > 0.0 ? fmin(1.0, huber / fabs(r)) : 1.0;
        double wJ[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) wJ[k] = w * J[k];
        int k = 0;
#pragma unroll
        for (int r_ = 0; r_ < 8; ++r_)
#pragma unroll
            for (int c = r_; c < 8; ++c) acc[k++] += wJ[r_] * J[c];
#pragma unroll
        for (int c = 0; c < 8; ++c) acc[36 + c] += wJ[c] * r;
        acc[44] += (w * r) * r;
        acc[45] += 1.0;
    }
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
#pragma unroll
    for (int k = 0; k < NS; ++k) {
        const double s = wave_sum_d(acc[k]);
        if (lane == 0) red[wave][k] = s;
    }
    __syncthreads();
    if (threadIdx.x < NS)
        partials[((int64_t)b * gridDim.x + blockIdx.x) * NS + threadIdx.x] =
            ((red[0][threadIdx.x] + red[1][threadIdx.x]) + red[2][threadIdx.x]) + red[3][threadIdx.x];
}

// --------------------------------------------------------------------------------------------------------------------- per-pair steps
__device__ void mat3(const double* a, const double* b, double* o) {
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) o[3 * i + j] = (a[3 * i] * b[j] + a[3 * i + 1] * b[3 + j]) + a[3 * i + 2] * b[6 + j];
}

__device__ void norm22(double* m) {
    const double s = m[8];
    for (int k = 0; k < 9; ++k) m[k] = m[k] / s;
}

// T of level l (level-l pixel -> level-0 pixel) and its inverse
__device__ void level_T(int l, double* T, double* Ti) {
    const double s = (double)(1 << l), o = (s - 1.0) / 2.0;
    const double t[9] = {s, 0, o, 0, s, o, 0, 0, 1.0}, ti[9] = {1.0 / s, 0, -o / s, 0, 1.0 / s, -o / s, 0, 0, 1.0};
    for (int k = 0; k < 9; ++k) { T[k] = t[k]; Ti[k] = ti[k]; }
}

__device__ void to_level(double* A, int src, int dst) {
    if (src == dst) return;
    double Ts[9], Tsi[9], Td[9], Tdi[9], t[9], A0[9];
    level_T(src, Ts, Tsi);
    level_T(dst, Td, Tdi);
    mat3(Ts, A, t); mat3(t, Tsi, A0);
    mat3(Tdi, A0, t); mat3(t, Td, A);
    norm22(A);
}

__global__ void init_kernel(const float* __restrict__ h, double* __restrict__ state, int B) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    double m[9], a[9];
    for (int k = 0; k < 9; ++k) m[k] = h[b * 9 + k];
    inv3(m, a);
    norm22(a);
    double* s = state + (int64_t)b * NSTATE;
    for (int k = 0; k < NSTATE; ++k) s[k] = 0.0;
    for (int k = 0; k < 9; ++k) s[S_BEST + k] = s[S_CAND + k] = a[k];
}

// A level of pair b's I2 is flat when its largest and smallest pixel are equal.  A view without contrast says nothing about geometry: the
// residual is then I1(w(p)) minus a constant, and "descent" only drags the sampling window towards the parts of I1 nearest that constant.
// A flat I1 needs no such mark: its gradients, hence J, are zero and the solve is singular.  Block (j, l, b) leaves the smallest and the
// largest of its pixels at range[((b * MAXL + l) * FLAT_BLOCKS + j) * 2]; transition_kernel finishes the level it enters.
constexpr int FLAT_BLOCKS = 64;

__global__ __launch_bounds__(256) void flat_kernel(const float* __restrict__ pyr, const PyrGeom g, float* __restrict__ range) {
    __shared__ float lo[4], hi[4];
    const int l = blockIdx.y, b = blockIdx.z;
    const int n = g.h[l] * g.w[l];
    const float* I2 = pyr + g.off[l] + ((int64_t)g.B + b) * n;
    float mn = I2[0], mx = I2[0];
    for (int i = blockIdx.x * 256 + threadIdx.x; i < n; i += FLAT_BLOCKS * 256) {
        const float v = I2[i];
        mn = fminf(mn, v); mx = fmaxf(mx, v);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        mn = fminf(mn, __shfl_xor(mn, o, 64));
        mx = fmaxf(mx, __shfl_xor(mx, o, 64));
    }
    if ((threadIdx.x & 63) == 0) { lo[threadIdx.x >> 6] = mn; hi[threadIdx.x >> 6] = mx; }
    __syncthreads();
    if (threadIdx.x == 0) {
        float* o = range + (((int64_t)b * MAXL + l) * FLAT_BLOCKS + blockIdx.x) * 2;
        o[0] = fminf(fminf(lo[0], lo[1]), fminf(lo[2], lo[3]));
        o[1] = fmaxf(fmaxf(hi[0], hi[1]), fmaxf(hi[2], hi[3]));
    }
}

// One wave per pair.  The best of level `src` becomes level `dst`'s start: best = candidate, lambda = 1e-3, the next candidate is the
// level's first; and level `dst` is marked flat or not from flat_kernel's block ranges (lane j reads block j's).
__global__ __launch_bounds__(64) void transition_kernel(double* __restrict__ state, const float* __restrict__ range, int src, int dst) {
    const int b = blockIdx.x;
    const float* r = range + (((int64_t)b * MAXL + dst) * FLAT_BLOCKS + threadIdx.x) * 2;
    float mn = r[0], mx = r[1];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        mn = fminf(mn, __shfl_xor(mn, o, 64));
        mx = fmaxf(mx, __shfl_xor(mx, o, 64));
    }
    if (threadIdx.x != 0) return;
    double* s = state + (int64_t)b * NSTATE;
    double a[9];
    for (int k = 0; k < 9; ++k) a[k] = s[S_BEST + k];
    to_level(a, src, dst);
    for (int k = 0; k < 9; ++k) s[S_BEST + k] = s[S_CAND + k] = a[k];
    s[S_LAMBDA] = 1e-3; s[S_FIRST] = 1.0; s[S_ALIVE] = 1.0;
    s[S_FLAT + dst] = mx == mn ? 1.0 : 0.0;
}
static_assert(FLAT_BLOCKS == 64, "transition_kernel reads one block range per lane");

// Gaussian elimination with partial pivoting on the augmented 8 x 9 system; false for a singular or non-finite solve.  Fully unrolled with
// the row exchange written as selects, so that M stays in registers (dynamic row indices would put it in scratch memory); the operations
// and their order are those of the rolled loops (csrc/homography_train.hip: solve8).
__device__ bool solve8(double (&M)[8][9], double (&x)[8]) {
    bool finite = true;
#pragma unroll
    for (int r = 0; r < 8; ++r)
#pragma unroll
        for (int c = 0; c < 9; ++c) finite = finite && isfinite(M[r][c]);
    if (!finite) return false;
    bool ok = true;
#pragma unroll
    for (int c = 0; c < 8; ++c) {
        int piv = c;
        double big = fabs(M[c][c]);
#pragma unroll
        for (int r = c + 1; r < 8; ++r) {
            const double v = fabs(M[r][c]);
            if (v > big) { big = v; piv = r; }
        }
        ok = ok && big >= 1e-300;
#pragma unroll
        for (int r = c + 1; r < 8; ++r) {
            const bool sw = piv == r;
#pragma unroll
            for (int k = 0; k < 9; ++k) {
                const double t = M[c][k], u = M[r][k];
                M[c][k] = sw ? u : t;
                M[r][k] = sw ? t : u;
            }
        }
        const double inv = 1.0 / M[c][c];
#pragma unroll
        for (int r = c + 1; r < 8; ++r) {
            const double f = M[r][c] * inv;
#pragma unroll
            for (int k = c; k < 9; ++k) M[r][k] = M[r][k] - f * M[c][k];
        }
    }
#pragma unroll
    for (int c = 7; c >= 0; --c) {
        double s = M[c][8];
#pragma unroll
        for (int k = c + 1; k < 8; ++k) s = s - M[c][k] * x[k];
        x[c] = s / M[c][c];
    }
#pragma unroll
    for (int c = 0; c < 8; ++c) ok = ok && isfinite(x[c]);
    return ok;
}

// what one pair does with the sums of its candidate: `s` is the pair's state, `sums` the 46 sums (both in LDS)
__device__ void update_pair(double* s, const double* sums, double area, double min_overlap, int level, int record_first) {
    const double n = sums[45];
    const double cost = n > 0.0 ? sums[44] / n : 0.0;
    if (record_first) {
        s[S_COST_FIRST] = cost; s[S_HAVE_FIRST] = 1.0;
        return;
    }
    if (s[S_ALIVE] == 0.0) return;
    bool ok;
    if (s[S_FIRST] != 0.0) {
        s[S_FIRST] = 0.0;
        if (level == 0 && s[S_HAVE_FIRST] == 0.0) { s[S_COST_FIRST] = cost; s[S_HAVE_FIRST] = 1.0; }
        if (!(n > 0.0) || s[S_FLAT + level] != 0.0) { s[S_ALIVE] = 0.0; return; }      // nothing to align, or nothing to align TO
        ok = true;
    } else {
        ok = cost < s[S_COST_BEST] && n >= min_overlap * area;
        s[ok ? S_ACCEPTED : S_REJECTED] += 1.0;
    }
    double lam = s[S_LAMBDA];
    if (ok) {
        for (int k = 0; k < 9; ++k) s[S_BEST + k] = s[S_CAND + k];
        for (int k = 0; k < NS; ++k) s[S_KEPT + k] = sums[k];
        s[S_COST_BEST] = cost; s[S_VALID_SHARE] = n / area;
        lam = fmax(lam / 10.0, 1e-9);
    } else {
        lam = fmin(lam * 10.0, 1e6);
    }
    double M[8][9], delta[8];
    int k = 0;
#pragma unroll
    for (int r = 0; r < 8; ++r)
#pragma unroll
        for (int c = r; c < 8; ++c) { M[r][c] = M[c][r] = s[S_KEPT + k]; ++k; }
#pragma unroll
    for (int r = 0; r < 8; ++r) {
        M[r][r] = M[r][r] + lam * M[r][r];
        M[r][8] = -s[S_KEPT + 36 + r];
    }
    if (solve8(M, delta)) {
#pragma unroll
        for (int c = 0; c < 8; ++c) s[S_CAND + c] = s[S_BEST + c] + delta[c];
        s[S_CAND + 8] = s[S_BEST + 8];
    } else {
        s[S_REJECTED] += 1.0;
        lam = fmin(lam * 10.0, 1e6);
        for (int c = 0; c < 9; ++c) s[S_CAND + c] = s[S_BEST + c];
    }
    s[S_LAMBDA] = lam;
}

// One block per pair.  The pair's partials and state come into LDS with coalesced loads (one thread walking them in global memory pays a
// miss per step); thread k < 46 adds column k in block order; thread 0 takes the decision and the solve; the state goes back.
// record_first = 1: the pass only records level 0's cost of the input matrix.
__global__ __launch_bounds__(256) void update_kernel(double* __restrict__ state, const double* __restrict__ partials, int nblk, double area,
                                                     double min_overlap, int level, int record_first) {
    __shared__ double part[HESIC_HREFINE_MAX_BLOCKS * NS];
    __shared__ double st[NSTATE];
    __shared__ double sums[NS];
    const int b = blockIdx.x, tid = threadIdx.x;
    for (int i = tid; i < nblk * NS; i += 256) part[i] = partials[(int64_t)b * nblk * NS + i];
    if (tid < NSTATE) st[tid] = state[(int64_t)b * NSTATE + tid];
    __syncthreads();
    if (tid < NS) {
        double s = 0.0;
#pragma unroll 8
        for (int j = 0; j < nblk; ++j) s += part[j * NS + tid];
        sums[tid] = s;
    }
    __syncthreads();
    if (tid == 0) update_pair(st, sums, area, min_overlap, level, record_first);
    __syncthreads();
    if (tid < NSTATE) state[(int64_t)b * NSTATE + tid] = st[tid];
}

__global__ void final_kernel(const double* __restrict__ state, const float* __restrict__ h, float* __restrict__ h_out,
                             double* __restrict__ info, int B, int levels_used) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    const double* s = state + (int64_t)b * NSTATE;
    bool refined = s[S_ALIVE] != 0.0 && s[S_ACCEPTED] > 0.0 && s[S_COST_BEST] < s[S_COST_FIRST];
    float o[9];
    if (refined) {
        double a[9], m[9];
        for (int k = 0; k < 9; ++k) a[k] = s[S_BEST + k];
        inv3(a, m);
        norm22(m);
        for (int k = 0; k < 9; ++k) {
            o[k] = (float)m[k];
            refined = refined && isfinite(o[k]);
        }
    }
    for (int k = 0; k < 9; ++k) h_out[b * 9 + k] = refined ? o[k] : h[b * 9 + k];
    double* q = info + (int64_t)b * HESIC_HREFINE_INFO;
    q[0] = s[S_COST_FIRST];
    q[1] = refined ? s[S_COST_BEST] : s[S_COST_FIRST];
    q[2] = s[S_ACCEPTED]; q[3] = s[S_REJECTED]; q[4] = s[S_VALID_SHARE];
    q[5] = (double)levels_used; q[6] = refined ? 1.0 : 0.0; q[7] = 0.0;
}

int launch_pyramid(const float* x1, const int64_t* s1, const float* x2, const int64_t* s2, int C, const PyrGeom& g, float* pyr,
                   hipStream_t stream) {
    PyrArgs a;
    a.g = g; a.src[0] = x1; a.src[1] = x2; a.C = C; a.pyr = pyr;
    for (int k = 0; k < 4; ++k) { a.s[0][k] = s1[k]; a.s[1][k] = s2[k]; }
    hipLaunchKernelGGL(pyramid_kernel, dim3((unsigned)cdiv64((int64_t)g.h[0] * g.w[0], 256), 2 * g.B), dim3(256), 0, stream, a);
    return 0;
}

void launch_normal_eq(const float* pyr, const PyrGeom& g, int level, const double* A, int64_t a_stride, double huber, double* partials,
                      hipStream_t stream) {
    const int Hl = g.h[level], Wl = g.w[level];
    const float* I1 = pyr + g.off[level];
    hipLaunchKernelGGL(normal_eq_kernel, dim3(hesic_hrefine_blocks(Hl, Wl), g.B), dim3(256), 0, stream, I1, I1 + (int64_t)g.B * Hl * Wl, Hl,
                       Wl, A, a_stride, huber, partials);
}

int check_images(const float* x1, const int64_t* s1, const float* x2, const int64_t* s2, int B, int C, int H, int W, const char* who) {
    HESIC_CHECK_ARG(x1 && x2 && s1 && s2, "%s: null pointer", who);
    HESIC_CHECK_ARG(B > 0 && B < 32768 && (C == 1 || C == 3), "%s: bad batch or channel count (C is 1 or 3)", who);
    HESIC_CHECK_ARG(H >= HESIC_HREFINE_MIN_SIDE && W >= HESIC_HREFINE_MIN_SIDE && (int64_t)H * W < (1 << 30),
                    "%s: images of %d to 2^15 pixels on a side", who, HESIC_HREFINE_MIN_SIDE);
    for (int k = 0; k < 4; ++k) HESIC_CHECK_ARG(s1[k] >= 0 && s2[k] >= 0, "%s: negative stride", who);
    return 0;
}

}  // namespace

extern "C" int hesic_hrefine_levels(int H, int W, int levels) {
    PyrGeom g;
    if (!pyr_geom(1, H, W, levels, &g)) return -1;
    return g.nlev;
}

extern "C" int hesic_hrefine_blocks(int Hl, int Wl) { return grid_for((int64_t)Hl * Wl, 256, HESIC_HREFINE_MAX_BLOCKS); }

extern "C" int64_t hesic_hrefine_pyramid_elems(int B, int H, int W, int levels) {
    PyrGeom g;
    if (!pyr_geom(B, H, W, levels, &g)) return -1;
    return g.total;
}

extern "C" int64_t hesic_homography_refine_ws_bytes(int B, int H, int W, int levels) {
    PyrGeom g;
    if (!pyr_geom(B, H, W, levels, &g)) return -1;
    const int64_t pyr_bytes = (g.total * 4 + 255) / 256 * 256;
    return pyr_bytes + (int64_t)B * (HESIC_HREFINE_MAX_BLOCKS * NS + NSTATE) * 8 + (int64_t)B * MAXL * FLAT_BLOCKS * 2 * 4;
}

extern "C" int hesic_hrefine_pyramid(const float* x1, const int64_t* s1, const float* x2, const int64_t* s2, int B, int C, int H, int W,
                                     int levels, float* pyr, void* stream) {
    if (int e = check_images(x1, s1, x2, s2, B, C, H, W, "hrefine_pyramid")) return e;
    PyrGeom g;
    HESIC_CHECK_ARG(pyr && pyr_geom(B, H, W, levels, &g) && g.nlev == levels, "hrefine_pyramid: levels must be what hesic_hrefine_levels returns");
    launch_pyramid(x1, s1, x2, s2, C, g, pyr, (hipStream_t)stream);
    HESIC_LAUNCH_RETURN("hrefine_pyramid");
}

extern "C" int hesic_hrefine_normal_eq(const float* pyr, int B, int H, int W, int levels, int level, const double* A, int64_t a_stride,
                                       double huber, double* partials, void* stream) {
    PyrGeom g;
    HESIC_CHECK_ARG(pyr && A && partials && B > 0 && B < 32768 && a_stride >= 9, "hrefine_normal_eq: bad arguments");
    HESIC_CHECK_ARG(pyr_geom(B, H, W, levels, &g) && g.nlev == levels && level >= 0 && level < levels && (int64_t)H * W < (1 << 30),
                    "hrefine_normal_eq: bad level geometry");
    launch_normal_eq(pyr, g, level, A, a_stride, huber, partials, (hipStream_t)stream);
    HESIC_LAUNCH_RETURN("hrefine_normal_eq");
}

extern "C" int hesic_homography_refine(const float* x1, const int64_t* s1, const float* x2, const int64_t* s2, int B, int C, int H, int W,
                                       const float* h, int levels, int iters, double huber, double min_overlap, void* ws, int64_t ws_bytes,
                                       float* h_out, double* info, void* stream) {
    if (int e = check_images(x1, s1, x2, s2, B, C, H, W, "homography_refine")) return e;
    PyrGeom g;
    HESIC_CHECK_ARG(h && h_out && info && ws, "homography_refine: null pointer");
    HESIC_CHECK_ARG(iters >= 0 && iters <= 1000 && min_overlap >= 0.0 && min_overlap <= 1.0 && !(huber != huber),
                    "homography_refine: iters in [0, 1000], min_overlap in [0, 1]");
    HESIC_CHECK_ARG(pyr_geom(B, H, W, levels, &g) && g.nlev >= 1, "homography_refine: levels in [1, %d]", MAXL);
    HESIC_CHECK_ARG(ws_bytes >= hesic_homography_refine_ws_bytes(B, H, W, levels) && ((uintptr_t)ws & 7) == 0,
                    "homography_refine: workspace too small or misaligned");
    hipStream_t st = (hipStream_t)stream;
    float* pyr = (float*)ws;
    double* partials = (double*)((char*)ws + (g.total * 4 + 255) / 256 * 256);
    double* state = partials + (int64_t)B * HESIC_HREFINE_MAX_BLOCKS * NS;
    float* range = (float*)(state + (int64_t)B * NSTATE);
    const dim3 pb((B + 63) / 64), pt(64);
    launch_pyramid(x1, s1, x2, s2, C, g, pyr, st);
    hipLaunchKernelGGL(init_kernel, pb, pt, 0, st, h, state, B);
    hipLaunchKernelGGL(flat_kernel, dim3(FLAT_BLOCKS, g.nlev, B), dim3(256), 0, st, (const float*)pyr, g, range);
    const int L = g.nlev;
    if (L > 1) {                // level 0's cost of the input matrix: the walk starts above it
        launch_normal_eq(pyr, g, 0, state + S_CAND, NSTATE, huber, partials, st);
        hipLaunchKernelGGL(update_kernel, dim3(B), dim3(256), 0, st, state, (const double*)partials, hesic_hrefine_blocks(g.h[0], g.w[0]),
                           (double)g.h[0] * g.w[0], min_overlap, 0, 1);
    }
    for (int l = L - 1; l >= 0; --l) {
        hipLaunchKernelGGL(transition_kernel, dim3(B), dim3(64), 0, st, state, (const float*)range, l == L - 1 ? 0 : l + 1, l);
        const int nblk = hesic_hrefine_blocks(g.h[l], g.w[l]);
        for (int it = 0; it <= iters; ++it) {
            launch_normal_eq(pyr, g, l, state + S_CAND, NSTATE, huber, partials, st);
            hipLaunchKernelGGL(update_kernel, dim3(B), dim3(256), 0, st, state, (const double*)partials, nblk, (double)g.h[l] * g.w[l],
                               min_overlap, l, 0);
        }
    }
    hipLaunchKernelGGL(final_kernel, pb, pt, 0, st, (const double*)state, h, h_out, info, B, L);
    HESIC_LAUNCH_RETURN("homography_refine");
}

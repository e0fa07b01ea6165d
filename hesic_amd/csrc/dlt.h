// The 4-point DLT and the 3x3 inverse shared by homography.hip (inference) and homography_train.hip (its adjoint): fp64, one thread
// per pair.  kornia is not vendored by the reference (unpinned): the DLT is restated from its published definition
// (8x8 linear system, rows [x y 1 0 0 0 -xu -yu | u], [0 0 0 x y 1 -xv -yv | v]).
#pragma once

// solve the 4-point DLT for dst ~ H src; returns false for a singular configuration
static __device__ bool dlt4(const double sx[4], const double sy[4], const double dx[4], const double dy[4], double h[9]) {
    double A[8][9];
    for (int i = 0; i < 4; ++i) {
        const double x = sx[i], y = sy[i], u = dx[i], v = dy[i];
        double* r0 = A[2 * i];
        double* r1 = A[2 * i + 1];
        r0[0] = x; r0[1] = y; r0[2] = 1; r0[3] = 0; r0[4] = 0; r0[5] = 0; r0[6] = -x * u; r0[7] = -y * u; r0[8] = u;
        r1[0] = 0; r1[1] = 0; r1[2] = 0; r1[3] = x; r1[4] = y; r1[5] = 1; r1[6] = -x * v; r1[7] = -y * v; r1[8] = v;
    }
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
        for (int k = c + 1; k < 8; ++k) s -= A[c][k] * h[k];
        h[c] = s / A[c][c];
    }
    h[8] = 1.0;
    return true;
}

static __device__ void inv3(const double m[9], double o[9]) {
    const double c0 = m[4] * m[8] - m[5] * m[7], c1 = m[5] * m[6] - m[3] * m[8], c2 = m[3] * m[7] - m[4] * m[6];
    const double id = 1.0 / (m[0] * c0 + m[1] * c1 + m[2] * c2);
    o[0] = c0 * id; o[1] = (m[2] * m[7] - m[1] * m[8]) * id; o[2] = (m[1] * m[5] - m[2] * m[4]) * id;
    o[3] = c1 * id; o[4] = (m[0] * m[8] - m[2] * m[6]) * id; o[5] = (m[2] * m[3] - m[0] * m[5]) * id;
    o[6] = c2 * id; o[7] = (m[1] * m[6] - m[0] * m[7]) * id; o[8] = (m[0] * m[4] - m[1] * m[3]) * id;
}

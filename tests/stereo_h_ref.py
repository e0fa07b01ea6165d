"""NumPy restatement of ``hesic_amd.stereo_h`` (steps 1-6 of the stereo homography estimator), for the tests only.

It follows the definitions of ``hesic_amd/csrc/stereo_h.hip`` operation by operation (fp32 where the kernels use fp32, fp64 where
they use fp64, the same rounding calls, the same orders of summation, sampling and tie-breaks), so the GPU stages can be compared
with it stage by stage.  One place is not bit-for-bit: the descriptor dot products of the matcher are formed here as exact fp64
products summed in fp64 and rounded once to fp32, where the matrix cores form a k-ordered fp32 fused multiply-add chain; the two
differ by a few ulp, which moves a ratio-test decision only when it sits on its bar.

The product never imports this module.
"""
from __future__ import annotations

import numpy as np

N_OCTAVES, N_LAYERS, THRESHOLD = 4, 3, np.float32(100.0)
F = np.float32
FLT_EPS = float(np.finfo(np.float32).eps)

# OpenCV SURF's Haar patterns at size 9: (x1, y1, x2, y2, weight) of each box, relative to the top-left sample
_DX = ((0, 2, 3, 7, 1), (3, 2, 6, 7, -2), (6, 2, 9, 7, 1))
_DY = ((2, 0, 7, 3, 1), (2, 3, 7, 6, -2), (2, 6, 7, 9, 1))
_DXY = ((1, 1, 4, 4, 1), (5, 1, 8, 4, -1), (1, 5, 4, 8, -1), (5, 5, 8, 8, 1))


# ---------------------------------------------------------------- step 1
def to_u8(img):
    """(3, H, W) uint8, or float in [0, 1] quantised as rint(clamp(x, 0, 1) * 255) in fp32."""
    img = np.asarray(img)
    if img.dtype == np.uint8:
        return img
    x = np.clip(img.astype(np.float32), F(0), F(1)) * F(255)
    return np.rint(x).astype(np.uint8)


def grey(img):
    """cvtColor(COLOR_BGR2GRAY) of an RGB array (OpenCV reads channel 0 as blue): 0.114 R + 0.587 G + 0.299 B in OpenCV's 14-bit
    fixed point."""
    c = to_u8(img).astype(np.int32)
    return ((c[0] * 1868 + c[1] * 9617 + c[2] * 4899 + 8192) >> 14).astype(np.int32)


def integral(g):
    H, W = g.shape
    out = np.zeros((H + 1, W + 1), dtype=np.int64)
    out[1:, 1:] = g.astype(np.int64).cumsum(0).cumsum(1)
    return out.astype(np.int32)


# ---------------------------------------------------------------- step 2
def layer_geometry(H, W):
    """[(octave, layer, size, step)] in generation order: 4 octaves of 5 layers."""
    return [(o, l, (9 + 6 * l) << o, 1 << o) for o in range(N_OCTAVES) for l in range(N_LAYERS + 2)]


def _pattern(src, size):
    ratio = F(size) / F(9)
    out = []
    for x1, y1, x2, y2, w in src:
        dx1, dy1, dx2, dy2 = (int(np.rint(ratio * F(v))) for v in (x1, y1, x2, y2))
        out.append((dx1, dy1, dx2, dy2, F(w) / F((dx2 - dx1) * (dy2 - dy1))))
    return out


def _haar(I, pat, r0, c0):
    """Sum over the boxes of (box sum * weight): each product in fp32, the sum in fp64, rounded to fp32 (OpenCV's calcHaarPattern)."""
    d = np.zeros(r0.shape, dtype=np.float64)
    for dx1, dy1, dx2, dy2, w in pat:
        v = (I[r0 + dy1, c0 + dx1].astype(np.int64) + I[r0 + dy2, c0 + dx2] - I[r0 + dy2, c0 + dx1] - I[r0 + dy1, c0 + dx2])
        d += (v.astype(np.float32) * w).astype(np.float64)
    return d.astype(np.float32)


def hessian_layers(I):
    """[det (H // step, W // step) fp32] per layer in generation order; 0 where the filter does not fit."""
    H, W = I.shape[0] - 1, I.shape[1] - 1
    dets = []
    for o, l, size, step in layer_geometry(H, W):
        R, C = H // step, W // step
        det = np.zeros((R, C), dtype=np.float32)
        if size <= H and size <= W:
            si, sj = 1 + (H - size) // step, 1 + (W - size) // step
            m = (size // 2) // step
            r0 = (np.arange(si) * step)[:, None] + np.zeros((1, sj), dtype=np.int64)
            c0 = (np.arange(sj) * step)[None, :] + np.zeros((si, 1), dtype=np.int64)
            dx, dy, dxy = (_haar(I, _pattern(p, size), r0, c0) for p in (_DX, _DY, _DXY))
            det[m:m + si, m:m + sj] = dx * dy - F(0.81) * dxy * dxy
        dets.append(det)
    return dets


def _solve3(A, b):
    """Cramer's rule in fp64 on the fp32 system, result in fp32 (zeros where the determinant is 0)."""
    A = A.astype(np.float64)
    b = b.astype(np.float64)
    a00, a01, a02, a10, a11, a12, a20, a21, a22 = (A[..., i, j] for i in range(3) for j in range(3))
    det = a00 * (a11 * a22 - a12 * a21) - a01 * (a10 * a22 - a12 * a20) + a02 * (a10 * a21 - a11 * a20)
    ok = det != 0
    inv = np.where(ok, 1.0 / np.where(ok, det, 1.0), 0.0)
    b0, b1, b2 = b[..., 0], b[..., 1], b[..., 2]
    x0 = (b0 * (a11 * a22 - a12 * a21) - a01 * (b1 * a22 - a12 * b2) + a02 * (b1 * a21 - a11 * b2)) * inv
    x1 = (a00 * (b1 * a22 - a12 * b2) - b0 * (a10 * a22 - a12 * a20) + a02 * (a10 * b2 - b1 * a20)) * inv
    x2 = (a00 * (a11 * b2 - b1 * a21) - a01 * (a10 * b2 - b1 * a20) + b0 * (a10 * a21 - a11 * a20)) * inv
    return np.stack([x0, x1, x2], -1).astype(np.float32)


def detect(I, dets=None):
    """Candidates in generation order (octave, middle layer, row, column): (N, 4) fp32 [x, y, size, response]."""
    H, W = I.shape[0] - 1, I.shape[1] - 1
    dets = hessian_layers(I) if dets is None else dets
    geo = layer_geometry(H, W)
    out = []
    for o in range(N_OCTAVES):
        for l in range(1, N_LAYERS + 1):
            k = o * (N_LAYERS + 2) + l
            _, _, size, step = geo[k]
            R, C = H // step, W // step
            m = (geo[k + 1][2] // 2) // step + 1
            if R - 2 * m <= 0 or C - 2 * m <= 0:
                continue
            lo, mid, hi = dets[k - 1], dets[k], dets[k + 1]
            ii, jj = np.meshgrid(np.arange(m, R - m), np.arange(m, C - m), indexing="ij")
            v0 = mid[ii, jj]
            N9 = np.stack([d[ii + dy, jj + dx] for d in (lo, mid, hi) for dy in (-1, 0, 1) for dx in (-1, 0, 1)], -1)
            others = np.delete(N9, 13, axis=-1)
            keep = (v0 > THRESHOLD) & (v0[..., None] > others).all(-1)
            ii, jj, v0, N = ii[keep], jj[keep], v0[keep], N9[keep].reshape(-1, 3, 9)
            if not len(v0):
                continue
            two = F(2)
            b = np.stack([-(N[:, 1, 5] - N[:, 1, 3]) / two, -(N[:, 1, 7] - N[:, 1, 1]) / two, -(N[:, 2, 4] - N[:, 0, 4]) / two], -1)
            dxx = N[:, 1, 3] - two * N[:, 1, 4] + N[:, 1, 5]
            dyy = N[:, 1, 1] - two * N[:, 1, 4] + N[:, 1, 7]
            dss = N[:, 0, 4] - two * N[:, 1, 4] + N[:, 2, 4]
            dxy = (N[:, 1, 8] - N[:, 1, 6] - N[:, 1, 2] + N[:, 1, 0]) / F(4)
            dxs = (N[:, 2, 5] - N[:, 2, 3] - N[:, 0, 5] + N[:, 0, 3]) / F(4)
            dys = (N[:, 2, 7] - N[:, 2, 1] - N[:, 0, 7] + N[:, 0, 1]) / F(4)
            A = np.stack([dxx, dxy, dxs, dxy, dyy, dys, dxs, dys, dss], -1).reshape(-1, 3, 3)
            x = _solve3(A, b)
            ok = (x != 0).any(-1) & (np.abs(x) <= 1).all(-1)
            ci = (step * (ii - (size // 2) // step)).astype(np.float32) + F((size - 1) * 0.5)
            cj = (step * (jj - (size // 2) // step)).astype(np.float32) + F((size - 1) * 0.5)
            px = cj + x[:, 0] * F(step)
            py = ci + x[:, 1] * F(step)
            ps = np.rint(F(size) + x[:, 2] * F(size - geo[k - 1][2]))
            out.append(np.stack([px, py, ps, v0], -1)[ok])
    return np.concatenate(out).astype(np.float32) if out else np.zeros((0, 4), np.float32)


def select(cands, max_keypoints):
    """The strongest ``max_keypoints`` (response descending, ties to the earlier candidate), kept in generation order."""
    if len(cands) <= max_keypoints:
        return cands
    order = np.lexsort((np.arange(len(cands)), -cands[:, 3].astype(np.float64)))
    keep = np.zeros(len(cands), bool)
    keep[order[:max_keypoints]] = True
    return cands[keep]


# ---------------------------------------------------------------- step 3
def gauss_table():
    """(20, 20) fp32 weights of the descriptor samples, sigma 3.3 sample spacings (= 3.3 s) around the keypoint."""
    u = np.arange(20, dtype=np.float64) - 9.5
    return np.exp(-(u[:, None] ** 2 + u[None, :] ** 2) / (2 * 3.3 * 3.3)).astype(np.float32)


def _box(I, y0, y1, x0, x1):
    H, W = I.shape[0] - 1, I.shape[1] - 1
    y0, y1, x0, x1 = (np.clip(v, 0, lim) for v, lim in ((y0, H), (y1, H), (x0, W), (x1, W)))
    return I[y1, x1].astype(np.int64) - I[y0, x1] - I[y1, x0] + I[y0, x0]


def describe(I, kps):
    """U-SURF, 64-d: 20 x 20 samples spaced s = 1.2 size / 9 around (x, y), Haar responses of size 2 round(s) on the integral
    image, Gaussian weights, (sum dx, sum |dx|, sum dy, sum |dy|) per 5 x 5 sub-region, L2-normalised.  (N, 64) fp32 and the
    descriptors' squared norms (fp32, sequential fused multiply-add chain)."""
    n = len(kps)
    if n == 0:
        return np.zeros((0, 64), np.float32), np.zeros((0,), np.float32)
    x, y, size = kps[:, 0:1, None], kps[:, 1:2, None], kps[:, 2:3, None]
    s = size * F(1.2) / F(9)
    u = np.arange(20, dtype=np.float32) - F(9.5)
    px = np.rint(x + u[None, None, :] * s).astype(np.int64)          # (n, 1, 20): column u
    py = np.rint(y + u[None, :, None] * s).astype(np.int64)          # (n, 20, 1): row v
    px, py = np.broadcast_to(px, (n, 20, 20)), np.broadcast_to(py, (n, 20, 20))
    hs = np.maximum(1, np.rint(s).astype(np.int64))
    dx = (_box(I, py - hs, py + hs, px, px + hs) - _box(I, py - hs, py + hs, px - hs, px)).astype(np.float32)
    dy = (_box(I, py, py + hs, px - hs, px + hs) - _box(I, py - hs, py, px - hs, px + hs)).astype(np.float32)
    g = gauss_table()[None]
    dx, dy = g * dx, g * dy
    comp = np.zeros((n, 4, 4, 4), np.float32)
    for vv in range(5):
        for uu in range(5):
            a, b = dx[:, vv::5, uu::5], dy[:, vv::5, uu::5]
            comp[..., 0] += a
            comp[..., 1] += np.abs(a)
            comp[..., 2] += b
            comp[..., 3] += np.abs(b)
    comp = comp.reshape(n, 64)
    ss = np.zeros(n, np.float32)
    for c in range(64):
        ss = ss + comp[:, c] * comp[:, c]
    nrm = np.sqrt(ss)
    desc = np.where(nrm[:, None] > 0, comp / np.where(nrm > 0, nrm, F(1))[:, None], F(0)).astype(np.float32)
    return desc, fma_chain_sq(desc)


def fma_chain_sq(d):
    acc = np.zeros(len(d), np.float32)
    for k in range(d.shape[1]):
        acc = (d[:, k].astype(np.float64) * d[:, k] + acc).astype(np.float32)
    return acc


# ---------------------------------------------------------------- step 4
def match(d1, n1, d2, n2):
    """2-NN of every query (view 1) over the train set (view 2) by d^2 = |a|^2 + |b|^2 - 2 a.b (fp32), ties to the lower index; the
    ratio test d1^2 < 0.49 d2^2.  (M, 2) int32 [query, train] in query order."""
    if len(d1) == 0 or len(d2) < 2:
        return np.zeros((0, 2), np.int32)
    dot = (d1.astype(np.float64) @ d2.astype(np.float64).T).astype(np.float32)
    d = (n1[:, None] + n2[None, :]) - F(2) * dot
    order = np.argsort(d, axis=1, kind="stable")[:, :2]
    r = np.arange(len(d1))
    best, second = d[r, order[:, 0]], d[r, order[:, 1]]
    good = best < F(0.49) * second
    return np.stack([r[good], order[good, 0]], -1).astype(np.int32)


# ---------------------------------------------------------------- step 5
def _mix(x):
    x = np.asarray(x, dtype=np.uint32)
    x = x ^ (x >> np.uint32(16))
    x = x * np.uint32(0x7FEB352D)
    x = x ^ (x >> np.uint32(15))
    x = x * np.uint32(0x846CA68B)
    return x ^ (x >> np.uint32(16))


def hash4(seed, pair, hyp, draw):
    with np.errstate(over="ignore"):
        h = _mix(np.uint32(seed & 0xFFFFFFFF))
        h = _mix(h ^ np.uint32(pair & 0xFFFFFFFF))
        h = _mix(h ^ np.asarray(hyp, dtype=np.uint32))
        return _mix(h ^ np.asarray(draw, dtype=np.uint32))


MAX_DRAWS = 16


def sample(seed, pair, n_hyp, M):
    """(n_hyp, 4) int64 sample indices, -1 where fewer than 4 distinct matches came out of MAX_DRAWS draws."""
    idx = np.full((n_hyp, 4), -1, np.int64)
    cnt = np.zeros(n_hyp, np.int64)
    h = np.arange(n_hyp, dtype=np.uint32)
    for c in range(MAX_DRAWS):
        v = (hash4(seed, pair, h, c) % np.uint32(max(M, 1))).astype(np.int64)
        fresh = (cnt < 4) & ~(idx == v[:, None]).any(1)
        idx[fresh, np.minimum(cnt[fresh], 3)] = v[fresh]
        cnt += fresh
    idx[cnt < 4] = -1
    return idx


def _degenerate(p):
    """p: (n, 4, 2) fp64.  Collinear triples (OpenCV's test: |cross| <= FLT_EPSILON (|dx1| + |dy1| + |dx2| + |dy2|))."""
    bad = np.zeros(len(p), bool)
    for i, j, k in ((0, 1, 2), (0, 1, 3), (0, 2, 3), (1, 2, 3)):
        dx1, dy1 = p[:, j, 0] - p[:, i, 0], p[:, j, 1] - p[:, i, 1]
        dx2, dy2 = p[:, k, 0] - p[:, i, 0], p[:, k, 1] - p[:, i, 1]
        bad |= np.abs(dx2 * dy1 - dy2 * dx1) <= FLT_EPS * (np.abs(dx1) + np.abs(dy1) + np.abs(dx2) + np.abs(dy2))
    return bad


def _orient(p, i, j, k):
    return (p[:, j, 0] - p[:, i, 0]) * (p[:, k, 1] - p[:, i, 1]) - (p[:, j, 1] - p[:, i, 1]) * (p[:, k, 0] - p[:, i, 0])


def subset_ok(src, dst):
    ok = ~_degenerate(src) & ~_degenerate(dst)
    neg = np.zeros(len(src), np.int64)
    for t in ((0, 1, 2), (1, 2, 3), (0, 2, 3), (0, 1, 3)):
        neg += (_orient(src, *t) * _orient(dst, *t)) < 0
    return ok & ((neg == 0) | (neg == 4))


def _hartley(p):
    cx = ((p[:, 0, 0] + p[:, 1, 0]) + p[:, 2, 0] + p[:, 3, 0]) / 4.0
    cy = ((p[:, 0, 1] + p[:, 1, 1]) + p[:, 2, 1] + p[:, 3, 1]) / 4.0
    md = np.zeros(len(p))
    for i in range(4):
        md = md + np.sqrt((p[:, i, 0] - cx) * (p[:, i, 0] - cx) + (p[:, i, 1] - cy) * (p[:, i, 1] - cy))
    md = md / 4.0
    ok = md > 0
    sc = np.sqrt(2.0) / np.where(ok, md, 1.0)
    return cx, cy, sc, ok


def _dlt4(sx, sy, dx, dy):
    """Gaussian elimination with partial pivoting on the 8 x 9 system (h33 = 1), fp64, vectorised over the leading axis."""
    n = len(sx)
    A = np.zeros((n, 8, 9))
    for i in range(4):
        x, y, u, v = sx[:, i], sy[:, i], dx[:, i], dy[:, i]
        A[:, 2 * i] = np.stack([x, y, np.ones(n), 0 * x, 0 * x, 0 * x, -x * u, -y * u, u], -1)
        A[:, 2 * i + 1] = np.stack([0 * x, 0 * x, 0 * x, x, y, np.ones(n), -x * v, -y * v, v], -1)
    ok = np.ones(n, bool)
    r = np.arange(n)
    for c in range(8):
        piv = c + np.argmax(np.abs(A[:, c:, c]), axis=1)
        ok &= ~(np.abs(A[r, piv, c]) < 1e-300)
        rows_c, rows_p = A[r, c].copy(), A[r, piv].copy()
        A[r, c], A[r, piv] = rows_p, rows_c
        inv = 1.0 / np.where(ok, A[:, c, c], 1.0)
        for rr in range(c + 1, 8):
            f = A[:, rr, c] * inv
            A[:, rr, c:] = A[:, rr, c:] - f[:, None] * A[:, c, c:]
    h = np.zeros((n, 9))
    for c in range(7, -1, -1):
        s = A[:, c, 8].copy()
        for k in range(c + 1, 8):
            s = s - A[:, c, k] * h[:, k]
        h[:, c] = s / np.where(ok, A[:, c, c], 1.0)
    h[:, 8] = 1.0
    return h, ok


def _mul3(a, b):
    """(n, 9) x (n, 9) row-major 3 x 3 products, each entry summed left to right."""
    out = np.empty_like(a)
    for i in range(3):
        for j in range(3):
            out[:, 3 * i + j] = a[:, 3 * i] * b[:, j] + a[:, 3 * i + 1] * b[:, 3 + j] + a[:, 3 * i + 2] * b[:, 6 + j]
    return out


def hypotheses(src4, dst4):
    """src4 / dst4: (n, 4, 2) fp32 sample points.  -> (n, 9) fp64 H (h33 = 1), ok mask."""
    src, dst = src4.astype(np.float64), dst4.astype(np.float64)
    ok = subset_ok(src, dst)
    c1x, c1y, s1, ok1 = _hartley(src)
    c2x, c2y, s2, ok2 = _hartley(dst)
    hn, ok3 = _dlt4((src[..., 0] - c1x[:, None]) * s1[:, None], (src[..., 1] - c1y[:, None]) * s1[:, None],
                    (dst[..., 0] - c2x[:, None]) * s2[:, None], (dst[..., 1] - c2y[:, None]) * s2[:, None])
    z = np.zeros_like(s1)
    o = np.ones_like(s1)
    T1 = np.stack([s1, z, -s1 * c1x, z, s1, -s1 * c1y, z, z, o], -1)
    T2i = np.stack([1.0 / s2, z, c2x, z, 1.0 / s2, c2y, z, z, o], -1)
    Hm = _mul3(T2i, _mul3(hn, T1))
    ok4 = np.abs(Hm[:, 8]) > 1e-12
    Hm = Hm / np.where(ok4, Hm[:, 8], 1.0)[:, None]
    return Hm, ok & ok1 & ok2 & ok3 & ok4


def reproj_err(Hf, p1, p2):
    """Hf: (n, 9) fp32; p1, p2: (M, 2) fp32 -> (n, M) fp32 |H p1 - p2|^2 (one-directional, fp32 in the kernel's order)."""
    x, y = p1[None, :, 0], p1[None, :, 1]
    h = [Hf[:, k:k + 1] for k in range(9)]
    u = h[0] * x + h[1] * y + h[2]
    v = h[3] * x + h[4] * y + h[5]
    w = h[6] * x + h[7] * y + h[8]
    ex = u / w - p2[None, :, 0]
    ey = v / w - p2[None, :, 1]
    return ex * ex + ey * ey


def ransac(p1, p2, seed=0, pair=0, n_hyp=2048):
    """Best hypothesis: most inliers (err <= 25), then the lower sum of min(err, 25), then the lower index.
    -> (best index or -1, H fp32 (9,), inlier count, per-hypothesis counts, error sums)."""
    M = len(p1)
    cnt = np.full(n_hyp, -1, np.int64)
    esum = np.zeros(n_hyp, np.float32)
    if M < 4:
        return -1, None, 0, cnt, esum
    idx = sample(seed, pair, n_hyp, M)
    have = (idx >= 0).all(1)
    safe = np.where(idx >= 0, idx, 0)
    Hd, ok = hypotheses(p1[safe], p2[safe])
    ok &= have
    Hf = Hd.astype(np.float32)
    with np.errstate(all="ignore"):
        e = reproj_err(Hf, p1, p2)
    inl = e <= F(25)
    tr = np.fmin(e, F(25))
    s = np.cumsum(tr, axis=1, dtype=np.float32)[:, -1]
    cnt = np.where(ok, inl.sum(1), -1)
    esum = np.where(ok, s, F(0)).astype(np.float32)
    if not ok.any():
        return -1, None, 0, cnt, esum
    order = np.lexsort((np.arange(n_hyp), esum.astype(np.float64), -cnt))
    b = int(order[0])
    return b, Hf[b], int(cnt[b]), cnt, esum


# ---------------------------------------------------------------- step 6
def _solve(A, b):
    """Gaussian elimination with partial pivoting (the torch refit's _solve, fp64)."""
    A = np.concatenate([A, b[:, None]], 1).astype(np.float64)
    n = A.shape[0]
    for c in range(n):
        p = c + int(np.argmax(np.abs(A[c:, c])))
        A[[c, p]] = A[[p, c]]
        A[c + 1:] -= (A[c + 1:, c] / A[c, c])[:, None] * A[c]
    x = np.zeros(n)
    for c in range(n - 1, -1, -1):
        x[c] = (A[c, n] - A[c, c + 1:n] @ x[c + 1:]) / A[c, c]
    return x


def _norm(p):
    c = p.mean(0)
    s = np.sqrt(2.0) / np.sqrt(((p - c) ** 2).sum(1)).mean()
    return c, s


def _resid_jac(h, a, b):
    x, y = a[:, 0], a[:, 1]
    u = h[0] * x + h[1] * y + h[2]
    v = h[3] * x + h[4] * y + h[5]
    w = h[6] * x + h[7] * y + 1.0
    r = np.concatenate([u / w - b[:, 0], v / w - b[:, 1]])
    z, o = np.zeros_like(x), np.ones_like(x)
    ju = np.stack([x, y, o, z, z, z, -x * u / w, -y * u / w], -1) / w[:, None]
    jv = np.stack([z, z, z, x, y, o, -x * v / w, -y * v / w], -1) / w[:, None]
    return r, np.concatenate([ju, jv])


def refit(p1, p2, iters=10):
    """Normalised least-squares DLT (h33 = 1) over the inliers, then Levenberg-Marquardt on the reprojection error (in the
    normalised frames).  -> (3, 3) fp64 with H[2, 2] = 1."""
    p1, p2 = p1.astype(np.float64), p2.astype(np.float64)
    c1, s1 = _norm(p1)
    c2, s2 = _norm(p2)
    a, b = (p1 - c1) * s1, (p2 - c2) * s2
    x, y, u, v = a[:, 0], a[:, 1], b[:, 0], b[:, 1]
    z, o = np.zeros_like(x), np.ones_like(x)
    A = np.concatenate([np.stack([x, y, o, z, z, z, -x * u, -y * u], -1), np.stack([z, z, z, x, y, o, -x * v, -y * v], -1)])
    rhs = np.concatenate([u, v])
    h = _solve(A.T @ A, A.T @ rhs)
    r, J = _resid_jac(h, a, b)
    cost, lam = r @ r, 1e-3
    for _ in range(iters):
        JtJ = J.T @ J
        g = J.T @ r
        step = _solve(JtJ + lam * np.diag(np.diag(JtJ)), -g)
        hn = h + step
        rn, Jn = _resid_jac(hn, a, b)
        cn = rn @ rn
        if cn < cost:
            h, r, J, cost, lam = hn, rn, Jn, cn, lam * 0.1
        else:
            lam = lam * 10.0
    Hn = np.append(h, 1.0).reshape(3, 3)
    T1 = np.array([[s1, 0, -s1 * c1[0]], [0, s1, -s1 * c1[1]], [0, 0, 1.0]])
    T2i = np.array([[1 / s2, 0, c2[0]], [0, 1 / s2, c2[1]], [0, 0, 1.0]])
    Hm = T2i @ Hn @ T1
    return Hm / Hm[2, 2]


# ---------------------------------------------------------------- the whole pipeline
def estimate(img1, img2, max_keypoints=4096, hypotheses_n=2048, seed=0, pair=0):
    """One pair of (3, H, W) images (uint8, or float in [0, 1]).  -> dict with H (3, 3) fp64 or None, and every stage."""
    out = {}
    for v, img in (("1", img1), ("2", img2)):
        I = integral(grey(img))
        dets = hessian_layers(I)
        kps = select(detect(I, dets), max_keypoints)
        d, n = describe(I, kps)
        out.update({"I" + v: I, "dets" + v: dets, "kps" + v: kps, "desc" + v: d, "nrm" + v: n})
    m = match(out["desc1"], out["nrm1"], out["desc2"], out["nrm2"])
    out["matches"] = m
    p1, p2 = out["kps1"][m[:, 0], :2], out["kps2"][m[:, 1], :2]
    best, Hb, cnt, counts, esum = ransac(p1, p2, seed, pair, hypotheses_n)
    out.update(best=best, H_ransac=Hb, inliers=cnt, counts=counts, esum=esum)
    if best < 0 or cnt < 4:
        out["H"] = None
        out["inlier_mask"] = np.zeros(len(m), bool)
        return out
    with np.errstate(all="ignore"):
        inl = reproj_err(Hb[None], p1, p2)[0] <= F(25)
    out["inlier_mask"] = inl
    out["H"] = refit(p1[inl], p2[inl])
    return out


def corner_error(H, H_true, height, width):
    """Max displacement (px) of the four image corners between H and H_true."""
    c = np.array([[0, 0, 1], [width - 1, 0, 1], [width - 1, height - 1, 1], [0, height - 1, 1]], dtype=np.float64)
    a = c @ np.asarray(H, np.float64).T
    b = c @ np.asarray(H_true, np.float64).T
    return float(np.max(np.hypot(*(a[:, :2] / a[:, 2:] - b[:, :2] / b[:, 2:]).T)))

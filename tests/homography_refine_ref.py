"""numpy fp64 restatement of the photometric homography refiner (include/hesic_homography_refine.h, csrc/homography_refine.hip):
the grey pyramid, the normal equations of a candidate, the Levenberg-Marquardt walk with its level transitions and the "never worse" rule,
operation for operation in the kernels' order (no fused multiply-add on either side), plus the textures and known warps the tests use.

Notation: ``H`` maps a pixel of x1 to a pixel of x2 (``h_matrix`` of ``HSIC.forward``); ``A = inverse(H)`` scaled to ``a22 = 1`` maps a
destination pixel p = (x, y) to its source position w(p) = (X/Z, Y/Z); pixel coordinates follow ``align_corners=True``."""
import numpy as np

NSUMS = 46                      # 36 upper-triangle sums of w J^T J, 8 of w J^T r, sum w r^2, valid count
MIN_SIDE = 16                   # levels are built while min(H_l, W_l) >= MIN_SIDE
LAMBDA0, LAMBDA_MIN, LAMBDA_MAX = 1e-3, 1e-9, 1e6


# ---------------------------------------------------------------------------------------------------------------- small fp64 pieces
def mat3(a, b):
    """a @ b for 3x3, every entry (a0 b0 + a1 b1) + a2 b2."""
    o = np.empty((3, 3))
    for i in range(3):
        for j in range(3):
            o[i, j] = (a[i, 0] * b[0, j] + a[i, 1] * b[1, j]) + a[i, 2] * b[2, j]
    return o


def inv3(m):
    """The adjugate inverse of csrc/dlt.h (no pivoting; a singular matrix gives non-finite entries)."""
    m = np.asarray(m, np.float64).reshape(9)
    c0, c1, c2 = m[4] * m[8] - m[5] * m[7], m[5] * m[6] - m[3] * m[8], m[3] * m[7] - m[4] * m[6]
    with np.errstate(all="ignore"):
        d = 1.0 / ((m[0] * c0 + m[1] * c1) + m[2] * c2)
        o = np.array([c0 * d, (m[2] * m[7] - m[1] * m[8]) * d, (m[1] * m[5] - m[2] * m[4]) * d,
                      c1 * d, (m[0] * m[8] - m[2] * m[6]) * d, (m[2] * m[3] - m[0] * m[5]) * d,
                      c2 * d, (m[1] * m[6] - m[0] * m[7]) * d, (m[0] * m[4] - m[1] * m[3]) * d])
    return o.reshape(3, 3)


def norm22(m):
    with np.errstate(all="ignore"):
        return m / m[2, 2]


def level_T(l):
    s = float(2 ** l)
    o = (s - 1.0) / 2.0
    return np.array([[s, 0, o], [0, s, o], [0, 0, 1.0]]), np.array([[1 / s, 0, -o / s], [0, 1 / s, -o / s], [0, 0, 1.0]])


def to_level(A, src, dst):
    """A of level ``src`` as level ``dst``'s: through level 0, (T^-1 (T_src A T_src^-1)) T, renormalised to a22 = 1."""
    if src == dst:
        return A.copy()
    Ts, Tsi = level_T(src)
    Td, Tdi = level_T(dst)
    with np.errstate(all="ignore"):
        A0 = mat3(mat3(Ts, A), Tsi)
        return norm22(mat3(mat3(Tdi, A0), Td))


def solve8(M, rhs):
    """Gaussian elimination with partial pivoting on the augmented 8x9 system (csrc: solve8); None for a singular or non-finite solve."""
    A = np.concatenate([M, rhs[:, None]], 1).astype(np.float64)
    if not np.isfinite(A).all():
        return None
    with np.errstate(all="ignore"):
        for c in range(8):
            piv = c
            for r in range(c + 1, 8):
                if abs(A[r, c]) > abs(A[piv, c]):
                    piv = r
            if not abs(A[piv, c]) >= 1e-300:
                return None
            if piv != c:
                A[[c, piv]] = A[[piv, c]]
            inv = 1.0 / A[c, c]
            for r in range(c + 1, 8):
                f = A[r, c] * inv
                A[r, c:] = A[r, c:] - f * A[c, c:]
        x = np.zeros(8)
        for c in range(7, -1, -1):
            s = A[c, 8]
            for k in range(c + 1, 8):
                s = s - A[c, k] * x[k]
            x[c] = s / A[c, c]
    return x if np.isfinite(x).all() else None


def dlt4(src, dst):
    """dst ~ H src for four points (rows [x y 1 0 0 0 -xu -yu | u], [0 0 0 x y 1 -xv -yv | v]), h22 = 1."""
    M, b = np.zeros((8, 8)), np.zeros(8)
    for i, ((x, y), (u, v)) in enumerate(zip(src, dst)):
        M[2 * i] = [x, y, 1, 0, 0, 0, -x * u, -y * u]
        M[2 * i + 1] = [0, 0, 0, x, y, 1, -x * v, -y * v]
        b[2 * i], b[2 * i + 1] = u, v
    return np.append(np.linalg.solve(M, b), 1.0).reshape(3, 3)


# ------------------------------------------------------------------------------------------------------------------------- pyramid
def level_sizes(H, W, levels):
    """[(H_l, W_l)] of the levels actually used: min(levels, available), level l + 1 = (H_l // 2, W_l // 2) while min(H_l, W_l) >= 16."""
    out = []
    while len(out) < levels and min(H, W) >= MIN_SIDE:
        out.append((H, W))
        H, W = H // 2, W // 2
    return out


def grey(x):
    """(C, H, W) fp32, C in {1, 3} -> (H, W) fp32: the unweighted channel mean in fp64, rounded once."""
    x = np.asarray(x, np.float32).astype(np.float64)
    if x.shape[0] == 1:
        return x[0].astype(np.float32)
    return (((x[0] + x[1]) + x[2]) / 3.0).astype(np.float32)


def pyramid(x, levels):
    """(C, H, W) -> [level 0, level 1, ...] fp32; level l + 1 is the 2 x 2 mean of level l in fp64, rounded once; odd tails dropped."""
    g = grey(x)
    out = []
    for (h, w) in level_sizes(g.shape[0], g.shape[1], levels):
        if out:
            p = out[-1].astype(np.float64)
            g = ((((p[0:2 * h:2, 0:2 * w:2] + p[0:2 * h:2, 1:2 * w:2]) + p[1:2 * h:2, 0:2 * w:2]) + p[1:2 * h:2, 1:2 * w:2]) * 0.25).astype(np.float32)
        out.append(g)
    return out


# ---------------------------------------------------------------------------------------------------------------- normal equations
def tri_index(i, j):
    return i * 8 - i * (i - 1) // 2 + (j - i)


def normal_equations(I1, I2, A, huber=None, with_abs=False):
    """The 46 sums of candidate ``A`` (3x3, destination -> source) on one level: I1, I2 (H, W) fp32.  Returns ``sums`` (46,) and, with
    ``with_abs``, also the sums of the absolute per-pixel terms."""
    H, W = I1.shape
    I1d, I2d = I1.astype(np.float64), I2.astype(np.float64)
    A = np.asarray(A, np.float64).reshape(9)
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)
    with np.errstate(all="ignore"):
        X = (A[0] * x + A[1] * y) + A[2]
        Y = (A[3] * x + A[4] * y) + A[5]
        Z = (A[6] * x + A[7] * y) + A[8]
        iz = 1.0 / Z                                       # the one division by Z
        u, v_ = X * iz, Y * iz
        fx0, fy0 = np.floor(u), np.floor(v_)
        valid = (fx0 >= 0) & (fy0 >= 0) & (fx0 <= W - 2) & (fy0 <= H - 2)        # NaN compares false
    sums = np.zeros(NSUMS)
    sabs = np.zeros(NSUMS)
    if valid.any():
        x, y, u, v_, iz = x[valid], y[valid], u[valid], v_[valid], iz[valid]
        x0, y0 = fx0[valid].astype(np.int64), fy0[valid].astype(np.int64)
        fx, fy = u - fx0[valid], v_ - fy0[valid]
        a, b, c, d = I1d[y0, x0], I1d[y0, x0 + 1], I1d[y0 + 1, x0], I1d[y0 + 1, x0 + 1]
        gx = (b - a) * (1.0 - fy) + (d - c) * fy
        gy = (c - a) * (1.0 - fx) + (d - b) * fx
        val = (a * (1.0 - fx) + b * fx) * (1.0 - fy) + (c * (1.0 - fx) + d * fx) * fy
        r = val - I2d[valid]
        t0, t1 = gx * iz, gy * iz
        t2 = -(gx * u + gy * v_) * iz
        J = [t0 * x, t0 * y, t0, t1 * x, t1 * y, t1, t2 * x, t2 * y]
        if huber is not None:
            with np.errstate(all="ignore"):
                w = np.minimum(1.0, float(huber) / np.abs(r))
        else:
            w = np.ones_like(r)
        wJ = [w * j for j in J]
        for i in range(8):
            for j in range(i, 8):
                t = wJ[i] * J[j]
                sums[tri_index(i, j)], sabs[tri_index(i, j)] = t.sum(), np.abs(t).sum()
            t = wJ[i] * r
            sums[36 + i], sabs[36 + i] = t.sum(), np.abs(t).sum()
        t = (w * r) * r
        sums[44], sabs[44] = t.sum(), np.abs(t).sum()
        sums[45] = sabs[45] = float(valid.sum())
    return (sums, sabs) if with_abs else sums


def _cost(sums):
    return sums[44] / sums[45] if sums[45] > 0 else 0.0


def lm_step(kept, lam):
    """delta of (J^T J + lam diag(J^T J)) delta = -J^T r from the kept sums, or None."""
    M = np.zeros((8, 8))
    for i in range(8):
        for j in range(i, 8):
            M[i, j] = M[j, i] = kept[tri_index(i, j)]
    for i in range(8):
        M[i, i] = M[i, i] + lam * M[i, i]
    return solve8(M, -kept[36:44])


# -------------------------------------------------------------------------------------------------------------------- the whole call
def refine(x1, x2, h, levels=3, iters=10, huber=None, min_overlap=0.25, trace=None):
    """One pair: x1, x2 (C, H, W) fp32, ``h`` (3, 3) fp32 -> (h_refined fp32 (3, 3), info dict).  ``trace``: a list that receives every
    accepted cost as (level, cost)."""
    h = np.asarray(h, np.float32)
    p1, p2 = pyramid(x1, levels), pyramid(x2, levels)
    L = len(p1)
    flat = [float(p.max()) == float(p.min()) for p in p2]
    A0 = norm22(inv3(h.astype(np.float64)))
    accepted = rejected = 0
    valid_share = 0.0
    cost_first = None
    if L > 1:
        cost_first = _cost(normal_equations(p1[0], p2[0], A0, huber))
    best = to_level(A0, 0, L - 1)
    cost_best, alive = 0.0, False
    for l in range(L - 1, -1, -1):
        I1, I2 = p1[l], p2[l]
        area = float(I1.shape[0] * I1.shape[1])
        cand, lam, first, alive, kept = best.copy(), LAMBDA0, True, True, None
        for _ in range(iters + 1):
            if not alive:
                break
            s = normal_equations(I1, I2, cand, huber)
            cost = _cost(s)
            if first:
                first = False
                if l == 0 and cost_first is None:
                    cost_first = cost
                if s[45] == 0 or flat[l]:                       # nothing to align, or (a view without contrast) nothing to align TO
                    alive = False
                    break
                ok = True
            else:
                ok = cost < cost_best and s[45] >= min_overlap * area
                if ok:
                    accepted += 1
                else:
                    rejected += 1
            if ok:
                best, kept, cost_best, valid_share = cand.copy(), s, cost, s[45] / area
                lam = max(lam / 10.0, LAMBDA_MIN)
                if trace is not None:
                    trace.append((l, cost))
            else:
                lam = min(lam * 10.0, LAMBDA_MAX)
            delta = lm_step(kept, lam)
            if delta is None:
                rejected += 1
                lam = min(lam * 10.0, LAMBDA_MAX)
                cand = best.copy()
            else:
                cand = best.copy()
                cand.reshape(9)[:8] += delta
        if l > 0:
            best = to_level(best, l, l - 1)
    refined = bool(alive and accepted > 0 and cost_best < cost_first)
    out = h.copy()
    if refined:
        with np.errstate(all="ignore"):
            hr = norm22(inv3(best)).astype(np.float32)
        if np.isfinite(hr).all():
            out = hr
        else:
            refined = False
    info = {"cost_before": cost_first, "cost_after": cost_best if refined else cost_first, "accepted": accepted, "rejected": rejected,
            "valid_share": valid_share, "levels_used": L, "refined": refined}
    return out, info


# ----------------------------------------------------------------------------------------------------------- textures, known warps
def texture(seed, H, W, sigma=2.0):
    """default_rng(seed).standard_normal((H, W)), low-passed in the Fourier domain by exp(-2 (pi sigma)^2 (fx^2 + fy^2)), min-max scaled to
    [0, 1]; fp32."""
    g = np.random.default_rng(seed).standard_normal((H, W))
    fy, fx = np.fft.fftfreq(H)[:, None], np.fft.fftfreq(W)[None, :]
    t = np.fft.ifft2(np.fft.fft2(g) * np.exp(-2.0 * (np.pi * sigma) ** 2 * (fx * fx + fy * fy))).real
    return ((t - t.min()) / (t.max() - t.min())).astype(np.float32)


def corners_of(H, W):
    return np.array([[0, 0], [W - 1, 0], [W - 1, H - 1], [0, H - 1]], np.float64)


def known_warp(seed, H, W, rho):
    """The DLT of the four image corners displaced by default_rng(100 + seed).uniform(-rho, rho, (4, 2)): x1 pixel -> x2 pixel."""
    c = corners_of(H, W)
    return dlt4(c, c + np.random.default_rng(100 + seed).uniform(-rho, rho, (4, 2)))


def warp_image(I1, Hm):
    """x2(p) = bilinear(I1, H^-1 p) where all four taps lie inside I1, zero elsewhere; fp32."""
    H, W = I1.shape
    A = np.linalg.inv(np.asarray(Hm, np.float64))
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)
    Z = A[2, 0] * x + A[2, 1] * y + A[2, 2]
    u, v = (A[0, 0] * x + A[0, 1] * y + A[0, 2]) / Z, (A[1, 0] * x + A[1, 1] * y + A[1, 2]) / Z
    x0, y0 = np.floor(u), np.floor(v)
    valid = (x0 >= 0) & (y0 >= 0) & (x0 <= W - 2) & (y0 <= H - 2)
    xi, yi = np.where(valid, x0, 0).astype(np.int64), np.where(valid, y0, 0).astype(np.int64)
    fx, fy = u - x0, v - y0
    I = I1.astype(np.float64)
    val = (I[yi, xi] * (1 - fx) + I[yi, xi + 1] * fx) * (1 - fy) + (I[yi + 1, xi] * (1 - fx) + I[yi + 1, xi + 1] * fx) * fy
    return np.where(valid, val, 0.0).astype(np.float32)


def corner_points(Hm, H, W):
    c = corners_of(H, W)
    p = np.concatenate([c, np.ones((4, 1))], 1) @ np.asarray(Hm, np.float64).T
    return p[:, :2] / p[:, 2:]


def corner_error(Ha, Hb, H, W):
    """Mean over the four image corners of the distance between their images under the two matrices, in pixels."""
    return float(np.sqrt(((corner_points(Ha, H, W) - corner_points(Hb, H, W)) ** 2).sum(-1)).mean())


def known_case(seed, H=96, W=128, sigma=2.0, rho=8.0):
    """(x1 (1,H,W), x2 (1,H,W), H_true) of a seed."""
    t = texture(seed, H, W, sigma)
    Ht = known_warp(seed, H, W, rho)
    return t[None], warp_image(t, Ht)[None], Ht


def huber_case(seed, H=96, W=128, sigma=2.0, rho=8.0):
    """``known_case`` with rows 30 - 54 and columns 40 - 72 of x2 replaced by another texture."""
    x1, x2, Ht = known_case(seed, H, W, sigma, rho)
    x2 = x2.copy()
    x2[0, 30:55, 40:73] = texture(1000 + seed, H, W, sigma)[30:55, 40:73]
    return x1, x2, Ht

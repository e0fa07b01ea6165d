"""NumPy restatement of the oriented and extended SURF of ``hesic_amd.stereo_h`` (orient_kernel, describe_ex_kernel<64 / 128> and
match_kernel<128> of ``hesic_amd/csrc/stereo_h.hip``), for the tests only.  It builds on ``stereo_h_ref`` (the upright 64-d
pipeline) and follows the kernels operation by operation: fp32 where they use fp32, the same rounding calls, summation orders and
tie-breaks.  The matcher is ``stereo_h_ref.match``, already generic in the descriptor width.

The product never imports this module.
"""
from __future__ import annotations

import math

import numpy as np

import stereo_h_ref as R

F = np.float32

# OpenCV's fastAtan2 coefficients, each times (float)(180 / pi) in fp32
_R2D = F(180.0 / np.pi)
P1, P3, P5, P7 = (F(v) * _R2D for v in (0.9997878412794807, -0.3258083974640975, 0.1555786518463281, -0.04432655554792128))
_EPS = F(np.finfo(np.float64).eps)


def ori_table():
    """The 109 orientation samples: (i, j) int64 in row-major order (i outer) with i^2 + j^2 < 36, and their fp32 weights
    G[i + 6] * G[j + 6] (13-tap Gaussian, sigma 2.5, normalised in fp64 by a sequential sum, rounded to fp32)."""
    g = [math.exp(-float((k - 6) * (k - 6)) / (2.0 * 2.5 * 2.5)) for k in range(13)]
    total = 0.0
    for v in g:
        total += v
    G = np.array([v / total for v in g]).astype(np.float32)
    ij = np.array([(i, j) for i in range(-6, 7) for j in range(-6, 7) if i * i + j * j < 36], dtype=np.int64)
    return ij[:, 0], ij[:, 1], G[ij[:, 0] + 6] * G[ij[:, 1] + 6]


def fast_atan2(y, x):
    """Degrees in [0, 360] of (x, y), OpenCV's fastAtan2 with every step in fp32."""
    y, x = np.asarray(y, np.float32), np.asarray(x, np.float32)
    ax, ay = np.abs(x), np.abs(y)
    ge = ax >= ay
    with np.errstate(all="ignore"):
        c = np.where(ge, ay / (ax + _EPS), ax / (ay + _EPS)).astype(np.float32)
    c2 = c * c
    p = (((P7 * c2 + P5) * c2 + P3) * c2 + P1) * c
    a = np.where(ge, p, F(90) - p)
    a = np.where(x < 0, F(180) - a, a)
    return np.where(y < 0, F(360) - a, a).astype(np.float32)


def orient(I, kps, return_fallbacks=False):
    """(n, 2) fp32 [cos, sin] of each keypoint's dominant direction: Haar responses of size g = 2 rint(2 s) at the 109 samples
    (boxes that leave the image skipped), weighted, their angles from fast_atan2; for w0 = 0, 5, ..., 355 the weighted responses
    with |rint(angle) - w0| < 30 or > 330 summed in sample order; the first window of largest sumx^2 + sumy^2 (> 0) gives the
    direction, normalised.  (1, 0) where no window is non-zero; ``return_fallbacks`` also returns how many keypoints got it."""
    n = len(kps)
    H, W = I.shape[0] - 1, I.shape[1] - 1
    if n == 0:
        out = np.zeros((0, 2), np.float32)
        return (out, 0) if return_fallbacks else out
    ti, tj, tw = ori_table()
    x, y = kps[:, 0:1], kps[:, 1:2]
    s = kps[:, 2:3] * F(1.2) / F(9)
    g = 2 * np.rint(F(2) * s).astype(np.int64)
    h = g // 2
    half = (g - 1).astype(np.float32) / F(2)
    x0 = np.rint(x + ti[None].astype(np.float32) * s - half).astype(np.int64)
    y0 = np.rint(y + tj[None].astype(np.float32) * s - half).astype(np.int64)
    ok = (x0 >= 0) & (y0 >= 0) & (x0 + g <= W) & (y0 + g <= H)
    gx = R._box(I, y0, y0 + g, x0 + h, x0 + g) - R._box(I, y0, y0 + g, x0, x0 + h)
    gy = R._box(I, y0 + h, y0 + g, x0, x0 + g) - R._box(I, y0, y0 + h, x0, x0 + g)
    X = np.where(ok, gx.astype(np.float32) * tw[None], F(0))
    Y = np.where(ok, gy.astype(np.float32) * tw[None], F(0))
    ang = np.rint(fast_atan2(Y, X)).astype(np.int64)
    w0 = 5 * np.arange(72)
    sx = np.zeros((n, 72), np.float32)
    sy = np.zeros((n, 72), np.float32)
    for q in range(len(tw)):
        d = np.abs(ang[:, q:q + 1] - w0[None])
        sel = ok[:, q:q + 1] & ((d < 30) | (d > 330))
        sx = np.where(sel, sx + X[:, q:q + 1], sx)
        sy = np.where(sel, sy + Y[:, q:q + 1], sy)
    mod = sx * sx + sy * sy
    best = np.argmax(mod, axis=1)                       # the first largest window
    r = np.arange(n)
    bx, by, bm = sx[r, best], sy[r, best], mod[r, best]
    fall = ~(bm > 0)
    with np.errstate(all="ignore"):
        nrm = np.sqrt(bx * bx + by * by)
        out = np.stack([np.where(fall, F(1), bx / nrm), np.where(fall, F(0), by / nrm)], -1).astype(np.float32)
    return (out, int(fall.sum())) if return_fallbacks else out


def describe_ex(I, kps, ori=None, dim=64):
    """SURF in the keypoint's frame: the 20 x 20 samples at kp + s R (u - 9.5, v - 9.5) (rint), describe()'s axis-aligned Haar
    responses there, rotated into the frame (dx' = c dx + s dy, dy' = -s dx + c dy), Gaussian-weighted; 64-d as describe(), or
    128-d with each sum split by the sign of the other response.  ``ori`` None: upright.  -> (n, dim) fp32 and squared norms."""
    n = len(kps)
    if n == 0:
        return np.zeros((0, dim), np.float32), np.zeros((0,), np.float32)
    x, y, size = kps[:, 0:1, None], kps[:, 1:2, None], kps[:, 2:3, None]
    if ori is None:
        c, sn = np.ones((n, 1, 1), np.float32), np.zeros((n, 1, 1), np.float32)
    else:
        c, sn = ori[:, 0:1, None].astype(np.float32), ori[:, 1:2, None].astype(np.float32)
    s = size * F(1.2) / F(9)
    fu = (np.arange(20, dtype=np.float32) - F(9.5))[None, None, :]      # column u
    fv = (np.arange(20, dtype=np.float32) - F(9.5))[None, :, None]      # row v
    px = np.rint(x + (fu * c - fv * sn) * s).astype(np.int64)
    py = np.rint(y + (fu * sn + fv * c) * s).astype(np.int64)
    hs = np.maximum(1, np.rint(s).astype(np.int64))
    dx = (R._box(I, py - hs, py + hs, px, px + hs) - R._box(I, py - hs, py + hs, px - hs, px)).astype(np.float32)
    dy = (R._box(I, py, py + hs, px - hs, px + hs) - R._box(I, py - hs, py, px - hs, px + hs)).astype(np.float32)
    rx = c * dx + sn * dy
    ry = -sn * dx + c * dy
    gw = R.gauss_table()[None]
    dx, dy = gw * rx, gw * ry
    per = dim // 16
    comp = np.zeros((n, 4, 4, per), np.float32)
    z = F(0)
    for vv in range(5):
        for uu in range(5):
            a, b = dx[:, vv::5, uu::5], dy[:, vv::5, uu::5]
            if dim == 64:
                terms = (a, np.abs(a), b, np.abs(b))
            else:
                bp, ap = b >= 0, a >= 0
                terms = (np.where(bp, a, z), np.where(bp, np.abs(a), z), np.where(bp, z, a), np.where(bp, z, np.abs(a)),
                         np.where(ap, b, z), np.where(ap, np.abs(b), z), np.where(ap, z, b), np.where(ap, z, np.abs(b)))
            for k, t in enumerate(terms):
                comp[..., k] += t
    comp = comp.reshape(n, dim)
    ss = np.zeros(n, np.float32)
    for k in range(dim):
        ss = ss + comp[:, k] * comp[:, k]
    nrm = np.sqrt(ss)
    desc = np.where(nrm[:, None] > 0, comp / np.where(nrm > 0, nrm, F(1))[:, None], F(0)).astype(np.float32)
    return desc, R.fma_chain_sq(desc)


def estimate(img1, img2, max_keypoints=4096, hypotheses_n=2048, seed=0, pair=0, upright=True, extended=False):
    """stereo_h_ref.estimate with the descriptor options of estimate_homography.  -> dict with H (3, 3) fp64 or None, every stage,
    ``ori1`` / ``ori2`` and ``fallbacks`` (keypoints left upright by orient) when not upright."""
    out = {"fallbacks": 0}
    dim = 128 if extended else 64
    for v, img in (("1", img1), ("2", img2)):
        I = R.integral(R.grey(img))
        dets = R.hessian_layers(I)
        kps = R.select(R.detect(I, dets), max_keypoints)
        ori = None
        if not upright:
            ori, nf = orient(I, kps, return_fallbacks=True)
            out["ori" + v] = ori
            out["fallbacks"] += nf
        d, n = R.describe(I, kps) if upright and not extended else describe_ex(I, kps, ori, dim)
        out.update({"I" + v: I, "dets" + v: dets, "kps" + v: kps, "desc" + v: d, "nrm" + v: n})
    m = R.match(out["desc1"], out["nrm1"], out["desc2"], out["nrm2"])
    out["matches"] = m
    p1, p2 = out["kps1"][m[:, 0], :2], out["kps2"][m[:, 1], :2]
    best, Hb, cnt, counts, esum = R.ransac(p1, p2, seed, pair, hypotheses_n)
    out.update(best=best, H_ransac=Hb, inliers=cnt, counts=counts, esum=esum)
    if best < 0 or cnt < 4:
        out["H"] = None
        out["inlier_mask"] = np.zeros(len(m), bool)
        return out
    with np.errstate(all="ignore"):
        inl = R.reproj_err(Hb[None], p1, p2)[0] <= F(25)
    out["inlier_mask"] = inl
    out["H"] = R.refit(p1[inl], p2[inl])
    return out

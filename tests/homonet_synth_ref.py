"""numpy restatement of ``hesic_homonet_synth_items`` (include/hesic_homonet_synth.h) BY DEFINITION: ``grey_a``, ``patch_a`` and ``corners``
are ``homonet_items_ref`` / ``homography_prep_ref`` on the item's crop, ``h`` is ``homography_train_ref.dlt_torch`` in fp64 on the absolute
corners, ``grey_b`` is the header's fp64 bilinear sum -- operation by operation, in the stated order, so that it can be asked for bits
from a GIVEN ``h`` -- and ``patch_b`` is sliced from it.  No GPU."""
import numpy as np
import torch

import homography_train_ref as HT
import homonet_items_ref as IR

NAMES = ("grey_a", "patch_a", "corners", "delta", "h", "grey_b", "patch_b")


def dlt(corners, delta):
    """(B, 9) fp64: ``dlt_torch(corners -> corners + delta)`` on the ABSOLUTE corners, h[8] = 1."""
    c = torch.from_numpy(np.asarray(corners, dtype=np.float64))
    d = torch.from_numpy(np.asarray(delta, dtype=np.float64)).reshape(-1, 4, 2)
    return HT.dlt_torch(c, c + d).reshape(-1, 9).numpy()


def corner_residual(h, corners, delta):
    """max |h applied to the four corners - (corners + delta)| per item, in fp64 numpy: (B,)."""
    h = np.asarray(h, dtype=np.float64).reshape(-1, 3, 3)
    c = np.asarray(corners, dtype=np.float64).reshape(-1, 4, 2)
    want = c + np.asarray(delta, dtype=np.float64).reshape(-1, 4, 2)
    p = np.concatenate([c, np.ones((len(c), 4, 1))], -1) @ h.transpose(0, 2, 1)
    return np.abs(p[..., :2] / p[..., 2:] - want).reshape(len(c), -1).max(1)


def warp(grey_a, h, align_corners, with_outside=False, dtype=np.float32):
    """``grey_b`` (B,1,S,S) fp32 from ``grey_a`` (B,1,S,S) fp32 and ``h`` (B,9) fp64, the header's arithmetic: every line below is one IEEE
    fp64 operation per element.  ``with_outside``: also the (B,1,S,S) bool map of elements with at least one tap outside the frame.
    ``dtype=np.float64`` returns the sum before its one rounding to fp32 (for the cross-check against grid_sample)."""
    grey_a = np.asarray(grey_a)
    assert grey_a.dtype == np.float32 and grey_a.ndim == 4 and grey_a.shape[1] == 1 and grey_a.shape[2] == grey_a.shape[3]
    h = np.asarray(h, dtype=np.float64).reshape(-1, 9)
    B, S = grey_a.shape[0], grey_a.shape[2]
    y, x = np.meshgrid(np.arange(S, dtype=np.float64), np.arange(S, dtype=np.float64), indexing="ij")
    out, outside = np.empty((B, 1, S, S), dtype=dtype), np.zeros((B, 1, S, S), dtype=bool)
    with np.errstate(all="ignore"):
        for b in range(B):
            if np.isnan(h[b, 0]):
                out[b] = np.nan
                continue
            hb, src = h[b], grey_a[b, 0].astype(np.float64)
            X = (hb[0] * x + hb[1] * y) + hb[2]
            Y = (hb[3] * x + hb[4] * y) + hb[5]
            Z = (hb[6] * x + hb[7] * y) + hb[8]
            u, v = X / Z, Y / Z
            if align_corners:
                sx, sy = u, v
            else:
                k = np.float64(S) / np.float64(S - 1)
                sx, sy = u * k - 0.5, v * k - 0.5
            fx, fy = np.floor(sx), np.floor(sy)
            wx1, wy1 = sx - fx, sy - fy
            wx0, wy0 = 1.0 - wx1, 1.0 - wy1
            acc = np.zeros((S, S), dtype=np.float64)
            for ty, tx, w in ((fy, fx, wx0 * wy0), (fy, fx + 1.0, wx1 * wy0), (fy + 1.0, fx, wx0 * wy1), (fy + 1.0, fx + 1.0, wx1 * wy1)):
                inside = (tx >= 0) & (tx <= S - 1) & (ty >= 0) & (ty <= S - 1)          # False for NaN
                iy, ix = np.where(inside, ty, 0).astype(np.int64), np.where(inside, tx, 0).astype(np.int64)
                acc = np.where(inside, acc + src[iy, ix] * w, acc)
                outside[b, 0] |= ~inside
            out[b, 0] = acc.astype(dtype)
    return (out, outside) if with_outside else out


def synth_items(views, geometry, deltas, S, P, mean, std, align_corners, h=None):
    """``views``: per item the stored (rows, pitch_px, 3) uint8 array; ``geometry``: per item ``(x0, y0, cw, ch, wx, wy)``; ``deltas``: per
    item eight integers.  Returns the seven outputs in the entry's order; ``h``: use these (B,9) fp64 words instead of ``dlt``'s."""
    grey_a, _, patch_a, _, corners = IR.prepare_items(views, views, geometry, S, P, mean, std)
    delta = np.asarray(deltas, dtype=np.float32).reshape(-1, 4, 2)
    h = dlt(corners, delta) if h is None else np.asarray(h, dtype=np.float64).reshape(-1, 9)
    grey_b = warp(grey_a, h, align_corners)
    patch_b = np.stack([grey_b[b, :, wy:wy + P, wx:wx + P] for b, (_, _, _, _, wx, wy) in enumerate(geometry)])
    return grey_a, patch_a, corners, delta, h, grey_b, patch_b


# ------------------------------------------------------------------------------------------------------------------- the cases
# The GPU test's batch, shared with the CPU test: the shapes, stored sizes and crops of tests/test_gpu_homonet_items.py -- a whole image,
# an interior crop at an odd origin, a crop flush against the last byte of its image, and an S x S copy.
S, P = 16, 8
STORED = [(13, 17), (32, 20), (9, 40), (16, 16)]                                    # (rows, pitch_px)
CROPS = [(0, 0, 17, 13), (3, 5, 11, 23), (7, 4, 33, 5), (0, 0, 16, 16)]             # (x0, y0, cw, ch)
RHOS = (2, 5)       # rho = 2: windows in [2, 6], every sample inside the frame's neighbourhood; rho = 5: S - rho - P < rho, the window is
#                     (0, 0) and negative deltas push samples outside the frame, onto the zero-padding path


def stored_views():
    """The four stored views: random bytes with the even-level and corner tweaks of the item test's ``_case()``."""
    g = np.random.Generator(np.random.PCG64(2025))
    views = [g.integers(0, 256, size=(r, p, 3), dtype=np.uint8) for r, p in STORED]
    for v in views:
        v[: max(v.shape[0] // 2, 1), : max(v.shape[1] // 2, 1)] &= 0xFE          # even levels: averages land on k + 0.5 there
        v[0, 0], v[-1, -1] = 255, 0
    return views


def case(rho):
    """``(geometry, deltas)`` of the batch for ``rho``: the windows by ``homography.window_origins``' rule, the deltas by
    ``homography.draw_deltas``, both from seeded streams of their own."""
    import random

    from hesic_amd import homography
    windows = homography.window_origins(len(CROPS), None, S, P, rho, random.Random(f"synth-case/{rho}/windows"))
    deltas = homography.draw_deltas(len(CROPS), windows, P, rho, random.Random(f"synth-case/{rho}/deltas"))
    return [c + w for c, w in zip(CROPS, windows)], deltas

"""numpy restatement of ``hesic_pair_batch_gather_aug`` (include/hesic_pair_augment.h), operation for operation in the order the header states:
the pixels are those of tests/pair_batch_ref.py read through the header's index map, and for the matrix every fp64 product, sum,
difference and quotient is ONE numpy operation on scalars, so nothing is fused and nothing is reassociated.  The GPU test holds the kernel
to these bits; tests/test_pair_augment_cpu.py holds this file to numpy flips, ``numpy.linalg.inv`` and a bilinear warp."""
import numpy as np

F = np.float32
D = np.float64
HFLIP, VFLIP, SWAP = 1, 2, 4


def pixels(left, right, x0, y0, ph, pw, flags):
    """(x1, x2) of one item, (3, ph, pw) fp32 each: x1[c, r, q] = (float)A[y0 + r', x0 + q', c] / 255.0f, index by index as the header
    writes it (no numpy flip: tests/test_pair_augment_cpu.py compares this against ``[::-1]``)."""
    A, B = (right, left) if flags & SWAP else (left, right)
    rows = np.array([ph - 1 - r if flags & VFLIP else r for r in range(ph)]) + y0
    cols = np.array([pw - 1 - q if flags & HFLIP else q for q in range(pw)]) + x0
    assert 0 <= cols.min() and cols.max() < A.shape[1] and 0 <= rows.min() and rows.max() < A.shape[0]
    out = []
    for view in (A, B):
        assert view.dtype == np.uint8 and view.ndim == 3 and view.shape[2] == 3
        crop = view[rows[:, None], cols[None, :]].transpose(2, 0, 1).astype(F)
        out.append((crop / F(255.0)).astype(F))
    return out[0], out[1]


def rebased(H, hx, hy):
    """R of include/hesic_pair_batch.h BEFORE its division, fp64 (3, 3): the operations of ``pair_batch_ref.matrix``."""
    H = np.asarray(H, dtype=D).reshape(3, 3)
    hx, hy = D(hx), D(hy)
    G = np.empty((3, 3), dtype=D)
    for j in range(3):
        G[0, j] = H[0, j] - hx * H[2, j]
        G[1, j] = H[1, j] - hy * H[2, j]
        G[2, j] = H[2, j]
    Rm = np.empty((3, 3), dtype=D)
    for i in range(3):
        Rm[i, 0] = G[i, 0]
        Rm[i, 1] = G[i, 1]
        Rm[i, 2] = (G[i, 0] * hx + G[i, 1] * hy) + G[i, 2]
    return Rm


def _mirror(Rm, ax, e):
    """R <- F R F for the mirror of axis ``ax`` (0: HFLIP, 1: VFLIP) with e = extent - 1: S = F R, then T = S F."""
    S = Rm.copy()
    for j in range(3):
        S[ax, j] = e * Rm[2, j] - Rm[ax, j]
    T = S.copy()
    for i in range(3):
        T[i, ax] = -S[i, ax]
        T[i, 2] = e * S[i, ax] + S[i, 2]
    return T


def _adjugate(m):
    U = np.empty((3, 3), dtype=D)
    U[0, 0] = m[1, 1] * m[2, 2] - m[1, 2] * m[2, 1]
    U[0, 1] = m[0, 2] * m[2, 1] - m[0, 1] * m[2, 2]
    U[0, 2] = m[0, 1] * m[1, 2] - m[0, 2] * m[1, 1]
    U[1, 0] = m[1, 2] * m[2, 0] - m[1, 0] * m[2, 2]
    U[1, 1] = m[0, 0] * m[2, 2] - m[0, 2] * m[2, 0]
    U[1, 2] = m[0, 2] * m[1, 0] - m[0, 0] * m[1, 2]
    U[2, 0] = m[1, 0] * m[2, 1] - m[1, 1] * m[2, 0]
    U[2, 1] = m[0, 1] * m[2, 0] - m[0, 0] * m[2, 1]
    U[2, 2] = m[0, 0] * m[1, 1] - m[0, 1] * m[1, 0]
    return U


def matrix64(H, hx, hy, ph, pw, flags):
    """The augmented matrix before the cast: fp64 (3, 3), R / R[2][2] after the header's steps."""
    Rm = rebased(H, hx, hy)
    if flags & HFLIP:
        Rm = _mirror(Rm, 0, D(pw - 1))
    if flags & VFLIP:
        Rm = _mirror(Rm, 1, D(ph - 1))
    if flags & SWAP:
        Rm = _adjugate(Rm)
    out = np.empty((3, 3), dtype=D)
    for i in range(3):
        for j in range(3):
            out[i, j] = Rm[i, j] / Rm[2, 2]
    return out


def matrix(H, hx, hy, ph, pw, flags):
    """(3, 3) fp32 ``h_out`` of one item; ``H`` nine fp64 values row-major, or None (h_index = -1): the identity whatever the flags."""
    if H is None:
        return np.eye(3, dtype=F)
    return matrix64(H, hx, hy, ph, pw, flags).astype(F)


def gather(items, h_table, ph, pw):
    """``items``: [(left view, right view, x0, y0, hx, hy, h_index, flags)] -- ``pair_batch_ref.gather``'s tuples with the flags appended.
    Returns (x1, x2, h): (B,3,ph,pw), (B,3,ph,pw), (B,3,3) fp32."""
    px = [pixels(it[0], it[1], it[2], it[3], ph, pw, it[7]) for it in items]
    h = np.stack([matrix(None if it[6] < 0 else h_table[it[6]], it[4], it[5], ph, pw, it[7]) for it in items])
    return np.stack([p[0] for p in px]), np.stack([p[1] for p in px]), h


def plan_batches(plan, images, h_rows, ph, pw):
    """The restatement applied to an ``epoch_plan`` and its ``plan.flags`` (``pair_batch_ref.plan_batches`` with the flags)."""
    for (indices, origins), flags in zip(plan, plan.flags):
        table = [h_rows[i] for i in indices]
        items = [(images[i][0], images[i][1], x0, y0, x0, y0, -1 if h_rows[i] is None else k, f)
                 for k, (i, (y0, x0), f) in enumerate(zip(indices, origins, flags))]
        yield gather(items, table, ph, pw)

"""numpy restatement of ``hesic_pair_batch_gather`` (include/hesic_pair_batch.h), operation for operation in the order the header states:
one fp32 division per pixel sample, and for the matrix every fp64 product, sum, difference and quotient ONE numpy operation on scalars, so
nothing is fused and nothing is reassociated.  The GPU test holds the kernel to these bits; tests/test_pair_batch_cpu.py holds this file to
the loader's host path (``compressai.datasets.ImageFolder``)."""
import numpy as np

F = np.float32
D = np.float64


def pixels(view, x0, y0, ph, pw):
    """(3, ph, pw) fp32 of a stored (rows, pitch_px, 3) uint8 view: x[c, r, q] = (float)view[y0 + r, x0 + q, c] / 255.0f."""
    assert view.dtype == np.uint8 and view.ndim == 3 and view.shape[2] == 3
    assert 0 <= x0 and x0 + pw <= view.shape[1] and 0 <= y0 and y0 + ph <= view.shape[0]
    crop = view[y0:y0 + ph, x0:x0 + pw].transpose(2, 0, 1).astype(F)
    return (crop / F(255.0)).astype(F)


def matrix(H, hx, hy):
    """(3, 3) fp32: T(-t) H T(t) / [2,2] with t = (hx, hy); ``H`` nine fp64 values row-major, or None (h_index = -1): the identity."""
    if H is None:
        return np.eye(3, dtype=F)
    H = np.asarray(H, dtype=D).reshape(3, 3)
    hx, hy = D(hx), D(hy)
    G = np.empty((3, 3), dtype=D)
    for j in range(3):
        G[0, j] = H[0, j] - hx * H[2, j]
        G[1, j] = H[1, j] - hy * H[2, j]
        G[2, j] = H[2, j]
    R = np.empty((3, 3), dtype=D)
    for i in range(3):
        R[i, 0] = G[i, 0]
        R[i, 1] = G[i, 1]
        R[i, 2] = (G[i, 0] * hx + G[i, 1] * hy) + G[i, 2]
    out = np.empty((3, 3), dtype=F)
    for i in range(3):
        for j in range(3):
            out[i, j] = F(R[i, j] / R[2, 2])
    return out


def gather(items, h_table, ph, pw):
    """``items``: [(left view, right view, x0, y0, hx, hy, h_index)] with the views as (rows, pitch_px, 3) uint8 arrays.
    Returns (x1, x2, h): (B,3,ph,pw), (B,3,ph,pw), (B,3,3) fp32."""
    x1 = np.stack([pixels(it[0], it[2], it[3], ph, pw) for it in items])
    x2 = np.stack([pixels(it[1], it[2], it[3], ph, pw) for it in items])
    h = np.stack([matrix(None if it[6] < 0 else h_table[it[6]], it[4], it[5]) for it in items])
    return x1, x2, h


def plan_batches(plan, images, h_rows, ph, pw):
    """The restatement applied to an ``epoch_plan``: ``images[i] = (left, right)`` the decoded uint8 HWC views of pair i, ``h_rows[i]`` its
    nine fp64 sidecar values or None.  Yields (x1, x2, h) per batch, the crop origin doubling as the re-basing translation."""
    for indices, origins in plan:
        table = [h_rows[i] for i in indices]
        items = [(images[i][0], images[i][1], x0, y0, x0, y0, -1 if h_rows[i] is None else k)
                 for k, (i, (y0, x0)) in enumerate(zip(indices, origins))]
        yield gather(items, table, ph, pw)

"""numpy fp32 restatement of ``hesic_homonet_prepare`` (include/hesic_homography_prep.h), operation for operation in the order the header
states: every product, sum, difference and quotient below is ONE fp32 numpy operation, so nothing is fused and nothing is reassociated.
The GPU test holds the kernel to these bits; tests/test_homography_prep_cpu.py holds this file to the loader's host path
(``ImageFolder._homonet_inputs``)."""
import numpy as np

F = np.float32

# (H, W) -> S, P, rho: the parity list of the GPU test, shared with the CPU test of this restatement against the loader
CASES = [
    ((64, 64), 32, 16, 4),          # exact 2:1, every tie half-to-even
    ((37, 53), 64, 32, 8),          # upsampling, odd sizes, both edge clamps
    ((96, 128), 256, 128, 45),      # the defaults at the dataset golden's size
    ((300, 517), 256, 128, 45),     # non-integer ratios, one above 2
    ((256, 256), 256, 128, 45),     # identity
    ((1, 5), 16, 8, 0),             # a one-row image
    ((40, 40), 64, 32, 20),         # the x = y = 0 fallback (S - rho - P < rho)
]


def case_id(case):
    (h, w), s, p, rho = case
    return f"{h}x{w}_to{s}_p{p}_rho{rho}"


def images(case, batch=3, seed=0):
    """Two uint8 (B,3,H,W) arrays of random levels (with runs of equal neighbours and the extremes 0 / 255 in them)."""
    (h, w), _, _, _ = case
    g = np.random.Generator(np.random.PCG64([seed, h, w]))
    x = g.integers(0, 256, size=(2, batch, 3, h, w), dtype=np.uint8)
    x[:, :, :, : max(h // 4, 1), : max(w // 4, 1)] &= 0xFE           # a region of even levels: 2:1 averages land on k + 0.5 there
    x[:, 0, :, 0, 0] = 255
    x[:, 0, :, -1, -1] = 0
    return x[0], x[1]


def windows(case, batch=3):
    """(rho, rho), (S-rho-P, S-rho-P) and one mixed -- or the fallback's (0, 0) where the rule leaves no room."""
    _, s, p, rho = case
    hi = s - rho - p
    if hi < rho:
        return [(0, 0)] * batch
    return ([(rho, rho), (hi, hi), (rho + (hi - rho) // 3, hi)] * batch)[:batch]


def levels(x):
    """The grey level of every sample as fp32: the byte, or rint(255 v) clamped to [0, 255]."""
    x = np.asarray(x)
    if x.dtype == np.uint8:
        return x.astype(F)
    assert x.dtype == F
    return np.clip(np.rint(F(255.0) * x), F(0.0), F(255.0)).astype(F)


def axis(n, S):
    """(i0, i1, l0, l1) of the S output positions along an axis of length n."""
    scale = F(n) / F(S)
    d = np.arange(S, dtype=F)
    s = np.maximum(scale * (d + F(0.5)) - F(0.5), F(0.0)).astype(F)
    i0 = np.minimum(s.astype(np.int64), n - 1)
    i1 = np.minimum(i0 + 1, n - 1)
    l1 = (s - i0.astype(F)).astype(F)
    l0 = (F(1.0) - l1).astype(F)
    return i0, i1, l0, l1


def resized_levels(x, S):
    """(B,3,H,W) uint8 / fp32 -> (B,3,S,S) fp32 integer levels: r = clamp(rint(hy0 (wx0 a + wx1 b) + hy1 (wx0 c + wx1 d)), 0, 255)."""
    lv = levels(x)
    H, W = lv.shape[-2:]
    y0, y1, hy0, hy1 = axis(H, S)
    x0, x1, wx0, wx1 = axis(W, S)
    a, b = lv[..., y0[:, None], x0[None, :]], lv[..., y0[:, None], x1[None, :]]
    c, d = lv[..., y1[:, None], x0[None, :]], lv[..., y1[:, None], x1[None, :]]
    top = (wx0 * a).astype(F) + (wx1 * b).astype(F)
    bot = (wx0 * c).astype(F) + (wx1 * d).astype(F)
    v = (hy0[:, None] * top).astype(F) + (hy1[:, None] * bot).astype(F)
    assert v.dtype == F
    return np.clip(np.rint(v), F(0.0), F(255.0)).astype(F)


def grey(x, S, mean, std):
    """(B,1,S,S) fp32: ((r0/255 - mean)/std + (r1/255 - mean)/std + (r2/255 - mean)/std) / 3, left to right."""
    mean, std = F(mean), F(std)
    n = ((resized_levels(x, S) / F(255.0)).astype(F) - mean) / std
    assert n.dtype == F
    return (((n[:, 0] + n[:, 1]) + n[:, 2]) / F(3.0)).astype(F)[:, None]


def prepare(x1, x2, xy, S, P, mean, std):
    """The five outputs of hesic_homonet_prepare as fp32 numpy arrays."""
    g1, g2 = grey(x1, S, mean, std), grey(x2, S, mean, std)
    p1 = np.stack([g1[b, :, y:y + P, x:x + P] for b, (x, y) in enumerate(xy)])
    p2 = np.stack([g2[b, :, y:y + P, x:x + P] for b, (x, y) in enumerate(xy)])
    corners = np.array([[[x, y], [x + P, y], [x + P, y + P], [x, y + P]] for x, y in xy], dtype=F)
    return g1, g2, p1, p2, corners


def _loader(S, P, rho):
    """An ``ImageFolder`` without a folder: ``_homonet_inputs`` reads only these three attributes."""
    from hesic_amd.compressai.datasets import ImageFolder
    ds = object.__new__(ImageFolder)
    ds.homopic_size, ds.homopatch_size, ds.rho = S, P, rho
    return ds


def loader_items(x1, x2, S, P, rho, seed):
    """``ImageFolder._homonet_inputs`` per item of the uint8 (B,3,H,W) pairs after ``random.seed(seed)``: (patch1, patch2, corners) as
    fp32 numpy arrays, the windows the loader's own draws."""
    import random
    ds = _loader(S, P, rho)
    random.seed(seed)
    items = [ds._homonet_inputs(np.ascontiguousarray(a.transpose(1, 2, 0)), np.ascontiguousarray(b.transpose(1, 2, 0))) for a, b in zip(x1, x2)]
    return tuple(np.stack([it[k].numpy() for it in items]) for k in range(3))


def loader_greys(x1, x2, S):
    """The loader's whole grey frames (B,1,S,S): ``_homonet_inputs`` with the window set to the frame (P = S, rho = 0 -> origin (0, 0))."""
    g1, g2, corners = loader_items(x1, x2, S, S, 0, 0)
    assert (corners[:, 0] == 0).all() and g1.shape[-2:] == (S, S)
    return g1, g2


def cut(g, xy, P):
    return np.stack([g[b, :, y:y + P, x:x + P] for b, (x, y) in enumerate(xy)])

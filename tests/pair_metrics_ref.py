"""fp64 / numpy restatement of the per-pair rate-distortion table (include/hesic_pair_metrics.h) and of the figures derived from it (a plain
module, not a conftest).  tests/test_pair_metrics_cpu.py holds it to the reference's definitions (the criterion of ywz/mywork/test3real.py at
batch 1, ``codec.quantise``'s uint8 images); tests/test_gpu_pair_metrics.py holds the kernel and ``models.pair_metrics*`` to it.

    table(liks, pairs)      (B, n_lik + 4) fp64: sum(log2 lik_i) over image b, sse1, sse2, sse8_1, sse8_2
    figures(table, keys, h, w, channels)   dict of (B,) fp64 arrays under ``models.pair_metrics_from``'s names
"""
import numpy as np
import torch


def _np(t):
    return t.detach().float().cpu().numpy() if torch.is_tensor(t) else np.asarray(t, dtype=np.float32)


def quantise8(v):
    """What a decoder's PNG holds, as fp32 values: ``codec.quantise``'s fp32 arithmetic, clamp to [0, 1], * 255, round half to even.  NaN stays NaN."""
    v = _np(v).astype(np.float32)
    with np.errstate(invalid="ignore"):
        return np.rint(np.clip(v, np.float32(0), np.float32(1)) * np.float32(255))


def sse8(a, b):
    """(B,) fp64: sum over image b of (q(a) - q(b))^2, an integer summed as integers; NaN for an image with a NaN operand."""
    qa, qb = quantise8(a), quantise8(b)
    B = qa.shape[0]
    out = np.empty(B, dtype=np.float64)
    for i in range(B):
        if np.isnan(qa[i]).any() or np.isnan(qb[i]).any():
            out[i] = np.nan
        else:
            d = qa[i].astype(np.int64) - qb[i].astype(np.int64)
            out[i] = float((d * d).sum())
    return out


def sse(a, b):
    """(B,) fp64: sum over image b of (a - b)^2, every operation in fp64 on the operands' exact values."""
    d = _np(a).astype(np.float64) - _np(b).astype(np.float64)
    return (d * d).reshape(d.shape[0], -1).sum(1)


def log2_sums(lik):
    """(B,) fp64: sum(log2(lik)) over image b of a map with the batch outermost."""
    l = _np(lik).astype(np.float64)
    return np.log2(l).reshape(l.shape[0], -1).sum(1)


def table(liks, pairs):
    (a1, b1), (a2, b2) = pairs
    cols = [log2_sums(l) for l in liks] + [sse(a1, b1), sse(a2, b2), sse8(a1, b1), sse8(a2, b2)]
    return np.stack(cols, 1)


def psnr_db(mse, peak=1.0):
    """10 log10(peak^2 / mse); exactly 100 where the error is zero (the reference's ``psnr()``, test3real.py:74-79)."""
    mse = np.asarray(mse, dtype=np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(mse == 0, 100.0, 10.0 * np.log10(peak * peak / mse))


def figures(tab, keys, h, w, channels=3):
    tab = np.asarray(tab, dtype=np.float64)
    n, nl = h * w, len(keys)
    bits = {k: -tab[:, i] for i, k in enumerate(keys)}
    mse1, mse2 = tab[:, nl] / (n * channels), tab[:, nl + 1] / (n * channels)
    p1, p2 = psnr_db(mse1), psnr_db(mse2)
    q1, q2 = psnr_db(tab[:, nl + 2] / (n * channels), 255.0), psnr_db(tab[:, nl + 3] / (n * channels), 255.0)
    bpp_loss = sum(bits.values(), np.zeros(tab.shape[0])) / n
    return {"bits": bits, "bpp_loss": bpp_loss, "bpp": bpp_loss / 2, "mse1": mse1, "mse2": mse2, "psnr1": p1, "psnr2": p2, "psnr": (p1 + p2) / 2,
            "psnr8_1": q1, "psnr8_2": q2, "psnr8": (q1 + q2) / 2}

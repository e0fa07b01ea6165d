"""numpy restatement of include/hesic_en_train.h: what the GPU tests hold ``hesic_en_loss``, ``hesic_en_loss_grad`` and
``hesic_c32_mirror_weights`` to.  Nothing here calls the library or torch."""
import math

import numpy as np


# ---------------------------------------------------------------------------------------------- fp32 -> 16 bits, round to nearest even
def round_bf16_bits(x):
    """fp32 array -> uint16 bfloat16 bits, round to nearest even by integer arithmetic; NaN -> a quiet NaN of the same sign."""
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32).astype(np.uint64)
    r = ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint32)
    nan = (u & 0x7FFFFFFF) > 0x7F800000
    r = np.where(nan, (u >> 16).astype(np.uint32) | 0x40, r)
    return (r & 0xFFFF).astype(np.uint16)


def round_f16_bits(x):
    """fp32 array -> uint16 IEEE binary16 bits, round to nearest even by integer arithmetic: subnormal results, overflow to infinity (no
    saturation), NaN -> a quiet NaN of the same sign."""
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32).astype(np.int64)
    sign = ((u >> 16) & 0x8000).astype(np.int64)
    mag = u & 0x7FFFFFFF
    e = (mag >> 23) - 127                                   # unbiased exponent (-127 for fp32 zeros / subnormals)
    m = (mag & 0x7FFFFF) | 0x800000                         # 24-bit significand with the hidden bit (wrong for fp32 subnormals: they round to 0)
    # the value is m * 2^(e - 23); binary16 keeps 10 fraction bits at exponent >= -14, so the unit of the result is 2^(max(e, -14) - 10)
    shift = np.clip(13 + np.maximum(-14 - e, 0), 13, 40)
    keep = m >> shift
    rem = m & ((np.int64(1) << shift) - 1)
    half = np.int64(1) << (shift - 1)
    keep = keep + ((rem > half) | ((rem == half) & ((keep & 1) == 1)))
    # normal: keep has the hidden bit at 2^10, so (e + 15 - 1) << 10 plus keep carries a rounding overflow into the exponent by itself;
    # subnormal (e < -14): keep is the fraction (or 2^10 = the smallest normal), exponent field 0
    out = np.where(e >= -14, ((e + 14) << 10) + keep, keep)
    out = np.where(mag < 0x33000000, 0, out)                # below 2^-25: rounds to zero (2^-25 itself is a tie to even = 0 as well)
    out = np.where(out >= 0x7C00, 0x7C00, out)              # overflow -> infinity
    out = np.where(mag == 0x7F800000, 0x7C00, out)
    out = np.where(mag > 0x7F800000, 0x7E00, out)
    return (sign | out).astype(np.uint16)


ROUND = {"bf16": round_bf16_bits, "f16": round_f16_bits}


# ------------------------------------------------------------------------------------------------------------------------ the criterion
def scale(B, H, W, lambda_255sq, seed=None):
    """s of hesic_en_loss_grad: 2 * lambda_255sq / n in double, rounded once to fp32, then times the fp32 seed in fp32."""
    s = np.float32(2.0 * float(lambda_255sq) / (float(B) * 3.0 * float(H) * float(W)))
    return s if seed is None else np.float32(s * np.float32(seed))


def grad_map_bits(a, b, lambda_255sq, fmt, seed=None):
    """(B, H, W, 32) uint16: channels 0..2 = round16(s * (a - b)) -- an fp32 subtract, an fp32 multiply, one rounding --, channels 3..31 zero."""
    a, b = np.asarray(a, dtype=np.float32), np.asarray(b, dtype=np.float32)
    B, C, H, W = a.shape
    assert C == 3
    with np.errstate(over="ignore", invalid="ignore"):
        g = (scale(B, H, W, lambda_255sq, seed) * (a - b).astype(np.float32)).astype(np.float32)
    out = np.zeros((B, H, W, 32), dtype=np.uint16)
    out[..., :3] = ROUND[fmt](g).transpose(0, 2, 3, 1)
    return out


def exact_sse(a, b):
    """sum((a - b)^2) with the fp32 difference widened to fp64 and squared there (exact), added without error by ``math.fsum``."""
    d = (np.asarray(a, dtype=np.float32) - np.asarray(b, dtype=np.float32)).astype(np.float64).reshape(-1)
    return math.fsum((d * d).tolist())


def loss_values(a1, b1, a2, b2, lambda_255sq):
    """[sse1, sse2, mse_loss, loss] of hesic_en_loss from the exact sums."""
    n = float(np.asarray(a1).size)
    s1, s2 = exact_sse(a1, b1), exact_sse(a2, b2)
    mse = s1 / n + s2 / n
    return [s1, s2, mse, float(lambda_255sq) * mse]


def sum_bar(n):
    """The relative bar of a sum of n exact non-negative fp64 terms added in ANY order: each of the n - 1 additions errs by at most 2^-53 of
    its (partial, hence smaller) result, so the total is within ((1 + 2^-53)^(n-1) - 1) <= (n + 8) * 2^-53 of the exact sum for every n
    these tests use."""
    return (n + 8) * 2.0 ** -53


# ---------------------------------------------------------------------------------------------------------------------------- the mirror
def mirror(w, pad_to=None):
    """(Cout, Cin, 3, 3) -> (Cin, max(Cout, pad_to), 3, 3): channels exchanged, taps mirrored, rows Cout.. zero."""
    w = np.asarray(w, dtype=np.float32)
    m = np.ascontiguousarray(w[:, :, ::-1, ::-1].transpose(1, 0, 2, 3))
    if pad_to is not None and m.shape[1] < pad_to:
        m = np.concatenate((m, np.zeros((m.shape[0], pad_to - m.shape[1], 3, 3), dtype=np.float32)), 1)
    return m

"""fp64 references with a per-element error model for the warp kernels (csrc/warp.hip) and the map / reduction half of csrc/glue.hip
(a plain module, not a conftest).  Used by tests/test_glue_ref_cpu.py (no GPU) and tests/test_gpu_glue_parity.py.

Every operand holds values that are exact in whatever the kernel receives: ``grid16`` draws from the 1/16 grid in [-2, 2] (exact in bf16,
IEEE half and fp32), both signs, exact zeros where |x| < 0.25.  A reference returns a dict  {"ref", "unit"[, "store"]}  of fp64 tensors and
``check`` asserts  |got_e - ref_e| <= c * unit_e + store_e  for every element; where unit_e == 0 the value must be exactly ref_e.  The printed
ratio is  max_e (|err_e| - store_e) / unit_e.  ``c`` is 1 for the bilinear samplers, whose unit bound is already a worst-case rounding count,
and ``C_BAR`` = 8 for the sums, whose unit bound  sqrt(n) 2^-24 S_e  is the statistical bound of tests/conv_grad_ref.py.

Bilinear samplers (warp forward, upsample4).  f(sx, sy) = sum_taps w v with zero (warp) or edge (upsample) padding is continuous in (sx, sy);
inside a cell |df/dsx| = |wy0 (v01 - v00) + wy1 (v11 - v10)| <= the largest x-neighbour difference of the cell's two rows, the padding counted
as a neighbour.  Lx_e / Ly_e take that maximum over the cells within one pixel of the sample point (a rounding never moves it further), so

    unit_e = k_c 2^-24 (max(1, |sx|) Lx_e + max(1, |sy|) Ly_e) + k_s 2^-24 sum_taps |w v|.

  k_c (coordinate roundings, in units of 2^-24 relative to max(1, |s|)):
    warp: the coordinate is formed in fp64 and rounded to fp32 ONCE (<= 1); wx1 = sx - floor(sx) is exact except for -1 < sx < 0, where it
          rounds by <= 2^-25 (<= 0.5); the fp64 restatement differs from the kernel's by a few 2^-53.  1.5 -> K_C_WARP = 2.
    upsample4: r = fl(fl(in-1) / fl(out-1)) and s = fl(r * dst), two roundings relative to s (2); s - trunc(s) is exact.  K_C_UP = 3 leaves the
          same half unit plus slack.
  k_s (roundings a tap's product w v meets, relative): 1 - wx1 (exact by Sterbenz for wx1 >= 1/2, else one rounding of a value >= 1/2: <= 2^-24
    relative), 1 - wy1 likewise, wx * wy, w * v, and at most three additions of partial sums each bounded by sum |w v| : 7, second-order terms
    -> K_S = 8.  (upsample4's nested lerp has six per tap.)
  Where all four taps lie outside the image the unit is 0 and the output must be exactly 0: rounding to fp32 is monotone, so it never carries a
  sample point across the integer at which the last tap leaves the image, and at that integer the tap's weight is exactly 0.
  A 16-bit destination adds ``store`` = u |ref| (+ h for IEEE half's subnormal step), u = 2^-8 / 2^-11.

Warp backward (float atomics, fp32):  d_src_e = sum_p g_p tent(sx_p - cx) tent(sy_p - cy).  bar_e = C_BAR sqrt(n_e) 2^-24 S_e +
K_C_WARP 2^-24 sum_p |g_p| (max(1, |sx_p|) + max(1, |sy_p|)), n_e contributions, S_e = sum |g w|, the second sum over the destination pixels
whose sample point lies within 1 + 2^-20 of the cell in both axes (the tent's slope is <= 1 per axis; this term travels as "store", the
first as "unit").  Exactly 0 where that set is empty.  upsample4's backward, a gather of at most 8 x 8 terms, is held to C_BAR * 8 * 2^-24 S_e.

Nothing here is fitted to a kernel: tests/test_glue_ref_cpu.py asserts that torch's own fp32 evaluation of every family stays below 1.0 of
the unit bound, and that seeded mutations of a correct result leave their bars.
"""
import functools
import math

import torch
import torch.nn.functional as F

from hesic_amd import synthetic

C_BAR = 8.0
U24 = 2.0 ** -24
K_C_WARP, K_C_UP, K_S = 2.0, 3.0, 8.0
FMT = {torch.bfloat16: (2.0 ** -8, 0.0), torch.float16: (2.0 ** -11, 2.0 ** -25), torch.float32: (0.0, 0.0), None: (0.0, 0.0)}
LEAK = torch.tensor(0.01, dtype=torch.float32)          # the kernels' 0.01f
# relative error of one device log2f.  The installed ROCm documentation states no ulp bound, so it is measured: the largest per-term error
# on an MI355X over the sum_log2 case inputs (9237 one-element hesic_sum_log2 calls: the scalar loop's log2f, widened to fp64) was
# 1.1506e-7 * max(|log2 x|, 2^-24), just under 2^-23 (profiles/glue_parity.json: "log2f_per_term"); U_LOG is twice that.
U_LOG = 2 * 1.1506e-7


def grid16(name, shape, zero_below=0.25):
    x = synthetic._uniform("glue." + name, shape, -2, 2)
    x = torch.where(x.abs() < zero_below, torch.zeros(()), x)
    return torch.round(x * 16) / 16


def storage(ref, dtype, live=None):
    u, h = FMT[dtype]
    s = u * ref.abs()
    return s + h * (live if live is not None else 1.0) if h else s


def check(R, got, c=1.0, name=""):
    """(ok, ratio, message) of ``got`` against R = {"ref", "unit"[, "store"]}: no element is left out."""
    ref, unit = R["ref"], R["unit"]
    got = got.detach().double().cpu().reshape(ref.shape)
    store = R.get("store")
    store = torch.zeros_like(ref) if store is None else store
    err = (got - ref).abs()
    live = unit > 0
    ratio = float(((err - store).clamp_min(0)[live] / unit[live]).max()) if bool(live.any()) else 0.0
    bad = ~(err <= c * unit + store)                  # NaN counts as a miss
    msg = ""
    if bool(bad.any()):
        idx = torch.nonzero(bad)
        worst = tuple(int(i) for i in idx[torch.argmax(torch.nan_to_num(err - c * unit - store, nan=1e300)[bad])])
        msg = (f"{name}: {int(bad.sum())} of {bad.numel()} elements outside their bar; worst at {worst}: got {float(got[worst]):.9g} "
               f"ref {float(ref[worst]):.9g} bar {float((c * unit + store)[worst]):.3g}; first index per dim {[int(i) for i in idx.min(0).values]} "
               f"last {[int(i) for i in idx.max(0).values]}; dead elements hit {int((bad & ~live & (store == 0)).sum())}")
    return not bool(bad.any()), ratio, msg


def same_bits(a, b):
    """Bit-for-bit equality of two tensors of one dtype (signed zeros and NaN payloads included)."""
    a, b = a.detach().cpu().contiguous(), b.detach().cpu().contiguous()
    it = {4: torch.int32, 2: torch.int16, 8: torch.int64}[a.element_size()]
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.view(it), b.view(it))


# ============================================================================================================ bilinear sampling
def _pooled_gather(D, kh, kw, idx):
    """max of D over a kh x kw window centred on each cell, gathered at the flat index ``idx`` (B, 1, P) for every channel."""
    Mx = F.max_pool2d(D, (kh, kw), stride=1, padding=(kh // 2, kw // 2))
    return torch.gather(Mx.flatten(2), 2, idx.expand(-1, D.shape[1], -1))


def sample(src, sx, sy, *, pad="zero", k_c=K_C_WARP, taps=None):
    """Bilinear sampling of src (B, C, H, W) at the fp64 points sx, sy (B, Ho, Wo): {"ref", "unit", "S", "dead"}, all (B, C, Ho, Wo) fp64.
    ``taps(x0, y0, k)`` may veto a tap (the CPU test's mutations)."""
    B, Cc, H, W = src.shape
    Ho, Wo = sx.shape[-2:]
    fin = torch.isfinite(sx) & torch.isfinite(sy)
    fx0, fy0 = torch.floor(sx), torch.floor(sy)
    big = ~fin | (fx0.abs() > 1e8) | (fy0.abs() > 1e8)
    wx1, wy1 = torch.where(big, 0.0, sx - fx0), torch.where(big, 0.0, sy - fy0)
    x0 = torch.where(big, -10.0, fx0).clamp(-2, W).long()
    y0 = torch.where(big, -10.0, fy0).clamp(-2, H).long()
    P = F.pad(src.double(), (2, 2, 2, 2), mode="constant" if pad == "zero" else "replicate")
    Wp = W + 4
    flat = P.flatten(2)
    val = torch.zeros((B, Cc, Ho * Wo), dtype=torch.float64)
    S = torch.zeros_like(val)
    inside = torch.zeros((B, 1, Ho * Wo), dtype=torch.bool)
    for k, (dy, dx) in enumerate(((0, 0), (0, 1), (1, 0), (1, 1))):
        w = ((wx1 if dx else 1 - wx1) * (wy1 if dy else 1 - wy1)).reshape(B, 1, -1)
        xi, yi = x0 + dx, y0 + dy
        ok = ((xi >= 0) & (xi < W) & (yi >= 0) & (yi < H)) if pad == "zero" else torch.ones_like(xi, dtype=torch.bool)
        if taps is not None:
            ok = ok & taps(xi, yi, k)
        ok = ok.reshape(B, 1, -1)
        v = torch.gather(flat, 2, ((yi + 2) * Wp + xi + 2).reshape(B, 1, -1).expand(-1, Cc, -1)) * ok
        val += w * v
        S += (w * v).abs()
        inside |= ok
    Dx = (P[..., 1:] - P[..., :-1]).abs()                       # (H+4, W+3): cell x0 at column x0 + 2
    Dy = (P[..., 1:, :] - P[..., :-1, :]).abs()                 # (H+3, W+4)
    Lx = _pooled_gather(Dx, 5, 3, ((y0 + 2) * (W + 3) + x0 + 2).reshape(B, 1, -1))
    Ly = _pooled_gather(Dy, 3, 5, ((y0.clamp(max=H) + 2) * Wp + x0 + 2).reshape(B, 1, -1))
    ax = torch.where(big, 1.0, sx.abs().clamp_min(1.0)).reshape(B, 1, -1)
    ay = torch.where(big, 1.0, sy.abs().clamp_min(1.0)).reshape(B, 1, -1)
    unit = (k_c * U24 * (ax * Lx + ay * Ly) + K_S * U24 * S) * inside
    shp = (B, Cc, Ho, Wo)
    return {"ref": val.reshape(shp), "unit": unit.reshape(shp), "S": S.reshape(shp), "dead": (~inside).expand(-1, Cc, -1).reshape(shp)}


def warp_coords(M, H, W, Ho, Wo, align_corners, inverse_map):
    """The kernel's coordinate chain in fp64: 3x3 adjugate / determinant inverse (skipped for ``inverse_map``), projective divide and the
    ``align_corners=False`` remap  x * W / (W - 1) - 0.5."""
    m = M.double().reshape(-1, 9)
    if inverse_map:
        iv = m
    else:
        a, b, c, d, e, f, g, h, i = m.unbind(1)
        A, Bc, Cc = e * i - f * h, -(d * i - f * g), d * h - e * g
        inv = 1.0 / (a * A + b * Bc + c * Cc)
        iv = torch.stack((A * inv, -(b * i - c * h) * inv, (b * f - c * e) * inv, Bc * inv, (a * i - c * g) * inv, -(a * f - c * d) * inv,
                          Cc * inv, -(a * h - b * g) * inv, (a * e - b * d) * inv), 1)
    iv = iv.reshape(-1, 9, 1, 1)
    oy, ox = torch.meshgrid(torch.arange(Ho, dtype=torch.float64), torch.arange(Wo, dtype=torch.float64), indexing="ij")
    X, Y, Z = (iv[:, 3 * r] * ox + iv[:, 3 * r + 1] * oy + iv[:, 3 * r + 2] for r in range(3))
    x, y = X / Z, Y / Z
    if not align_corners:
        x, y = x * W / (W - 1) - 0.5, y * H / (H - 1) - 0.5
    return x, y


def warp_forward_ref(src, M, dsize, align_corners, inverse_map=False, dst_dtype=None, **mut):
    B, Cc, H, W = src.shape
    sx, sy = warp_coords(M, H, W, dsize[0], dsize[1], align_corners, inverse_map)
    if "coords" in mut:
        sx, sy = mut["coords"](sx, sy)
    R = sample(src, sx, sy, taps=mut.get("taps"))
    R["store"] = storage(R["ref"], dst_dtype, ~R["dead"])
    R["sx"], R["sy"] = sx, sy
    return R


def warp_forward_fp32(src, M, dsize, align_corners, inverse_map=False):
    """The same operation evaluated in fp32 by torch on the CPU: coordinates rounded once, weights and taps in fp32 (the kernel's order)."""
    B, Cc, H, W = src.shape
    sx, sy = warp_coords(M, H, W, dsize[0], dsize[1], align_corners, inverse_map)
    sx, sy = sx.float(), sy.float()
    fx0, fy0 = torch.floor(sx), torch.floor(sy)
    wx1, wy1 = sx - fx0, sy - fy0
    wx0, wy0 = 1 - wx1, 1 - wy1
    x0, y0 = fx0.clamp(-2, W).long(), fy0.clamp(-2, H).long()
    flat = F.pad(src.float(), (2, 2, 2, 2)).flatten(2)
    out = torch.zeros((B, Cc, sx.shape[1] * sx.shape[2]))
    for dy, dx in ((0, 0), (0, 1), (1, 0), (1, 1)):
        w = ((wx1 if dx else wx0) * (wy1 if dy else wy0)).reshape(B, 1, -1)
        xi, yi = x0 + dx, y0 + dy
        ok = ((xi >= 0) & (xi < W) & (yi >= 0) & (yi < H)).reshape(B, 1, -1)
        out = out + torch.gather(flat, 2, ((yi + 2) * (W + 4) + xi + 2).reshape(B, 1, -1).expand(-1, Cc, -1)) * w * ok
    return out.reshape(B, Cc, *sx.shape[1:])


def _scatter(shape, g, x0, y0, dx, dy, weight):
    B, Cc, H, W = shape
    xi, yi = x0 + dx, y0 + dy
    ok = ((xi >= 0) & (xi < W) & (yi >= 0) & (yi < H)).reshape(B, 1, -1)
    idx = (yi.clamp(0, H - 1) * W + xi.clamp(0, W - 1)).reshape(B, 1, -1).expand(-1, Cc, -1)
    out = torch.zeros((B, Cc, H * W), dtype=g.dtype)
    return out.scatter_add_(2, idx, g.reshape(B, Cc, -1) * (weight(xi, yi).reshape(B, 1, -1) * ok).to(g.dtype)).reshape(shape)


def warp_backward_ref(shape, g, M, align_corners, inverse_map=False):
    """Source gradient of the warp, the fp64 transpose through tent weights, with the bar of the module docstring."""
    B, Cc, H, W = shape
    Ho, Wo = g.shape[-2:]
    sx, sy = warp_coords(M, H, W, Ho, Wo, align_corners, inverse_map)
    fin = torch.isfinite(sx) & torch.isfinite(sy) & (sx.abs() < 1e8) & (sy.abs() < 1e8)
    sxc, syc = torch.where(fin, sx, -10.0), torch.where(fin, sy, -10.0)
    x0, y0 = torch.floor(sxc).clamp(-4, W + 2).long(), torch.floor(syc).clamp(-4, H + 2).long()
    g64 = g.double()
    ref, S, n, coord = (torch.zeros(shape, dtype=torch.float64) for _ in range(4))
    tent = lambda xi, yi: (1 - (sxc - xi).abs()).clamp_min(0) * (1 - (syc - yi).abs()).clamp_min(0)
    reach = 1 + 2.0 ** -20
    near = lambda xi, yi: (((sxc - xi).abs() <= reach) & ((syc - yi).abs() <= reach)).double()
    amp = (sxc.abs().clamp_min(1) + syc.abs().clamp_min(1)).unsqueeze(1)
    ones = torch.ones_like(g64)
    for dy in (-1, 0, 1, 2):
        for dx in (-1, 0, 1, 2):
            if dx in (0, 1) and dy in (0, 1):
                ref += _scatter(shape, g64, x0, y0, dx, dy, tent)
                S += _scatter(shape, g64.abs(), x0, y0, dx, dy, tent)
                n += _scatter(shape, ones, x0, y0, dx, dy, lambda xi, yi: torch.ones_like(sxc))
            coord += _scatter(shape, g64.abs() * amp, x0, y0, dx, dy, near)
    return {"ref": ref, "unit": n.sqrt() * U24 * S, "store": K_C_WARP * U24 * coord, "S": S, "n": n}


def warp_backward_fp32(shape, g, M, align_corners, inverse_map=False):
    """The scatter evaluated in fp32 by torch on the CPU (coordinates rounded once, fp32 weights, fp32 sums in index order)."""
    B, Cc, H, W = shape
    sx, sy = warp_coords(M, H, W, g.shape[-2], g.shape[-1], align_corners, inverse_map)
    sx, sy = sx.float(), sy.float()
    fx0, fy0 = torch.floor(sx), torch.floor(sy)
    wx1, wy1 = sx - fx0, sy - fy0
    x0, y0 = fx0.clamp(-4, W + 2).long(), fy0.clamp(-4, H + 2).long()
    out = torch.zeros(shape)
    for dy, dx in ((0, 0), (0, 1), (1, 0), (1, 1)):
        w = (wx1 if dx else 1 - wx1) * (wy1 if dy else 1 - wy1)
        out = out + _scatter(shape, g.float(), x0, y0, dx, dy, lambda xi, yi: w)
    return out


# ------------------------------------------------------------------------------------------------------------------ warp cases
def _affine(B, scale=1.0, shift=(0.0, 0.0), persp=0.0, name="m"):
    """B different fp32 matrices: a mild rotation / scale / shift (+ projective terms), image 0 and image 1 differ."""
    out = []
    for b in range(B):
        t = 0.05 + 0.04 * b
        c, s = math.cos(t) * scale, math.sin(t) * scale
        out.append([[c, -s, shift[0] + 1.7 * b], [s, c * (1.02 + 0.03 * b), shift[1] - 0.9 * b], [persp * (1 + b), -persp * 0.5, 1.0]])
    return torch.tensor(out, dtype=torch.float32)


def _shift(B, tx, ty):
    m = torch.eye(3).repeat(B, 1, 1)
    for b in range(B):
        m[b, 0, 2], m[b, 1, 2] = tx + b, ty - b
    return m


# tag: (B, C, (H, W), (Ho, Wo), align_corners, inverse_map, layout, 16-bit?, matrix).  Ratios measured on an MI355X (max over elements of
# (|err| - storage / coordinate term) / unit bound; the bar is 1 for dst, C_BAR for dsrc) are in profiles/glue_parity.json and, rounded, in
# [brackets].  dsrc 0.000: the whole error sits inside the coordinate term
WARP = {
    # fast path (planar fp32, C == 3).  Wo = 300: blockIdx.x = 1 with 44 of 256 lanes live; Ho = 38 = 9 * 4 + 2: a partial block of rows
    "fast_wide_ac":   (2, 3, (37, 300), (38, 300), True, False, "nchw", False, lambda B: _affine(B, 1.01, (-3.3, 1.2), 2e-5)),   # [dst 0.465; dsrc 0.000]
    "fast_wide":      (2, 3, (37, 300), (38, 300), False, False, "nchw", False, lambda B: _affine(B, 0.99, (-2.6, 1.4), 2e-5)),   # [dst 0.433; dsrc 0.000]
    "fast_tiny":      (2, 3, (2, 2), (3, 5), False, False, "nchw", False, lambda B: _affine(B, 1.3, (0.4, 0.2))),     # smallest legal source; [dst 0.092; dsrc 0.000]
    # generic kernel: pixel stride 3 (channels-last), C == 1, 16-bit source and destination at C = 128
    "nhwc_c3":        (2, 3, (21, 40), (20, 41), False, False, "nhwc", False, lambda B: _affine(B, 1.05, (1.5, 0.5), 1e-4)),   # [dst 0.380]
    "c1":             (2, 1, (7, 9), (8, 8), True, False, "nchw", False, lambda B: _affine(B, 0.9, (0.5, 0.5), 1e-3)),   # [dst 0.160]
    "c128_h16":       (2, 128, (9, 11), (9, 11), False, False, "nhwc", True, lambda B: _affine(B, 1.1, (0.7, -0.6), 1e-3)),   # [dst bf16 0.000 / f16 0.034]
    # a whole-pixel shift + 0.5 (align_corners=True, an exact inverse): every weight is 1/2 and a tap leaves exactly on the image border
    "shift":          (2, 3, (6, 7), (6, 7), True, False, "nchw", False, lambda B: _shift(B, 2.5, -1.5)),   # [dst 0.000; dsrc 0.000]
    "off_frame":      (2, 3, (6, 7), (5, 6), True, False, "nchw", False, lambda B: _shift(B, 40.5, 3.0)),       # all taps outside: zeros, exactly; [dst 0.000]
    # inverse_map with a horizon between columns 20 and 21: Z = (ox - 20.5) / 64, |Z| >= 2^-7, |sx| up to 444
    "horizon":        (2, 3, (12, 40), (12, 40), True, True, "nchw", False,
                       lambda B: torch.tensor([[[0.3, 0.0, -3.0], [6 / 64, 0.05, -6 * 20.5 / 64 - 0.3], [1 / 64, 0.0, -20.5 / 64]],
                                               [[0.25, 0.02, -2.0], [5 / 64, 0.06, -5 * 20.5 / 64 - 0.4], [1 / 64, 0.0, -20.5 / 64]]])),   # [dst 0.312; dsrc 0.000]
    # one launch, Ho * Wo = 532900 > 2048 * 256: the generic kernel's loop runs a second time (2082 blocks wanted, 2048 launched).  grid_for caps
    # a launch at 2048 blocks, so a launch that iterates twice always has a block count that IS a multiple of 8: xcd_remap with nb % 8 != 0 and
    # nb > 8 cannot be met in the same launch and has the case "c1_45_blocks" below (and the backward of fast_wide: 45 blocks)
    "grid_stride":    (1, 1, (730, 730), (730, 730), False, False, "nchw", False, lambda B: _affine(B, 1.0, (0.3, -0.2), 1e-6)),   # [dst 0.460]
    # generic forward kernel, B = 1, C = 1: Ho * Wo = 11400 -> 45 blocks, not a multiple of 8 and more than 8: xcd_remap's ragged tail
    "c1_45_blocks":   (1, 1, (37, 300), (38, 300), False, False, "nchw", False, lambda B: _affine(B, 0.98, (-1.9, 0.8), 3e-5)),   # [dst 0.423]
    # backward only: 4:1 down-scaling (64x64 destination gradient into a 16x16 source): 16 destination pixels per cell, 64 atomics
    "down4":          (2, 3, (16, 16), (64, 64), True, True, "nchw", False,
                       lambda B: torch.tensor([[[0.25, 0, 0.1], [0, 0.25, 0.2], [0, 0, 1.0]], [[0.24, 0.01, 0.3], [0.0, 0.26, -0.2], [0, 0, 1.0]]])),   # [dsrc 0.000]
}
WARP_FWD = [t for t in WARP if t != "down4"]
WARP_BWD = ["fast_wide_ac", "fast_wide", "shift", "horizon", "fast_tiny", "down4"]


@functools.lru_cache(maxsize=None)
def warp_operands(tag):
    B, Cc, (H, W), (Ho, Wo), ac, inv, layout, h16, mat = WARP[tag]
    return {"src": grid16(f"warp.{tag}.s", (B, Cc, H, W)), "M": mat(B), "g": grid16(f"warp.{tag}.g", (B, Cc, Ho, Wo))}


@functools.lru_cache(maxsize=None)
def warp_reference(tag, dst_dtype=None):
    B, Cc, (H, W), dsize, ac, inv, layout, h16, mat = WARP[tag]
    o = warp_operands(tag)
    return warp_forward_ref(o["src"], o["M"], dsize, ac, inv, dst_dtype)


@functools.lru_cache(maxsize=None)
def warp_backward_reference(tag):
    B, Cc, (H, W), dsize, ac, inv, layout, h16, mat = WARP[tag]
    o = warp_operands(tag)
    return warp_backward_ref((B, Cc, H, W), o["g"], o["M"], ac, inv)


# ================================================================================================================== upsample4
# (B, C, H, W); measured [y f32 / bf16 / f16; dz f32 / bf16]
UPSAMPLE = {
    "v8":     (2, 128, 6, 5),       # 16-bit, C % 8 == 0: eight channels a thread; [y 0.178 / 0.125 / 0.116; dz 0.511 / 0.000]
    "scalar": (2, 12, 6, 5),        # element-wise kernel; [y 0.164 / 0.095 / 0.095; dz 0.458 / 0.000]
    "1x1":    (1, 8, 1, 1),         # ry = rx = 0; [y 0.000 / 0.000 / 0.000; dz 0.000 / 0.000]
    "1x7":    (1, 8, 1, 7),         # ry = 0; [y 0.122 / 0.042 / 0.012; dz 0.145 / 0.000]
    "7x1":    (1, 8, 7, 1),         # rx = 0; [y 0.200 / 0.042 / 0.000; dz 0.177 / 0.000]
    "stride": (1, 64, 24, 24),      # 16 B H W C = 589824 > 524288 work items in the element-wise forward (fp32): its loop runs a second time.  The v8 forward
                                    # has 73728 and the backward B H W C = 36864 here: their loops have the case LOOPS below; [y 0.107 / 0.033 / 0.044; dz 1.339 / 0.038]
}
# the grid-stride loops of upsample4_fwd_v8_kernel (16 B H W C / 8 = 1114112 work items) and upsample4_bwd_kernel (B H W C = 557056) run a second
# time: many channels on a small map, since the backward's bar counts no coordinate rounding (see upsample_reference) and |s| stays below 17.
# One 16-bit forward and one fp32 backward, in one test
UPSAMPLE_LOOPS = {"loops": (2, 1024, 16, 17)}     # [y bf16 0.103; dz f32 1.832]
# upsample4_cat: (Cz, Cy) -> yps = Cz + Cy, yco = Cz for the copied half: multiples of 8 (vector kernels) and not; [y f32 / bf16 / f16; dz f32 / bf16]
CAT = {"c8": (16, 8),               # [y 0.170 / 0.064 / 0.071; dz 0.376 / 0.000]
       "odd": (12, 5)}              # [y 0.157 / 0.022 / 0.033; dz 0.389 / 0.000]


def _lerp_matrix(n):
    """(4n, n) interpolation matrix of one axis, the 0/1 matrix of the outputs within 1 + 2^-20 of each cell, and max(1, |s|) per output."""
    s = torch.arange(4 * n, dtype=torch.float64) * ((n - 1) / (4 * n - 1))
    i0 = torch.floor(s).clamp(max=n - 1).long()
    l = s - i0
    Wm = torch.zeros((4 * n, n), dtype=torch.float64)
    Wm.scatter_add_(1, i0.unsqueeze(1), (1 - l).unsqueeze(1))
    Wm.scatter_add_(1, (i0 + 1).clamp(max=n - 1).unsqueeze(1), l.unsqueeze(1))
    reach = ((s.unsqueeze(1) - torch.arange(n, dtype=torch.float64)).abs() <= 1 + 2.0 ** -20).double()
    return Wm, reach, s.clamp_min(1.0)


@functools.lru_cache(maxsize=None)
def upsample_reference(tag, dtype=None):
    B, Cc, H, W = UPSAMPLE[tag] if tag in UPSAMPLE else UPSAMPLE_LOOPS[tag] if tag in UPSAMPLE_LOOPS else (2, CAT[tag][0], 6, 5)
    z = grid16(f"up.{tag}.z", (B, Cc, H, W))
    g = grid16(f"up.{tag}.g", (B, Cc, 4 * H, 4 * W))
    oy, ox = torch.meshgrid(torch.arange(4 * H, dtype=torch.float64), torch.arange(4 * W, dtype=torch.float64), indexing="ij")
    sy = (oy * ((H - 1) / (4 * H - 1))).expand(B, -1, -1)
    sx = (ox * ((W - 1) / (4 * W - 1))).expand(B, -1, -1)
    fwd = sample(z, sx, sy, pad="edge", k_c=K_C_UP)
    fwd["store"] = storage(fwd["ref"], dtype)
    zz = z.double().requires_grad_()
    up = F.interpolate(zz, scale_factor=4, mode="bilinear", align_corners=True)
    assert float((up.detach() - fwd["ref"]).abs().max()) < 1e-12            # the sampler restates nn.UpsamplingBilinear2d
    (dz,) = torch.autograd.grad(up, zz, g.double())
    (Sz,) = torch.autograd.grad(up, zz, g.double().abs())
    # sqrt(n) = 8: a gather of at most 8 x 8 terms; the device is held to C_BAR of this unit (+ 16-bit storage).  The weights of those terms come
    # from fp32 coordinates, which the unit does not count: "coord" is the coordinate term of the warp's backward, |d(wx wy)| <= wy |dsx| + wx |dsy|
    # with |ds| <= K_C_UP 2^-24 max(1, |s|) summed over the outputs within reach of the cell, and only the CPU check of torch's fp32 backward
    # against ONE unit adds it.  (Without it torch's own fp32 backward reaches 3.57 of the unit bound at 24 x 24, where |s| is up to 23, and 0.77 at 6 x 5.)
    Wy, Iy, ay = _lerp_matrix(H)
    Wx, Ix, ax = _lerp_matrix(W)
    ga = g.double().abs()
    coord = Wy.T @ (ga * ax) @ Ix + Iy.T @ (ga * ay.reshape(-1, 1)) @ Wx
    bwd = {"ref": dz, "unit": 8.0 * U24 * Sz, "store": storage(dz, dtype), "coord": K_C_UP * U24 * coord}
    return {"z": z, "g": g, "fwd": fwd, "bwd": bwd}


# =============================================================================================================== spatial max
# (B, C, HW, with a gradient?): C % 64 != 0, C % 8 != 0 (scalar loads inside the vector kernel), one pixel, the route switch at HW = 256
SPATIAL = {"72x63": (2, 72, 63, True), "20x5": (2, 20, 5, True), "64x1": (1, 64, 1, True), "960x63": (2, 960, 63, True),
           "72x256": (2, 72, 256, False), "20x300": (1, 20, 300, False), "64x255": (1, 64, 255, False)}


@functools.lru_cache(maxsize=None)
def spatial_operands(tag):
    """x (B, C, HW) on the 1/16 grid (65 levels: ties in most channels) with four special channels: 0 all negative, 1 negative with a maximum
    of +0.0, 2 equal to -0.0 at every pixel, 3 negative except the LAST pixel (the last, partial pixel block of the split form)."""
    B, Cc, HW, _ = SPATIAL[tag]
    x = grid16(f"smax.{tag}.x", (B, Cc, HW))
    neg = -x.abs() - 0.0625
    x[:, 0] = neg[:, 0]
    x[:, 1] = neg[:, 1]
    x[:, 1, HW // 2] = 0.0
    x[:, 1, HW - 1] = 0.0
    x[:, 2] = -0.0
    x[:, 3] = neg[:, 3]
    x[:, 3, HW - 1] = 0.5
    return x, grid16(f"smax.{tag}.g", (B, Cc), zero_below=0.0)


def spatial_max_ref(x, leaky):
    """(values fp32, argmax int64) of x (B, C, HW): the maximum and the LOWEST pixel index that attains it (-0.0 == +0.0)."""
    x = x.float()
    mx = x.amax(2)
    HW = x.shape[2]
    arg = torch.where(x == mx.unsqueeze(2), torch.arange(HW), HW).amin(2)
    return (torch.where(mx > 0, mx, LEAK * mx) if leaky else mx), arg


def spatial_max_backward_ref(g, out, arg, HW, leaky, dtype):
    """dx (B, HW, C) as stored in ``dtype``: g (one fp32 product with 0.01f where leaky and out <= 0) at the arg-max pixel, +0 elsewhere."""
    gv = torch.where(out > 0, g, LEAK * g) if leaky else g
    dx = torch.zeros((g.shape[0], HW, g.shape[1]))
    dx.scatter_(1, arg.unsqueeze(1), gv.unsqueeze(1))
    return dx.to(dtype)


# ============================================================================================= pooled linear, softmax over K
# (B, N); measured [y dp dw db; mix_weights]: the operands' products and sums are exact in fp32, so 0.000 is expected of a correct kernel
POOLED = {
    "3x960": (3, 960),              # the model's shape; [0.000 0.000 0.000 0.000; 0.000]
    "9x100": (9, 100),              # two sample blocks, the second with one sample; per = 13: the n + u < n1 tail; 100 = 3 * 32 + 4: clamped columns; [0.000 0.000 0.000 0.000; 0.006]
    "8x5":   (8, 5),                # per = 1, the n-slices 5 - 7 start past N; [0.000 0.000 0.000 0.000; 0.000]
    "17x33": (17, 33),              # three sample blocks, per = 5, two column blocks with one live column in the second; [0.000 0.000 0.000 0.000; 0.014]
}
SOFTMAX = {"5x192": (5, 192),       # [weights / dlogits] [0.441 / 0.904]
           "3x7": (3, 7)}           # [0.000 / 0.618]


def _sum_ref(ref, S, n):
    return {"ref": ref, "unit": math.sqrt(n) * U24 * S}


@functools.lru_cache(maxsize=None)
def pooled_reference(tag):
    B, N = POOLED[tag]
    p, g = grid16(f"pl.{tag}.p", (B, N)), grid16(f"pl.{tag}.g", (B, N))
    w, b = grid16(f"pl.{tag}.w", (N, N)) / 16, grid16(f"pl.{tag}.b", (N,))
    p64, g64, w64, b64 = p.double(), g.double(), w.double(), b.double()
    return {"p": p, "g": g, "w": w, "b": b,
            "y": _sum_ref(p64 @ w64.T + b64, p64.abs() @ w64.abs().T + b64.abs(), N + 1),
            "dp": _sum_ref(g64 @ w64, g64.abs() @ w64.abs(), N),
            "dw": _sum_ref(g64.T @ p64, g64.abs().T @ p64.abs(), B),
            "db": _sum_ref(g64.sum(0), g64.abs().sum(0), B)}


def softmax_logits(tag, B=2):
    """(B, K*M) logits on the 1/16 grid (differences exact in fp32), channel k*M + m; column 0: K equal logits; column 1: a spread of 80."""
    K, M = SOFTMAX[tag]
    l = (grid16(f"sm.{tag}.l", (B, K, M)) * 2).clone()
    l[:, :, 0] = 1.25
    l[:, :, 1] = torch.linspace(-40, 40, K).reshape(1, K)
    return l.reshape(B, K * M)


def softmax_ref(logits, K, M, logit_unit=None):
    """softmax over K.  unit = sqrt(K) 2^-24 w (the K-term denominator); expf is folded in once per weight as "store" = 2^-23 w; an error of the logits
    (``logit_unit``, mix_weights) moves a weight by at most w * 2 max_k |dl_k|."""
    B = logits.shape[0]
    w = torch.softmax(logits.double().reshape(B, K, M), 1)
    unit = math.sqrt(K) * U24 * w
    if logit_unit is not None:
        unit = unit + w * 2 * logit_unit.reshape(B, K, M).amax(1, keepdim=True)
    return {"ref": w.reshape(B, K * M), "unit": unit.reshape(B, K * M), "store": (2.0 ** -23 * w).reshape(B, K * M)}


def softmax_backward_ref(w, g, K, M):
    """dl_k = w_k (g_k - sum_j g_j w_j) on the weights the forward SAVED (an operand, like the conv tests' saved y)."""
    B = w.shape[0]
    w, g = w.double().reshape(B, K, M), g.double().reshape(B, K, M)
    dot, adot = (g * w).sum(1, keepdim=True), (g * w).abs().sum(1, keepdim=True)
    return {"ref": (w * (g - dot)).reshape(B, K * M), "unit": (math.sqrt(K + 1) * U24 * w.abs() * (g.abs() + adot)).reshape(B, K * M)}


# ================================================================================================================= reductions
# (n, pointer offset in elements); measured [sum]
SUM_LOG2 = {
    "n1":        (1, 0),            # the scalar tail alone; [0.044]
    "n3":        (3, 0),            # [0.094]
    "n1027":     (1027, 0),         # 256 16-byte lanes + a tail of 3, two blocks; [0.181]
    "unaligned": (4096, 1),         # pointer off by one element: n4 = 0, everything through the scalar loop; [0.174]
    "n300000":   (300000, 0),       # 75000 lanes of work > 128 blocks x 256; [0.172]
}
# (B, C, H, W); measured [sum_sq_diff, every layout / dtype form; sq_diff_backward]
SQ_DIFF = {
    "50x100": (1, 3, 50, 100),      # 5 blocks: 1160 lanes take one trip of the 4-pixel loop, 360 pixels are left to the remainder loop; [0.000; 0.805]
    "2x2":    (1, 3, 2, 2),         # remainder loop only; [0.000; 0.601]
    "c5":     (1, 5, 9, 7),         # generic loop, no flush; [0.000; 0.805]
    "c19":    (1, 19, 9, 7),        # the c & 7 flush twice + a tail of 3; [0.000; 0.805]
    "big":    (2, 3, 600, 500),     # 600000 pixels > 512 x 256 x 4: every lane takes one trip, 75712 pixels in the remainder loop; 3.6 M gradient elements; [0.000; 0.805]
}


@functools.lru_cache(maxsize=None)
def likelihoods(tag):
    n, off = SUM_LOG2[tag]
    u = synthetic._uniform(f"glue.lik.{tag}", (n + off,), 0.0, 1.0)
    return (1e-9 + u * u).clamp(max=1.0).float()                # likelihoods in [1e-9, 1], dense near 0 and near 1


def sum_log2_ref(lik):
    l2 = torch.log2(lik.double())
    return {"ref": l2.sum().reshape(1), "unit": (U_LOG * l2.abs().clamp_min(U24).sum()).reshape(1)}


@functools.lru_cache(maxsize=None)
def sq_diff_operands(tag):
    shape = SQ_DIFF[tag]
    return grid16(f"sq.{tag}.a", shape), grid16(f"sq.{tag}.b", shape)


def remainder_pixels(npix):
    """Pixel indices the C == 3 form of sum_sq_diff leaves to its remainder loop: lane p takes four pixels a trip while p + 3 * stride < npix.
    This restates the block rule of hesic_sum_sq_diff / hesic_rd_sums in csrc/glue.hip (grid_for(npix, 256 * 4, 512): 256 lanes, 1024 pixels a
    block, at most 512 blocks); a comment at the launcher points here.  If that rule changes, this function and the counts that
    tests/test_glue_ref_cpu.py holds must change with it, or they stop describing the kernel."""
    stride = min(512, -(-npix // 1024)) * 256                     # grid_for(npix, 256 * 4, 512) blocks of 256 lanes
    p = torch.arange(min(stride, npix))
    trips = torch.where(p + 3 * stride < npix, (npix - 1 - 3 * stride - p) // (4 * stride) + 1, 0)
    first = p + trips * 4 * stride
    rest = torch.cat([first + k * stride for k in range(4)])
    return rest[rest < npix]


def sum_sq_diff_ref(a, b, drop=None):
    d2 = (a.double() - b.double()) ** 2
    B, Cc, H, W = a.shape
    s = d2.sum()
    if drop is not None:
        s = s - d2.permute(0, 2, 3, 1).reshape(-1, Cc)[drop].sum()
    return {"ref": s.reshape(1), "unit": ((2.0 ** -23 * Cc + 2.0 ** -52 * B * H * W) * d2.sum()).reshape(1)}


def elementwise_ref(ref, roundings=1):
    """An fp32 map with ``roundings`` correctly rounded operations per element."""
    return {"ref": ref, "unit": roundings * U24 * ref.abs()}

"""fp64 reference with a per-element error model for the fused conv + (I)GDN kernels (a plain module, not a conftest): the image stage
(3 -> 128 5x5 s2, csrc/sconv.hip), the wide stages (Cout = 128, the fused epilogue of csrc/conv_igemm.hip) and the 6 -> 3 cat stage with its
3-channel (I)GDN (``sconv_6to3_s1_kernel``).  It composes tests/conv_grad_ref.py (the conv) and tests/gdn_ref.py (the (I)GDN).

The 16-bit kernels compute v = conv(x, w) + b in fp32 on operands rounded to the format, square the fp32 v, round the squares and gamma' to
16 bit for the contraction (``pack_sq2``; the f16 build scales by 2^-6 / 2^6), form y = v rsqrt(n) | v sqrt(n) in fp32 and round y on store.
In training they also store v in 16 bit (``y_pre``).  So, all in fp64:

  v64, S_v   the conv on exactly the operands the kernel multiplies (x and w rounded RNE to the format, fp32 bias) and the same map on
             absolute values; n_v = Cin KH KW.
  Rg         gdn_ref.reference(v64 as (P, 128), None, beta, gamma, inverse), parameters from gdn_ref.params (clamped, negative and
             at-bound entries).
  unit_g     gdn_ref.bars(Rg, fmt)["y"]: the 16-bit C = 128 regime plus the fp32 unit.
  push       the conv's own fp32 error dv = sqrt(n_v) 2^-24 S_v carried through the (I)GDN to first order:
             push = r dv + 1/2 |y| / n ((2 |v| dv) @ gamma'^T).
  y is accepted where |got - ref| <= C_BAR (unit_g + push) + extra_g; where S_v == 0 (no bias, an all-zero receptive field) y and v must
  be exactly 0.  ``y_pre`` is a plain conv output: conv_grad_ref.check with y16 = True and the format's u / h.

The cat stage computes in fp32 throughout, so gdn_ref's fp32 regime (C = 3) stands in the same composition:
  mode 0  plain conv of the two halves:                    8 sqrt(150) 2^-24 S
  mode 1  (I)GDN on the conv output:                       8 (unit_g + push)
  mode 2  (I)GDN on the first tensor in front of the conv: 8 (unit_g(xa) pushed through |w| + sqrt(150) 2^-24 S), S formed on |IGDN(xa)|
A bf16 second tensor is an operand, not a rounding.  No element is left out of a comparison; there is no share cap; C_BAR = 8.

``emulate`` evaluates the chain in fp64 with exactly the by-design roundings and, with ``mut``, one deliberate defect on one tile or halo line
(tests/test_fused_gdn_ref_cpu.py: the emulation stays below C_BAR / 2, every defect leaves the bar at every position it is applied to).

Code paths that the cases below run for the first time outside whole-model tests: the fast image kernel's tile loop (a wave's second and
third tile, requested while the previous one computes, tile indices that cross an image in mid-loop), its in-kernel weight / gamma' gather
(``w_img == NULL``), the ``<h16_t>`` image form, ``y_pre`` of every variant, and the fused epilogue at each pixel tile (32 / 64 / 128) and in
``igemm_tr4_kernel<GDN, HALO>`` for both HALO values.  No case needed a kernel change.

Ratios measured on an MI355X (max over elements of (|err| - extra)+ / unit) are recorded in profiles/fused_gdn_parity.json and, rounded, in
[brackets] behind each case as  y bf16 / y f16 / y_pre."""
import functools
import math

import torch

import conv_grad_ref as G
import gdn_ref as GR

C_BAR = G.C_BAR
U24 = G.U24
FMT = GR.FMT
FORMATS = ("bf16", "f16")


def both(t):
    """``t`` rounded so that bf16 AND f16 hold it exactly (the f16 rounding of a bf16 value only drops low bits): one fp64 conv per case."""
    return t.to(torch.bfloat16).float().to(torch.float16).float()


def rnd(t, fmt):
    """fp32 ``t`` rounded RNE to the format, as fp32."""
    return t if fmt == "f32" else t.to(FMT[fmt]["dtype"]).float()


def to_pc(t):
    """(B, C, H, W) in any memory format -> (P, C), pixel major."""
    return t.permute(0, 2, 3, 1).reshape(-1, t.shape[1])


def from_pc(t, shape):
    B, C, H, W = shape
    return t.reshape(B, H, W, C).permute(0, 3, 1, 2)


# ------------------------------------------------------------------------------------------------------------------------ the case tables
# image stage: tag -> (B, H, W), form, options.  form: "fast" (fp32 planar, even W; the wrapper prepacks the weight image), "null_img" (the
# same kernel through hesic_sconv2d_gdn_forward: in-kernel gather), "f32" (generic <float>: odd W or NHWC), "h16" (generic <h16_t>).
IMAGE = {
    "img_2x2":        ((1, 2, 2), "fast", {}),                            # one pixel, every halo row a poisoned offset; [y 0.909 / 0.938]
    "img_6x6":        ((1, 6, 6), "fast", {}),                            # the ix0 + 4 < W edge; [y 0.973 / 0.938]
    "img_50x70":      ((2, 50, 70), "fast", {"ypre": True}),              # odd Ho, partial 16-column tiles; [y 0.990 / 0.985 y_pre 0.010]
    "img_130x34":     ((3, 130, 34), "fast", {}),                         # [y 0.988 / 0.986]
    "img_trips3":     ((3, 5600, 6), "fast", {"guard": True}),            # 4200 wave tiles of 2 x 3 pixels: three trips, images end in mid-loop; [y 0.993 / 0.985]
    "img_trips2":     ((2, 368, 368), "fast", {"guard": True, "ypre": True}),      # 2208 tiles: the second trip; [y 1.002 / 1.001 y_pre 0.021]
    "img_null_img":   ((2, 50, 70), "null_img", {}),                      # [y 0.987 / 0.981]
    "img_odd":        ((1, 51, 71), "f32", {"ypre": True}),               # odd W: the 64-bit gather; [y 0.988 / 0.969 y_pre 0.001]
    "img_nhwc":       ((2, 50, 70), "f32", {"nhwc": True}),               # [y 0.987 / 0.975]
    "img_h16":        ((2, 50, 70), "h16", {}),                           # [y 0.987 / 0.982]
    "img_h16_nhwc":   ((2, 50, 70), "h16", {"nhwc": True}),               # [y 0.986 / 0.982]
    "img_zero":       ((2, 50, 70), "fast", {"bias": False, "zero_corner": 40}),   # exact zeros where the receptive field is all zero; [y 0.986 / 0.980]
    "img_unrounded":  ((2, 50, 70), "fast", {"unrounded": True}),         # fp32 image and weights: pins RNE of the in-kernel rounding; [y 0.988 / 0.987]
    "img_v300":       ((2, 50, 70), "fast", {"w_scale": 256.0, "inverse": (False,)}),     # |v| around 300: the f16 range scaling (GDN); [y 1.008 / 0.965]
}
IMAGE_TRIPS = {"img_trips3": 3, "img_trips2": 2}

# wide stage: tag -> (Cin, k, stride, transposed, (B, H, W) of the input, planned (pixel tile, cout tile, K step, family), options).
# ``plan`` is what hesic_conv2d_variant answers (family 1 = igemm_glds_kernel, 2 = igemm_tr4_kernel); ``pf`` the phase-fusion mode the case
# sets.  Every row runs conv + GDN / deconv + IGDN, ``cross`` rows also the other (I)GDN; every row also runs with y_pre (bf16).
WIDE = {
    "w_c128_t32":     (128, 5, 2, 0, (2, 40, 24), (32, 128, 128, 1), {"cross": True, "guard": True}),      # [y 0.960 / 0.842 y_pre 0.000]
    "w_c192_t32":     (192, 5, 2, 0, (1, 20, 36), (32, 128, 64, 1), {"bias": False}),      # deep ring; [y 0.930 / 0.759 y_pre 0.000]
    "w_c32_t64":      (32, 3, 2, 0, (1, 20, 36), (64, 128, 32, 1), {"guard": True}),       # deep ring; [y 0.970 / 0.951 y_pre 0.000]
    "w_c64_t64":      (64, 3, 2, 0, (2, 222, 226), (64, 128, 64, 1), {"bias": False}),     # 448 blocks of 64 px, 224 of 128 px; ragged; [y 0.995 / 0.967 y_pre 0.003]
    "w_c32_t128":     (32, 3, 2, 0, (3, 254, 258), (128, 128, 32, 1), {"guard": True}),    # 432 blocks of 128 px; ragged; [y 0.991 / 0.989 y_pre 0.007]
    "w_c64_t128":     (64, 3, 2, 0, (3, 254, 258), (128, 128, 64, 1), {"bias": False}),    # [y 0.990 / 0.963 y_pre 0.005]
    "w_d192_t32":     (192, 5, 2, 1, (1, 12, 20), (32, 128, 64, 1), {}),                   # deep ring; [y 0.956 / 0.891 y_pre 0.000]
    "w_d32_t64":      (32, 5, 2, 1, (1, 12, 20), (64, 128, 32, 1), {}),                    # [y 0.992 / 0.957 y_pre 0.000]
    "w_d64_t64":      (64, 5, 2, 1, (2, 48, 64), (64, 128, 64, 1), {}),                    # [y 0.985 / 0.963 y_pre 0.003]
    "w_d64_t128":     (64, 5, 2, 1, (2, 64, 96), (128, 128, 64, 1), {"pf": 0}),            # four phase blocks per tile; [y 0.987 / 0.962 y_pre 0.003]
    "w_d128_tr4h":    (128, 5, 2, 1, (1, 12, 20), (128, 128, 64, 2), {"pf": 2, "cross": True, "guard": True}),      # igemm_tr4_kernel<., 1>; [y 0.971 / 0.919 y_pre 0.000]
    "w_d128_tr4h_r":  (128, 5, 2, 1, (1, 9, 17), (128, 128, 64, 2), {"pf": 2}),                                     # ragged halo patch; [y 0.974 / 0.906 y_pre 0.001]
    "w_d64_tr4":      (64, 5, 2, 1, (1, 12, 20), (128, 128, 64, 2), {"pf": 2, "guard": True, "bias": False}),       # igemm_tr4_kernel<., 0>; [y 0.977 / 0.932 y_pre 0.001]
}

# cat stage: tag -> (B, H, W), layout ("pp": planar fp32 + planar fp32, "nb": NHWC fp32 + planar bf16), mode (0 plain conv, 1 GDN on the
# conv output, 2 IGDN on the first tensor in front of the transposed conv).  Measured, modes 0 / 1 / 2:
#   17x130 pp [y 0.239 / 0.209 / 0.221]   17x130 nb [y 0.216 / 0.162 / 0.192]   16x128 pp [y 0.215 / 0.176 / 0.238]
#   16x128 nb [y 0.238 / 0.229 / 0.240]   17x131 pp [y 0.224 / 0.187 / 0.218]
CAT = {}
for _hw, _lay in (((17, 130), "pp"), ((17, 130), "nb"), ((16, 128), "pp"), ((16, 128), "nb"), ((17, 131), "pp")):
    for _mode in (0, 1, 2):
        CAT["cat_%dx%d_%s_m%d" % (_hw + (_lay, _mode))] = ((2,) + _hw, _lay, _mode)
CAT_GUARD = "cat_17x130_nb_m2"


def image_tiles(shape):
    """``sconv_gdn_launch``'s arithmetic: (wave tiles of 2 x 16 output pixels, blocks of 8 waves, tiles a launch covers per trip)."""
    B, H, W = shape
    Ho, Wo = G.out_hw(H, W, 5, 2, 2, False)
    tiles = ((Wo + 15) // 16) * ((Ho + 1) // 2) * B
    grid = min((tiles + 7) // 8, 256)
    return tiles, grid, grid * 8


def wide_ring_is_deep(tag):
    """``igemm_plan``'s ring-depth rule for a case's planned tile: a 4-deep ring where every block of the grid still fits in LDS at once."""
    Cin, k, s, tr, (B, H, W), (bm, bn, _, _), _ = WIDE[tag]
    QH, QW = (H, W) if tr else G.out_hw(H, W, k, s, k // 2, False)
    tw = 16
    while tw > 1 and tw // 2 >= QW:
        tw //= 2
    tw = min(32 if (bm == 128 and QW >= 32 and QH < 8) else tw, bm)
    th = bm // tw
    nblocks = (128 // bn) * -(-QW // tw) * -(-QH // th) * B * (s * s if tr else 1)
    if bm == 32 and Cin % 128 == 0:                      # the BK = 128 form of the 32-pixel tile has one ring depth, 2
        return False
    bk = 64 if Cin % 64 == 0 else 32
    fits = -(-nblocks // 256) * 4 * (bm + bn) * bk * 2 <= 160 * 1024
    return fits if bm < 128 else (bk == 32 and fits)


def wide_desc(tag):
    """The fields of a wide case's descriptor: (B, H, W, Cin, Ho, Wo, 128, k, stride, pad, transposed)."""
    Cin, k, s, tr, (B, H, W), _, _ = WIDE[tag]
    Ho, Wo = G.out_hw(H, W, k, s, k // 2, bool(tr))
    return B, H, W, Cin, Ho, Wo, 128, k, s, k // 2, tr


# ------------------------------------------------------------------------------------------------------------------------ operands
def _signed(name, shape):
    """Both signs in +-2, exact zeros where |x| < 0.25 (conv_grad_ref.operands' inputs)."""
    x = G.synthetic._uniform(name, shape, -2, 2)
    return torch.where(x.abs() < 0.25, torch.zeros(()), x)


@functools.lru_cache(maxsize=4)
def operands(tag):
    """fp32 tensors of a case.  x and w hold values both 16-bit formats represent (``both``) unless the case is ``unrounded``; the bias is
    plain fp32 in +-0.5 (large enough that leaving it out of the squares shows); beta, gamma from gdn_ref.params."""
    name = "fgp." + tag + "."
    if tag in CAT:
        (B, H, W), lay, mode = CAT[tag]
        tr = mode == 2
        xa, xb = _signed(name + "xa", (B, 3, H, W)), both(_signed(name + "xb", (B, 3, H, W)))
        w = G.synthetic._uniform(name + "w", (6, 3, 5, 5) if tr else (3, 6, 5, 5), -1, 1) * 0.2
        b = G.synthetic._uniform(name + "b", (3,), -0.5, 0.5)
        beta, gamma = GR.params(3, 1)
        return {"xa": xa, "xb": xb, "w": w, "b": b, "beta": beta, "gamma": gamma}
    if tag in IMAGE:
        (B, H, W), form, opt = IMAGE[tag]
        Cin, k, s, tr = 3, 5, 2, False
    else:
        Cin, k, s, tr, (B, H, W), _, opt = WIDE[tag]
    fan = Cin * k * k / (s * s if tr else 1)
    x = _signed(name + "x", (B, Cin, H, W))
    w = G.synthetic._uniform(name + "w", (Cin, 128, k, k) if tr else (128, Cin, k, k), -1, 1) * (3.0 / fan) ** 0.5 * opt.get("w_scale", 1.0)
    if not opt.get("unrounded"):
        x, w = both(x), both(w)
    if opt.get("zero_corner"):
        x[:, :, :opt["zero_corner"], :opt["zero_corner"]] = 0
    b = G.synthetic._uniform(name + "b", (128,), -0.5, 0.5) if opt.get("bias", True) else None
    beta, gamma = GR.params(128, 3)
    return {"x": x, "w": w, "b": b, "beta": beta, "gamma": gamma}


def geometry(tag):
    """(stride, pad, transposed) of an image or wide case."""
    if tag in IMAGE:
        return 2, 2, False
    _, k, s, tr, _, _, _ = WIDE[tag]
    return s, k // 2, bool(tr)


def inverses(tag):
    """Which (I)GDN directions a case runs."""
    if tag in IMAGE:
        return IMAGE[tag][2].get("inverse", (False, True))
    tr = bool(WIDE[tag][3])
    return (False, True) if WIDE[tag][6].get("cross") else (tr,)


# ------------------------------------------------------------------------------------------------------------------------ the reference
def conv_part(x, w, b, *, stride, pad, transposed, fmt):
    """v64 and S_v on the operands the kernel multiplies (x, w rounded RNE to ``fmt``; "f32": as they are), and n_v."""
    x64, w64 = rnd(x, fmt).double(), rnd(w, fmt).double()
    b64 = None if b is None else b.double()
    op = stride - 1 if transposed else None
    v = G._conv(x64, w64, b64, stride, pad, transposed, op)
    S = G._conv(x64.abs(), w64.abs(), None if b64 is None else b64.abs(), stride, pad, transposed, op)
    Cin = w.shape[0] if transposed else w.shape[1]
    return {"v": v, "S": S, "n": Cin * w.shape[-1] * w.shape[-2], "x": x64, "w": w64, "b": b64, "geom": (stride, pad, transposed)}


def _push(Rg, v_pc, dv_pc):
    """dv carried through the (I)GDN to first order."""
    y = Rg["ref"]["y"].abs()
    return Rg["r"] * dv_pc + 0.5 * y / Rg["n"] * ((2 * v_pc.abs() * dv_pc) @ Rg["gp"].abs().T)


def fuse(Rc, beta, gamma, inverse, fmt):
    """The fused reference of a conv part: {"ref", "bar" (unit, extra), "dead", "shape", "Rg", "conv"}; "conv" is the conv_grad_ref-style
    reference of the stored conv output."""
    v_pc, S_pc = to_pc(Rc["v"]), to_pc(Rc["S"])
    Rg = GR.reference(v_pc, None, beta, gamma, inverse)
    unit_g, extra_g = GR.bars(Rg, fmt)["y"]
    dead = S_pc == 0
    unit = unit_g + _push(Rg, v_pc, math.sqrt(Rc["n"]) * U24 * S_pc)
    zero = torch.zeros((), dtype=torch.float64)
    f = FMT[fmt]
    conv = {"ref": {"y": Rc["v"]}, "S": {"y": Rc["S"]}, "n": {"y": Rc["n"]}, "y16": fmt != "f32", "dx16": True, "u16": f["u"], "h16": f["h"]}
    return {"ref": Rg["ref"]["y"], "bar": (torch.where(dead, zero, unit), torch.where(dead, zero, extra_g)), "dead": dead,
            "shape": tuple(Rc["v"].shape), "Rg": Rg, "conv": conv, "fmt": fmt, "inverse": bool(inverse)}


@functools.lru_cache(maxsize=2)
def _cached_conv(tag, fmt):
    o = operands(tag)
    s, p, tr = geometry(tag)
    return conv_part(o["x"], o["w"], o["b"], stride=s, pad=p, transposed=tr, fmt=fmt)


def case_conv(tag, fmt):
    """The conv part of an image or wide case: shared by both formats (the operands are exact in both) unless the case is unrounded."""
    unr = tag in IMAGE and IMAGE[tag][2].get("unrounded")
    return _cached_conv(tag, fmt if unr else "bf16")


def reference_of(tag, fmt, inverse):
    o = operands(tag)
    return fuse(case_conv(tag, fmt), o["beta"], o["gamma"], inverse, fmt)


def check(R, got):
    """(ok, ratio, message) of a fused output ``got`` (B, C, H, W), any memory format: every element within C_BAR unit + extra, exact where
    the bar is 0."""
    return GR.check(R["ref"], R["bar"], to_pc(got.detach().cpu().double()), "y", C_BAR)


def outside(R, got_pc):
    """bool (P, C): the elements of ``got_pc`` outside their bar."""
    return GR.outside(R["ref"], R["bar"], got_pc, C_BAR)


def check_pre(R, got):
    """(ok, ratio, message) of the stored conv output."""
    return G.check(R["conv"], "y", got)


def clear_cache():
    _cached_conv.cache_clear()
    operands.cache_clear()
    cat_reference.cache_clear()


# ------------------------------------------------------------------------------------------------------------------------ the cat stage
def _gdn3(x, beta, gamma, inverse):
    """((I)GDN(x) in fp64, its fp32 unit) for a (B, 3, H, W) tensor."""
    Rg = GR.reference(to_pc(x.double()), None, beta, gamma, inverse)
    unit, _ = GR.bars(Rg, "f32")["y"]
    return from_pc(Rg["ref"]["y"], x.shape), from_pc(unit, x.shape), Rg


@functools.lru_cache(maxsize=4)
def cat_reference(tag, mut=None):
    """{"ref", "bar", "shape"} of a cat case; ``mut``: the same evaluation with one defect (no roundings to emulate: the kernel is fp32)."""
    (B, H, W), lay, mode = CAT[tag]
    o = operands(tag)
    tr = mode == 2
    xa, xb, w, b = o["xa"].double(), o["xb"].double(), o["w"].double(), o["b"].double()
    wa = w[:3].abs() if tr else w[:, :3].abs()
    zero = torch.zeros((), dtype=torch.float64)
    conv = lambda a_, b_, w_, bias: G._conv(torch.cat((a_, b_), 1), w_, bias, 1, 2, tr, 0 if tr else None)
    if mut == "halves_swapped":
        xa, xb = xb, xa
    ua = None
    if mode == 2:
        if mut == "gdn_on_second":
            xb = _gdn3(xb, o["beta"], o["gamma"], True)[0]
        else:
            xa, ua, _ = _gdn3(xa, o["beta"], o["gamma"], True)
    if mut == "pad_not_zero":                            # the padding ring of the first three staged planes holds 2^-6 instead of 0
        ring = torch.nn.functional.pad(torch.zeros_like(xa), (2, 2, 2, 2), value=2.0 ** -6)
        full = lambda t: torch.nn.functional.pad(t, (2, 2, 2, 2))
        xin = torch.cat((full(xa) + ring, full(xb)), 1)
        v = (torch.nn.functional.conv_transpose2d(xin, w, b, padding=4) if tr else torch.nn.functional.conv2d(xin, w, b))
    else:
        v = conv(xa, xb, w, b)
    S = conv(xa.abs(), xb.abs(), w.abs(), b.abs())
    dv = math.sqrt(150) * U24 * S
    if mode == 0:
        ref, unit = v, dv
    elif mode == 1:
        Rg = GR.reference(to_pc(v), None, o["beta"], o["gamma"], False)
        unit = from_pc(GR.bars(Rg, "f32")["y"][0] + _push(Rg, to_pc(v), to_pc(dv)), v.shape)
        ref = from_pc(Rg["ref"]["y"], v.shape)
    else:
        pushed = G._conv(ua, wa, None, 1, 2, tr, 0) if ua is not None else torch.zeros_like(v)
        ref, unit = v, pushed + dv
    return {"ref": to_pc(ref), "bar": (to_pc(unit), torch.zeros_like(to_pc(unit))), "shape": tuple(v.shape)}


CAT_MUTATIONS = {0: ("halves_swapped",), 1: ("halves_swapped",), 2: ("halves_swapped", "gdn_on_second", "pad_not_zero")}


# --------------------------------------------------------------------------------------------------------------- the by-design roundings
def r16(t, fmt):
    """fp64 ``t`` rounded to the storage type, back in fp64 (f16 saturates at +-65504 like ``pack_h2``)."""
    if fmt == "f16":
        t = t.clamp(-65504.0, 65504.0)
    return GR.rnd(t, fmt)


def _epilogue(v, sq_of, Rg, fmt, inverse, *, beta=True, swap_slabs=False):
    """y (unrounded fp64) of the fused epilogue on conv outputs ``v`` (P, C) whose squares are taken of ``sq_of``."""
    gp, bp = Rg["gp"], Rg["bp"]
    sq = sq_of * sq_of
    if fmt == "f16":                                     # the range scaling: squares 2^-6, gamma' 2^6
        sq16, gp16 = r16(sq / 64.0, fmt) * 64.0, r16(gp * 64.0, fmt) / 64.0
    else:
        sq16, gp16 = r16(sq, fmt), r16(gp, fmt)
    if swap_slabs:                                       # the K permutation: two 16-channel slabs of gamma' change places
        gp16 = gp16.clone()
        gp16[:, 0:16], gp16[:, 16:32] = gp16[:, 16:32].clone(), gp16[:, 0:16].clone()
    n = sq16 @ gp16.T + (bp if beta else 0.0)
    return v * (n.sqrt() if inverse else n.rsqrt()), n


def emulate(Rc, R, fmt):
    """(y, y_pre) as (P, C) fp64 tensors holding the stored values: the by-design roundings and nothing else."""
    v = to_pc(Rc["v"])
    y, _ = _epilogue(v, v, R["Rg"], fmt, R["inverse"])
    return r16(y, fmt), r16(v, fmt)


MUTATIONS = ("unwritten_tile", "tile_late", "drop_halo_col", "first_row_in_image", "bias_out_of_squares", "beta_missing", "slabs_swapped",
             "n_from_neighbour", "gdn_for_igdn", "ypre_is_y", "ypre_from_y_rows")
TILE_MUTATIONS = tuple(m for m in MUTATIONS if m not in ("drop_halo_col", "first_row_in_image"))
TILE_LATE_STRIDE = 16            # "tile_late": how many wave tiles earlier the rows a tile computes from were requested


def image_tile_pixels(shape_out, t):
    """Pixel rows (in (P, C) order) of wave tile ``t`` of the image kernels, with their (row, column) inside the 2 x 16 tile."""
    B, _, Ho, Wo = shape_out
    tx_n, ty_n = (Wo + 15) // 16, (Ho + 1) // 2
    tx, ty, b = t % tx_n, (t // tx_n) % ty_n, t // (tx_n * ty_n)
    out = {}
    for r in range(2):
        for c in range(16):
            oy, ox = ty * 2 + r, tx * 16 + c
            if oy < Ho and ox < Wo:
                out[(r, c)] = (b * Ho + oy) * Wo + ox
    return out


def mutate(Rc, R, fmt, mut, where):
    """``emulate``'s (y, y_pre) with one defect.  Tile mutations: ``where`` is a wave-tile index of the image kernels; halo mutations: ``where``
    is ignored (the line is fixed by the geometry).  Returns (y, y_pre, mask (P,) of the pixels the defect touches)."""
    v = to_pc(Rc["v"])
    Rg, inverse, shape = R["Rg"], R["inverse"], R["shape"]
    B, C, Ho, Wo = shape
    y, pre = emulate(Rc, R, fmt)
    y, pre = y.clone(), pre.clone()
    touched = torch.zeros(v.shape[0], dtype=torch.bool)
    if mut in ("drop_halo_col", "first_row_in_image"):
        x, w, b = Rc["x"], Rc["w"], Rc["b"]
        H, W = x.shape[-2:]
        v4 = Rc["v"].clone()
        if mut == "drop_halo_col":                       # tap column kx = 4 of the pixels whose ix0 + 4 is the last image column
            assert W % 2 == 1
            ox = (W - 1 - 2) // 2
            col = torch.nn.functional.conv2d(x[..., W - 1:W], w[..., 4:5], None, stride=(2, 1), padding=(2, 0))
            v4[..., ox:ox + 1] -= col
            sel = torch.zeros(B, Ho, Wo, dtype=torch.bool)
            sel[:, :, ox] = True
        else:                                            # output row 0: the two rows above the image read as rows H - 2, H - 1
            row = torch.nn.functional.conv2d(x[..., H - 2:H, :], w[..., 0:2, :], None, stride=(1, 2), padding=(0, 2))
            v4[..., 0:1, :] += row
            sel = torch.zeros(B, Ho, Wo, dtype=torch.bool)
            sel[:, 0, :] = True
        vm = to_pc(v4)
        ym, _ = _epilogue(vm, vm, Rg, fmt, inverse)
        touched = sel.reshape(-1)
        y[touched], pre[touched] = r16(ym, fmt)[touched], r16(vm, fmt)[touched]
        return y, pre, touched
    pix = image_tile_pixels(shape, where)
    idx = torch.tensor(sorted(pix.values()))
    touched[idx] = True
    if mut == "unwritten_tile":
        y[idx] = 0.0
    elif mut == "tile_late":                             # the rows requested for tile ``where`` - stride are used for tile ``where``
        src = image_tile_pixels(shape, where - TILE_LATE_STRIDE)
        for rc, p in pix.items():
            y[p] = y[src[rc]] if rc in src else 0.0
    elif mut == "ypre_is_y":
        pre[idx] = y[idx]
    elif mut == "ypre_from_y_rows":                      # one 32-channel slice of the wave's LDS rows still holds y
        pre[idx, 32:64] = y[idx, 32:64]
    else:
        if mut == "bias_out_of_squares":
            ym, _ = _epilogue(v, v - Rc["b"], Rg, fmt, inverse)
        elif mut == "beta_missing":
            ym, _ = _epilogue(v, v, Rg, fmt, inverse, beta=False)
        elif mut == "slabs_swapped":
            ym, _ = _epilogue(v, v, Rg, fmt, inverse, swap_slabs=True)
        elif mut == "gdn_for_igdn":
            ym, _ = _epilogue(v, v, Rg, fmt, not inverse)
        elif mut == "n_from_neighbour":
            _, n = _epilogue(v, v, Rg, fmt, inverse)
            n = torch.roll(n, -1, 0)
            ym = v * (n.sqrt() if inverse else n.rsqrt())
        else:
            raise KeyError(mut)
        y[idx] = r16(ym, fmt)[idx]
    return y, pre, touched

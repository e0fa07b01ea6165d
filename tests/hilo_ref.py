"""fp64 reference with a per-element error model for the hi/lo ("pair", bf16x3) analysis kernels (a plain module, not a conftest): the image
stage ``n2w_gdn_hilo_kernel<INV, OUT1>`` with its weight image (csrc/sconv_hilo.hip), ``im2col_hilo_kernel`` (csrc/glue.hip), the HL = 1 / 2
main loop of ``igemm_glds_kernel`` with its GDN = 3 / 4 epilogue (also behind single operands: ``hesic_conv2d_gdn_forward_hilo_out``), the
plain pair epilogue (y_hilo, y_abs, y32, acc_scale) and ``splitk_reduce_kernel``'s pair outputs (csrc/conv_igemm.hip).  It composes
tests/conv_grad_ref.py (the conv), tests/gdn_ref.py (the (I)GDN) and tests/fused_gdn_ref.py (their fusion).

OPERANDS are what the kernels multiply.  A pair is hi = rnd16(t), lo = rnd16(t - hi), RNE; the binary16 build clamps t to +-65504 first
(``split_h2``; the image samples are not clamped: ``split2_img``).  Activations: the test builds the [hi | lo] tensor itself.  Weights: the
host split of ``PackedWeightHiLo.get`` (binary16: w 2^s split, the launch multiplies its sums by acc_scale = 2^-s).  Image and 3 -> 128
weights: the in-kernel splits replicated on the host (``image_operands``).  gamma' = t t - 2^-36 is an fp32 expression a compiler may
contract: the reference takes gamma' in fp64 and the model counts its fp32 rounding (gdn_ref's S_n), the emulation rounds the fp64 value.

CONV, in fp64, by product class (hh = x_hi w_hi, lh = x_lo w_hi, hl = x_hi w_lo):
    three products              v = acc_scale (hh + lh + hl) + b     = conv(x_hi + x_lo, w_hi + w_lo) - conv(x_lo, w_lo): lo lo is dropped by design
    two products (_w1, OUT1)    v = hh + lh + b                      = conv(x_hi + x_lo, w), w the single weights
    hilo_out                    v = hh + b                           = conv(x16, w16)
    unit_v = sqrt(n) 2^-24 S,  n = products Cin KH KW,  S the same map on absolute values (|x_hi| + |x_lo| against |w_hi| + |w_lo|, + |b|; it
    is a scale, not a value, and is summed in fp32: all its terms are positive, so it is 0 exactly where every product is 0 and 2^-20
    relative otherwise).  Where S == 0 the output must be exactly 0.  Error-feedback weights (``hesic_pack_conv_weight_shaped``, the OUT1
    image) are given 16-bit-exact values, so that the walk is the identity; ``img_walk`` has fp32 weights and replays the serpentine walk in
    fp32 on the host (``shaped_walk``).

PAIR (I)GDN.  gdn_ref's 16-bit regime with the squares and gamma' carrying their own units: u_p = u^2 for a pair (u from gdn_ref.FMT: the
lo half rounds what the hi half left), u for the single gamma' of HL = 0 / 2 and OUT1:
    dn_i^2 = sum_j (u_g gamma'_ij + h_g)^2 sq_j^2 + gamma'_ij^2 (u_p sq_j + h_s)^2,   rho = dn / n,   unit_g = unit32 + 1/2 rho |y|
    binary16 floors: h_g = 2^-25 / 64 (gamma' is packed times 64); h_s = 2^-25 4^-k per pixel, 2^k the pixel's square scaling (``DYN_SQ``:
    its largest |v| brought to [2^6, 2^7); the model takes k from a maximum 2^-16 larger, the conservative side of a binade edge); OUT1 keeps
    the fixed 2^-6: h_s = 2^-19 (its bias and beta' enter as three 16-bit terms, 2^-24 relative: inside the fp32 unit).
    The conv's own error is carried through with fused_gdn_ref._push.  Storage: u_p |ref| + h for a pair output, u |ref| + h for OUT1.

CHECKS, on every output element (no element is left out, there is no share cap; C_BAR = conv_grad_ref.C_BAR = 8):
    sum    |hi + lo - ref| <= C_BAR unit + storage; exactly 0 where S == 0
    pair   |lo| <= ulp(hi) / 2: a pair is a pair, not two unrelated halves
    abs    with y_abs: hi >= 0 and the reference is |v|
    y32    with out = "both" / "f32": |y32 - ref| <= C_BAR unit_v
    same   with out = "both" both halves are defined by the fp32 map: (hi, lo) == split(y32) (of |y32| with y_abs), bit for bit

``emulate`` evaluates the chain in fp64 with exactly the by-design roundings (the pair squares under their scaling, gamma' as a pair or a
single value, the dropped gamma'_lo sq_lo, the split of the output) and, with ``mut``, one defect on one tile: tests/test_hilo_ref_cpu.py
holds the emulation below C_BAR / 2 and every applicable defect outside the checks at every tile position it is applied to.

WHAT THE BARS CANNOT SEE (``mutations_of`` leaves these out; nothing is widened for them).  The conservative fp32 unit of a wide layer,
8 sqrt(n) 2^-24 S with n >= 576, is larger than one lost lo class on ordinary operands (n = 3200: about 0.2 of the bar), so those defects
are shown on operands built for them: the CLASS ISOLATION launches (the test owns both halves: (x_hi, 0) (w_hi, 0), (0, x_lo) (w_hi, 0),
(x_hi, 0) (0, w_lo), (0, x_lo) (0, w_lo) with ordinary-size lo halves -- each class at full magnitude, the last one exactly act(bias)),
LO-HEAVY operands for the kernels that split inside (image, gamma': lo halves near half an ulp with the sign of hi, so that a lost class
is a coherent error) and a DOMINANT channel (one output channel's weights times 32: n is one gamma' v^2 term).
    drop_xlo_whi, drop_xhi_wlo   wide layers: on the isolation operands only; image stage: on the lo-heavy cases only.
    gamma_lo_dropped             on the lo-heavy cases (gamma' lo-heavy) only: bf16 and the image stage; in binary16 behind a wide conv (2^-12 of
                                 the norm) it stays inside the conv's own fp32 unit and is not shown.
    sq_lo_dropped                on the dominant-channel cases of the strict pair form only, bf16 and the image stage: beside a single gamma'
                                 (u gamma', HL = 0 / 2 and OUT1) a lost sq_lo (u sq) is the same size as what the form rounds away by
                                 design, and in binary16 behind a wide conv 2^-13 |y| is inside the conv's own fp32 unit.
    lo_zero, lo_of_neighbour, abs_after_split
                                 a wrong lo half is an error of 2^-9 |y| (bf16) / 2^-12 |y| (binary16): shown by the sum check in bf16 and for
                                 the image stage, and bit for bit by the ``same`` check of every out = "both" case; in binary16 behind a
                                 wide conv (n >= 576) the sum check alone cannot show it (lo_of_neighbour is then still shown by ``pair``
                                 wherever the neighbour is the larger value).

Ratios measured on an MI355X (max over elements of (|err| - storage)+ / unit) are recorded in profiles/hilo_parity.json and, rounded, in
[brackets] behind each case as  bf16 / f16."""
import functools
import math

import torch
import torch.nn.functional as F

import conv_grad_ref as G
import fused_gdn_ref as Fz
import gdn_ref as GR

C_BAR = G.C_BAR
U24 = G.U24
FMT = GR.FMT
FORMATS = ("bf16", "f16")
to_pc, from_pc = Fz.to_pc, Fz.from_pc
ZERO = torch.zeros((), dtype=torch.float64)


# ------------------------------------------------------------------------------------------------------------------------ pairs
def rnd16(t, fmt, clamp=True):
    """``t`` (fp32 or fp64) rounded RNE to the 16-bit format, same dtype back; binary16 saturates at +-65504 unless ``clamp`` is off."""
    if fmt == "f16" and clamp:
        t = t.clamp(-65504.0, 65504.0)
    return t.to(FMT[fmt]["dtype"]).to(t.dtype)


def split(t, fmt, clamp=True):
    """(hi, lo) of ``t`` as ``split_h2`` forms them (``clamp`` off: ``split2_img``).  In fp32 the residual t - hi is exact."""
    if fmt == "f16" and clamp:
        t = t.clamp(-65504.0, 65504.0)
    hi = rnd16(t, fmt, False)
    return hi, rnd16(t - hi, fmt, False)


def ulp16(hi, fmt):
    """The spacing of the 16-bit format at ``hi`` (fp64): 2^(e - 7) | 2^(e - 10), e not below the smallest normal exponent."""
    bits, emin = (7, -126) if fmt == "bf16" else (10, -14)
    _, ex = torch.frexp(hi.double().abs().clamp_min(2.0 ** -140))
    return torch.ldexp(torch.ones_like(hi, dtype=torch.float64), (ex - 1).clamp_min(emin) - bits)


def pair_shift(w, fmt):
    """``functional._pair_weight_shift`` on the host: binary16 pair weights are packed times 2^s, largest |w| in [2^13, 2^14)."""
    m = float(w.abs().max())
    if fmt != "f16" or not m > 0:
        return 0
    return max(0, min(24, 13 - math.frexp(m)[1] + 1))


def shaped_walk(w, fmt, scale=1.0):
    """``pack_weight_shaped_kernel`` / the OUT1 image: w (Cout, Cin, KH, KW) fp32 times ``scale``, rounded to 16 bit with error feedback
    along the serpentine walk of each (cout, cin) pair, in fp32 as the kernels do."""
    KH, KW = w.shape[-2:]
    out = torch.empty_like(w)
    e = torch.zeros(w.shape[:2])
    for ky in range(KH):
        for j in range(KW):
            kx = KW - 1 - j if ky & 1 else j
            tgt = w[:, :, ky, kx] * scale + e
            q = rnd16(tgt, fmt)
            e = tgt - q
            out[:, :, ky, kx] = q
    return out


def lo_heavy(t, fmt, frac=0.45):
    """fp32 values whose pair has ``t``'s 16-bit rounding as hi and a lo half of ``frac`` ulp(hi) with hi's sign."""
    hi = rnd16(t.float(), fmt)
    if fmt == "f16":
        hi = torch.where(hi.abs() < 2.0 ** -10, torch.zeros(()), hi)      # binary16: a lo half of at least 7 subnormal steps
    return (hi.double() + frac * ulp16(hi, fmt) * torch.sign(hi).double()).float()


def assert_lo_heavy(t, fmt, what, frac=0.4, clamp=True):
    hi, lo = split(t, fmt, clamp)
    live = hi != 0
    assert bool(live.any()) and bool((lo[live] * hi[live] > 0).all()), f"{what}: a lo half with the wrong sign"
    assert bool((lo[live].double().abs() >= frac * ulp16(hi[live], fmt)).all()), f"{what}: a lo half below {frac} ulp"


# ------------------------------------------------------------------------------------------------------------------------ the case tables
# image stage: tag -> ((B, H, W), options).  Every case runs the pair form and OUT1; "inverse": the directions (default both).
IMAGE = {
    "img_2x2":       ((1, 2, 2), {}),                                     # one pixel, every halo row a poisoned offset; [0.019 / 0.034]
    "img_6x6":       ((1, 6, 6), {}),                                     # the ix0 + 4 < W edge; [0.012 / 0.089]
    "img_50x70":     ((2, 50, 70), {}),                                   # odd Ho, partial 16-column tiles; [0.666 / 0.430]
    "img_130x34":    ((3, 130, 34), {}),      # [0.477 / 0.484]
    "img_crop":      ((2, 50, 70), {"crop": (3, 5, 7, 9)}),               # a crop of a larger tensor: strided rows and planes; [0.513 / 0.463]
    "img_trips3":    ((3, 5600, 6), {"inverse": (False,), "guard": True}),       # 4200 wave tiles: three trips, images end in mid-loop; [0.620 / 0.524]
    "img_trips2":    ((2, 368, 368), {"inverse": (False,), "guard": True}),      # 2208 tiles: two trips; [0.725 / 0.623]
    "img_zero":      ((2, 50, 70), {"bias": False, "zero_corner": 40}),   # both halves exactly 0 where the receptive field is all zero; [0.541 / 0.326]
    "img_loheavy":   ((2, 50, 70), {"loheavy": True}),                    # x, w, gamma' with lo halves near half an ulp; [2.800 / 2.246]
    "img_dominant":  ((2, 50, 70), {"dominant": 5}),                      # channel 5's weights times 32; [0.799 / 0.741]
    "img_w256":      ((2, 50, 70), {"w_scale": 256.0, "inverse": (False,)}),     # |v| around 300: binary16 range (GDN); [0.771 / 0.538]
    "img_walk":      ((2, 50, 70), {"walk": True, "forms": ("out1",)}),   # fp32 weights: the serpentine walk replayed on the host; [0.527 / 0.502]
}
IMAGE_TRIPS = {"img_trips3": 3, "img_trips2": 2}
IMAGE_FORMS = ("pair", "out1")
KP = 96                                                                   # im2col columns: 3 * 25 = 75, padded

# im2col route: tag -> ((B, H, W), nhwc); the columns are compared bit for bit, the figures are the 1 x 1 pair conv + (I)GDN on them
IM2COL = {
    "col_51x71":     ((1, 51, 71), False),                                # odd sizes; [0.028 / 0.082]
    "col_nhwc":      ((2, 50, 70), True),                                 # NHWC image: strided planes; [0.031 / 0.124]
}

# wide pair conv + (I)GDN, Cout 128: tag -> (Cin, k, stride, (B, H, W), planned (pixel tile, cout tile, K step) for GDN, options).
# products 3 and 2 unless "products"; GDN unless "inverse"; "cross": both directions.
WIDE = {
    "w_c64_t32":     (64, 5, 2, (2, 40, 24), (32, 128, 128), {"cross": True, "guard": True}),      # [0.684 / 0.441]
    "w_c96_t32":     (96, 5, 2, (1, 20, 36), (32, 128, 64), {"bias": False}),                   # deep ring; [0.556 / 0.412]
    "w_c32_t64":     (32, 3, 2, (2, 222, 226), (64, 128, 64), {"guard": True}),      # [1.271 / 0.935]
    "w_c32_t128":    (32, 3, 2, (3, 254, 258), (128, 128, 64), {"guard": True}),      # [1.314 / 0.935]
    "w_c32_t256":    (32, 3, 2, (4, 318, 322), (256, 128, 64), {"products": (3,), "guard": True}),      # [0.036 / 0.068]
    "w_c32_t256_i":  (32, 3, 2, (4, 318, 322), (128, 128, 64), {"products": (3,), "inverse": (True,)}),     # IGDN stays on 128; [0.033 / 0.083]
    "w_c128_real":   (128, 5, 2, (1, 24, 40), (32, 128, 128), {"cross": True}),                 # the real layer's geometry; [0.551 / 0.388]
    "w_dominant":    (64, 5, 2, (2, 40, 24), (32, 128, 128), {"dominant": 5, "cross": True}),      # [0.910 / 0.628]
    "w_loheavy":     (64, 5, 2, (2, 40, 24), (32, 128, 128), {"loheavy": True, "products": (3,)}),          # gamma' lo-heavy; [0.009 / 0.020]
}
# single operands, pair epilogue (hesic_conv2d_gdn_forward_hilo_out): both directions
HILO_OUT = {
    "o_c128_t32":    (128, 5, 2, (2, 40, 24), (32, 128, 128), {}),      # [0.591 / 0.414]
    "o_c32_t64":     (32, 3, 2, (1, 20, 36), (64, 128, 32), {}),      # [0.982 / 0.754]
    "o_c32_t128":    (32, 3, 2, (3, 254, 258), (128, 128, 32), {}),      # [1.430 / 0.903]
}
# plain pair conv: tag -> (Cin, Cout, k, stride, (B, H, W), planned (pixel tile, cout tile, K step, K slices), options).
# options: act, out ("f32" | "hilo" | "both"), y_abs, products (default (3, 2)), no_split (the plan under Fn.no_split_k()), acc (explicit
# acc_scale with weights times its inverse), guard
PLAIN = {
    "p_splitk":      (128, 192, 5, 2, (2, 16, 16), (64, 64, 128, 8), {"out": "both", "y_abs": True, "guard": True, "no_split": (64, 64, 128, 1)}),      # [0.023 / 0.020]
    "p_splitk_hilo": (128, 192, 5, 2, (2, 16, 16), (64, 64, 128, 8), {"out": "hilo", "act": G.ACT_LEAKY, "products": (3,)}),      # [0.002 / 0.004]
    "p_splitk_f32":  (128, 192, 5, 2, (2, 16, 16), (64, 64, 128, 8), {"out": "f32", "products": (3,)}),      # [0.009 / 0.006]
    "p_c32_t128":    (32, 192, 3, 2, (1, 254, 258), (128, 64, 64, 1), {"out": "both", "act": G.ACT_LEAKY}),      # [0.097 / 0.111]
    "p_c96_t64":     (96, 192, 3, 2, (2, 64, 96), (64, 64, 64, 1), {"out": "both", "y_abs": True}),      # [0.058 / 0.052]
    "p_c192_relu":   (192, 128, 3, 1, (2, 8, 8), (64, 128, 64, 8), {"out": "both", "act": G.ACT_RELU}),      # [0.006 / 0.008]
    "p_c128_n256":   (128, 256, 3, 1, (1, 12, 20), (128, 128, 64, 8), {"out": "hilo", "products": (3,)}),       # two cout tiles; [0.004 / 0.008]
    "p_acc":         (64, 128, 3, 1, (1, 12, 20), (128, 128, 64, 4), {"out": "both", "acc": 0.25, "products": (3,), "fmts": ("bf16",)}),      # [0.023]
}
ISOLATION = (64, 128, 3, 1, (1, 12, 20))                                  # the four class launches, products 3 and 2
# measured, y32 and sum:  hh [0.012 / 0.016] lh [0.012 / 0.015] hl [0.010 / 0.015] ll [0.000 / 0.000]
ISO_CLASSES = ("hh", "lh", "hl", "ll")
NAMES = {False: "gdn", True: "igdn"}


def image_runs():
    return [(t, f, i) for t, (_, o) in IMAGE.items() for f in o.get("forms", IMAGE_FORMS) for i in o.get("inverse", (False, True))]


def wide_runs():
    out = []
    for t, row in WIDE.items():
        o = row[5]
        inv = (False, True) if o.get("cross") else o.get("inverse", (False,))
        out += [(t, p, i) for p in o.get("products", (3, 2)) for i in inv]
    return out


def wide_plan(tag, products, inverse):
    """The planned (pixel tile, cout tile, K step) of a wide run: the 256-pixel tile is the strict pair form's, with GDN only."""
    plan = WIDE[tag][4]
    return (128,) + plan[1:] if plan[0] == 256 and (inverse or products != 3) else plan


def hilo_out_runs():
    return [(t, i) for t in HILO_OUT for i in (False, True)]


def plain_runs():
    return [(t, p, f) for t, row in PLAIN.items() for p in row[6].get("products", (3, 2)) for f in row[6].get("fmts", FORMATS)]


# ------------------------------------------------------------------------------------------------------------------------ operands
def _params(loheavy, fmt, salt=3):
    """beta, gamma of gdn_ref.params; ``loheavy``: gamma' = max(gamma, 2^-18)^2 - 2^-36 (fp32) has a lo-heavy pair."""
    beta, gamma = GR.params(128, salt)
    if loheavy:
        gp = gamma.clamp_min(GR.GAMMA_BOUND).double() ** 2 - GR.PED
        scale = 64.0 if fmt == "f16" else 1.0                             # binary16 packs gamma' times 64: that product is what is split
        tgt = lo_heavy((gp * scale).float(), fmt).double() / scale
        heavy = tgt > 0                                                   # the clamped entries (gamma' = 0) and the tiny ones stay as they are
        gamma = torch.where(heavy, (tgt + GR.PED).sqrt().float(), gamma)
        t = gamma.clamp_min(GR.GAMMA_BOUND)
        assert int(heavy.sum()) > 128 * 64
        assert_lo_heavy(((t * t - torch.tensor(GR.PED, dtype=torch.float32)) * scale)[heavy], fmt, "gamma'")
    return beta, gamma


@functools.lru_cache(maxsize=4)
def image_operands(tag, fmt, form, scaled=True):
    """The fp32 tensors of an image case and the 16-bit-exact operands the kernel makes of them (all fp32):
    x (the tensor handed over: a view for the crop case), xh, xl, w (handed over), wh, wl (None for OUT1; unscaled), b, beta, gamma.
    ``scaled`` off: the pair image of an IGDN launch, whose binary16 weights are split as they are (``PackedN2wHiLo.get(inverse=True)``)."""
    (B, H, W), o = IMAGE[tag]
    name = "hlp." + tag + "."
    top, left, bot, right = o.get("crop", (0, 0, 0, 0))
    full = Fz._signed(name + "x", (B, 3, H + top + bot, W + left + right))
    w = G.synthetic._uniform(name + "w", (128, 3, 5, 5), -1, 1) * (3.0 / 75) ** 0.5 * o.get("w_scale", 1.0)
    if o.get("dominant") is not None:
        w[o["dominant"]] *= 32.0
    if o.get("loheavy"):
        full, w = lo_heavy(full, fmt), lo_heavy(w, fmt)
    out1 = form == "out1"
    if out1 and not o.get("walk"):
        w = Fz.both(w * 0.125) * 8.0                                      # w and w / 8 (the binary16 OUT1 image) 16-bit exact in both formats: the walk is the identity
    x = full[:, :, top:top + H, left:left + W]
    if o.get("zero_corner"):
        x[:, :, :o["zero_corner"], :o["zero_corner"]] = 0
    xh, xl = split(x.contiguous(), fmt, clamp=False)
    if out1:
        root = 0.125 if fmt == "f16" else 1.0                             # H16_SQ_ROOT: the OUT1 image holds w sqrt(H16_SQ_SCALE)
        wh, wl = shaped_walk(w, fmt, root) / root, None
        if not o.get("walk"):
            assert bool((wh == w).all())
    else:
        sc = float(2 ** pair_shift(w, fmt)) if scaled else 1.0
        wh, wl = split(w * sc, fmt)
        wh, wl = wh / sc, wl / sc
    if o.get("loheavy"):
        assert_lo_heavy(x, fmt, "x", clamp=False)
        if not out1:
            assert_lo_heavy(w * sc, fmt, "w")
    b = G.synthetic._uniform(name + "b", (128,), -0.5, 0.5) if o.get("bias", True) else None
    beta, gamma = _params(bool(o.get("loheavy")), fmt)
    return {"x": x, "full": full, "crop": (top, left), "xh": xh, "xl": xl, "w": w, "wh": wh, "wl": wl, "b": b, "beta": beta, "gamma": gamma}


def _wide_xw(name, Cin, Cout, k, shape, o, fmt):
    B, H, W = shape
    x = Fz._signed(name + "x", (B, Cin, H, W))
    w = G.synthetic._uniform(name + "w", (Cout, Cin, k, k), -1, 1) * (3.0 / (Cin * k * k)) ** 0.5
    if o.get("dominant") is not None:
        w[o["dominant"]] *= 32.0
    return x, w


def weight_halves(w, fmt, products, acc=None):
    """(wh, wl, acc_scale, w handed to the packer) of a wide weight: products 3 -> the host split of PackedWeightHiLo.get (binary16: times
    2^s, acc_scale 2^-s; ``acc``: an explicit acc_scale with the weights times its inverse and no shift of their own); 2 -> 16-bit-exact
    single weights (the error-feedback walk is the identity); 1 -> the plain 16-bit weights of the hilo_out form."""
    if products != 3:
        w16 = Fz.both(w)
        return w16, None, 1.0, w16
    if acc is not None:
        wp = w / acc
        wh, wl = split(wp, fmt)
        return wh, wl, acc, wp
    sc = float(2 ** pair_shift(w, fmt))
    wh, wl = split(w * sc, fmt)
    return wh, wl, 1.0 / sc, w


@functools.lru_cache(maxsize=4)
def wide_operands(kind, tag, fmt, products):
    """kind "wide" | "out" | "plain": x fp32 and its pair (single 16-bit values for the hilo_out form), the weight halves as the launch
    multiplies them (packed values: times 1 / acc_scale), the weight handed to the packer, b, beta, gamma."""
    row = {"wide": WIDE, "out": HILO_OUT, "plain": PLAIN}[kind][tag]
    if kind == "plain":
        Cin, Cout, k, s, shape, _, o = row
    else:
        (Cin, k, s, shape, _, o), Cout = row, 128
    name = "hlp." + tag + "."
    x, w = _wide_xw(name, Cin, Cout, k, shape, o, fmt)
    if products == 1:
        xh, xl = Fz.both(x), None
    else:
        xh, xl = split(x, fmt)
    wh, wl, acc_scale, w_given = weight_halves(w, fmt, products, o.get("acc"))
    b = G.synthetic._uniform(name + "b", (Cout,), -0.5, 0.5) if o.get("bias", True) else None
    beta, gamma = _params(bool(o.get("loheavy")), fmt) if kind != "plain" else (None, None)
    return {"xh": xh, "xl": xl, "wh": wh, "wl": wl, "acc_scale": acc_scale, "w": w_given, "b": b, "beta": beta, "gamma": gamma,
            "geom": (s, k // 2)}


@functools.lru_cache(maxsize=2)
def isolation_operands(fmt, products):
    """Hand-built halves of the isolation launches: hi halves and ordinary-size lo halves, all 16-bit exact (no relation between them)."""
    Cin, Cout, k, s, (B, H, W) = ISOLATION
    name = "hlp.iso."
    r = lambda t: rnd16(t, fmt)
    xh, xl = r(Fz._signed(name + "xh", (B, Cin, H, W))), r(Fz._signed(name + "xl", (B, Cin, H, W)))
    a = (3.0 / (Cin * k * k)) ** 0.5
    wh, wl = r(G.synthetic._uniform(name + "wh", (Cout, Cin, k, k), -a, a)), r(G.synthetic._uniform(name + "wl", (Cout, Cin, k, k), -a, a))
    b = G.synthetic._uniform(name + "b", (Cout,), -0.5, 0.5)
    return {"xh": xh, "xl": xl, "wh": wh, "wl": wl, "b": b, "geom": (s, k // 2)}


# ------------------------------------------------------------------------------------------------------------------------ the conv part
def _c64(x, w, geom):
    return F.conv2d(x.double(), w.double(), None, stride=geom[0], padding=geom[1])


def conv_part(xh, xl, wh, wl, b, geom, acc_scale=1.0):
    """The product classes in fp64 (each times acc_scale), v, S and n.  ``xl`` / ``wl`` None: that half does not exist (is not read)."""
    a = float(acc_scale)
    hh = _c64(xh, wh, geom) * a
    lh = _c64(xl, wh, geom) * a if xl is not None else None
    hl = _c64(xh, wl, geom) * a if wl is not None else None
    xa = xh.abs() + (xl.abs() if xl is not None else 0)
    wa = (wh.abs() + (wl.abs() if wl is not None else 0)) * a
    S = F.conv2d(xa.float(), wa.float(), None if b is None else b.abs().float(), stride=geom[0], padding=geom[1]).double()
    products = 1 + (xl is not None) + (wl is not None)
    R = {"hh": hh, "lh": lh, "hl": hl, "b": None if b is None else b.double(), "S": S, "n": products * wh.shape[1] * wh.shape[2] * wh.shape[3],
         "geom": geom, "x": (xh, xl), "w": (wh, wl), "acc_scale": a, "products": products}
    R["v"] = value(R)
    return R


def value(Rc, drop=()):
    """v of a conv part; ``drop``: product classes left out."""
    v = torch.zeros_like(Rc["hh"])
    for c in ("hh", "lh", "hl"):
        if Rc[c] is not None and c not in drop:
            v = v + Rc[c]
    return v if Rc["b"] is None else v + Rc["b"].view(1, -1, 1, 1)


def act64(v, act):
    if act == G.ACT_RELU:
        return torch.relu(v)
    if act == G.ACT_LEAKY:
        return torch.where(v > 0, v, v * G.LEAKY32)
    return v


# ------------------------------------------------------------------------------------------------------------------------ the pair (I)GDN
def square_floor(v_pc, fmt, gform):
    """h_s: binary16's subnormal floor of a stored square, per pixel (P, 1) (0 for bf16)."""
    if fmt != "f16":
        return torch.zeros(v_pc.shape[0], 1, dtype=torch.float64)
    if gform == "out1":
        return torch.full((v_pc.shape[0], 1), 2.0 ** -19, dtype=torch.float64)
    return 2.0 ** -25 / dyn_scale(v_pc * (1 + 2.0 ** -16)) ** 2


def dyn_scale(v_pc):
    """2^k of ``DYN_SQ``: k = 7 - ex of the pixel's largest |v| (frexp), clamped to [-24, 40]; (P, 1) fp64."""
    m = v_pc.abs().max(1, keepdim=True).values
    _, ex = torch.frexp(m)
    ex = torch.where(m == 0, torch.zeros_like(ex), ex)
    return torch.ldexp(torch.ones_like(m), (7 - ex).clamp(-24, 40))


def pair_unit(Rg, fmt, gform):
    """gdn_ref._unit16's forward term with the squares (always a pair) and gamma' (a pair in the strict form, else single) carrying their own
    units.  gform: "pair" (HL = 1, the image pair form), "single" (HL = 0 / 2), "out1" (the image OUT1 form)."""
    u = FMT[fmt]["u"]
    f16 = fmt == "f16"
    u_p = u * u
    u_g = u_p if gform == "pair" else u
    h_g = 2.0 ** -25 / 64 if f16 else 0.0
    h_s = square_floor(Rg["x"], fmt, gform)
    sq, gp, n = Rg["sq"], Rg["gp"], Rg["n"]
    dn2 = (sq ** 2) @ ((u_g * gp + h_g) ** 2).T + ((u_p * sq + h_s) ** 2) @ (gp ** 2).T
    return 0.5 * dn2.sqrt() / n * Rg["ref"]["y"].abs()


def fuse(Rc, beta, gamma, inverse, fmt, gform):
    """The fused reference of a conv part: {"ref", "bar" (unit, storage), "dead", "shape", "Rg", "Rc", ...}, (P, C) tensors."""
    v_pc, S_pc = to_pc(Rc["v"]), to_pc(Rc["S"])
    Rg = GR.reference(v_pc, None, beta, gamma, inverse)
    unit = GR._unit32(Rg)["y"] + pair_unit(Rg, fmt, gform) + Fz._push(Rg, v_pc, math.sqrt(Rc["n"]) * U24 * S_pc)
    f = FMT[fmt]
    u_out = f["u"] if gform == "out1" else f["u"] ** 2
    ref = Rg["ref"]["y"]
    dead = S_pc == 0
    return {"ref": ref, "bar": (torch.where(dead, ZERO, unit), torch.where(dead, ZERO, u_out * ref.abs() + f["h"])), "dead": dead,
            "shape": tuple(Rc["v"].shape), "Rg": Rg, "Rc": Rc, "fmt": fmt, "inverse": bool(inverse), "gform": gform, "kind": "gdn",
            "pair_out": gform != "out1", "y_abs": False, "out": "hilo"}


def plain(Rc, fmt, act, out, y_abs):
    """The reference of a plain pair launch: act(v) (|.| for the pair with y_abs), the fp32 bar and the pair's storage term."""
    v_pc, S_pc = to_pc(Rc["v"]), to_pc(Rc["S"])
    ref32 = act64(v_pc, act)
    unit = math.sqrt(Rc["n"]) * U24 * S_pc
    f = FMT[fmt]
    ref = ref32.abs() if y_abs else ref32
    return {"ref": ref, "ref32": ref32, "bar": (unit, torch.where(S_pc == 0, ZERO, f["u"] ** 2 * ref.abs() + f["h"])),
            "bar32": (unit, torch.zeros_like(unit)), "dead": S_pc == 0, "shape": tuple(Rc["v"].shape), "Rc": Rc, "fmt": fmt, "kind": "plain",
            "act": act, "out": out, "y_abs": bool(y_abs), "pair_out": out != "f32"}


# ------------------------------------------------------------------------------------------------------------------------ references by case
def image_scaled(fmt, form, inverse):
    """False where a launch's weight image differs from the GDN launch's: the binary16 pair image of an IGDN launch is not scaled."""
    return not (fmt == "f16" and form == "pair" and inverse)


@functools.lru_cache(maxsize=2)
def _image_conv(tag, fmt, form, scaled):
    o = image_operands(tag, fmt, form, scaled)
    return conv_part(o["xh"], o["xl"], o["wh"], o["wl"], o["b"], (2, 2))


def image_reference(tag, fmt, form, inverse):
    scaled = image_scaled(fmt, form, inverse)
    o = image_operands(tag, fmt, form, scaled)
    return fuse(_image_conv(tag, fmt, form, scaled), o["beta"], o["gamma"], inverse, fmt, "pair" if form == "pair" else "out1")


@functools.lru_cache(maxsize=2)
def _wide_conv(kind, tag, fmt, products):
    o = wide_operands(kind, tag, fmt, products)
    return conv_part(o["xh"], o["xl"], o["wh"], o["wl"], o["b"], o["geom"], o["acc_scale"])


def wide_reference(tag, fmt, products, inverse):
    o = wide_operands("wide", tag, fmt, products)
    R = fuse(_wide_conv("wide", tag, fmt, products), o["beta"], o["gamma"], inverse, fmt, "pair" if products == 3 else "single")
    R["plan"] = wide_plan(tag, products, inverse)
    return R


def hilo_out_reference(tag, fmt, inverse):
    o = wide_operands("out", tag, fmt, 1)
    R = fuse(_wide_conv("out", tag, fmt, 1), o["beta"], o["gamma"], inverse, fmt, "single")
    R["plan"] = HILO_OUT[tag][4]
    return R


def plain_reference(tag, fmt, products):
    o = PLAIN[tag][6]
    R = plain(_wide_conv("plain", tag, fmt, products), fmt, o.get("act", G.ACT_NONE), o.get("out", "both"), o.get("y_abs", False))
    R["ksplit"], R["plan"] = PLAIN[tag][5][3], PLAIN[tag][5][:3]
    return R


def isolation_reference(fmt, products, cls, act=G.ACT_NONE):
    """One of the four class launches: the halves named by ``cls`` ("hh", "lh", "hl", "ll"), the others zero.  Returns (R, (xh, xl, wh, wl)
    as handed to the launch).  "ll" is exactly act(bias); with two products the weight lo half is not read: "hl" and "ll" are act(bias)."""
    o = isolation_operands(fmt, products)
    z = torch.zeros_like
    xh, xl = (o["xh"], z(o["xl"])) if cls[0] == "h" else (z(o["xh"]), o["xl"])
    wh, wl = (o["wh"], z(o["wl"])) if cls[1] == "h" else (z(o["wh"]), o["wl"])
    Rc = conv_part(xh, xl, wh, wl if products == 3 else None, o["b"], o["geom"])
    R = plain(Rc, fmt, act, "both", False)
    R["plan"] = (128, 128, 64)
    return R, (xh, xl, wh, wl)


@functools.lru_cache(maxsize=2)
def im2col_operands(tag, fmt):
    """The im2col route of the image stage: x fp32 (B, 3, H, W), its column matrix as the kernel forms it -- k = (ci 5 + ky) 5 + kx, zero
    beyond 75 up to KP and outside the image, split with the clamp (``pack_h2``) -- and the 3 -> 128 weight as the 1 x 1 pair weight over
    the columns (``PackedWeightHiLo.get(as_1x1=True, kp=KP)``)."""
    (B, H, W), nhwc = IM2COL[tag]
    name = "hlp." + tag + "."
    x = Fz._signed(name + "x", (B, 3, H, W))
    Ho, Wo = G.out_hw(H, W, 5, 2, 2, False)
    cols = F.unfold(x, 5, padding=2, stride=2).reshape(B, 75, Ho, Wo)
    cols = torch.cat((cols, torch.zeros(B, KP - 75, Ho, Wo)), 1)
    ch, cl = split(cols, fmt)
    w = G.synthetic._uniform(name + "w", (128, 3, 5, 5), -1, 1) * (3.0 / 75) ** 0.5
    w1 = torch.cat((w.reshape(128, 75), torch.zeros(128, KP - 75)), 1).reshape(128, KP, 1, 1)
    wh, wl, acc_scale, _ = weight_halves(w1, fmt, 3)
    b = G.synthetic._uniform(name + "b", (128,), -0.5, 0.5)
    beta, gamma = _params(False, fmt)
    return {"x": x, "nhwc": nhwc, "ch": ch, "cl": cl, "w": w, "wh": wh, "wl": wl, "acc_scale": acc_scale, "b": b, "beta": beta, "gamma": gamma}


IM2COL_PLAN = (32, 128, 64)


def im2col_reference(tag, fmt, inverse):
    """The 1 x 1 pair conv + (I)GDN on the host's columns."""
    o = im2col_operands(tag, fmt)
    Rc = conv_part(o["ch"], o["cl"], o["wh"], o["wl"], o["b"], (1, 0), o["acc_scale"])
    R = fuse(Rc, o["beta"], o["gamma"], inverse, fmt, "pair")
    R["plan"] = IM2COL_PLAN
    return R


def clear_cache():
    for f in (image_operands, wide_operands, isolation_operands, im2col_operands, _image_conv, _wide_conv):
        f.cache_clear()


# ------------------------------------------------------------------------------------------------------------------------ the checks
def halves(got, C):
    """(hi, lo) as (P, C) fp64 of a [hi(C) | lo(C)] map (B, 2C, H, W), any memory format."""
    g = to_pc(got.detach().cpu().double())
    return g[:, :C], g[:, C:]


def _ratio(err, unit, extra):
    over = (err - extra).clamp_min(0)
    return torch.where(unit > 0, over / unit.clamp_min(1e-300), torch.where(over > 0, torch.full_like(over, float("inf")), torch.zeros_like(over)))


def elementwise(R, out):
    """{check: (bad (P, C) bool, ratio (P, C))} of outputs ``out`` = {"hi", "lo"} | {"y"} (+ "y32"), (P, C) fp64 tensors.  A check's ratio is
    in units of its own bound: C_BAR for "sum" and "y32", 1 for "pair", 0 for "abs" and "same"."""
    res = {}
    fmt = R["fmt"]
    if R["pair_out"] or "y" in out:
        got = out["hi"] + out["lo"] if R["pair_out"] else out["y"]
        r = _ratio((got - R["ref"]).abs(), *R["bar"])
        r = torch.where(torch.isnan(got), torch.full_like(r, float("inf")), r)
        res["sum"] = (~(r <= C_BAR), r)
    if R["pair_out"]:
        r = out["lo"].abs() / (0.5 * ulp16(out["hi"], fmt))
        res["pair"] = (~(r <= 1.0), r)
        if R["y_abs"]:
            res["abs"] = (out["hi"] < 0, (out["hi"] < 0).double())
    if "y32" in out:
        r = _ratio((out["y32"] - R["ref32"]).abs(), *R["bar32"])
        r = torch.where(torch.isnan(out["y32"]), torch.full_like(r, float("inf")), r)
        res["y32"] = (~(r <= C_BAR), r)
        if R["pair_out"]:
            t = out["y32"].float()
            hi, lo = split(t.abs() if R["y_abs"] else t, fmt)
            bad = (hi.double() != out["hi"]) | (lo.double() != out["lo"])
            res["same"] = (bad, bad.double())
    return res


def check(R, out):
    """{check: (ok, largest ratio, message)} over every element."""
    res = {}
    for q, (bad, r) in elementwise(R, out).items():
        msg = ""
        if bool(bad.any()):
            w = int(torch.argmax(torch.where(bad, r, torch.full_like(r, -1.0))))
            p, c = divmod(w, r.shape[1])
            msg = f"{q}: {int(bad.sum())} of {bad.numel()} elements fail; worst ratio {float(r.reshape(-1)[w]):.4g} at pixel {p} channel {c}: " \
                  f"ref {float(R['ref'].reshape(-1)[w]):.9g} " + " ".join(f"{k} {float(t.reshape(-1)[w]):.9g}" for k, t in out.items())
        res[q] = (not bool(bad.any()), float(r.max()), msg)
    return res


def rows_of(R, out, rows):
    """(R, out) restricted to the pixel rows ``rows`` (an index tensor or bool mask): what ``elementwise`` reads, nothing else."""
    Rs = dict(R)
    Rs["ref"], Rs["bar"] = R["ref"][rows], tuple(t[rows] for t in R["bar"])
    if "ref32" in R:
        Rs["ref32"], Rs["bar32"] = R["ref32"][rows], tuple(t[rows] for t in R["bar32"])
    return Rs, {k: t[rows] for k, t in out.items()}


def outside(R, out, rows=None):
    """bool per pixel (of ``rows`` when given): an element of it fails a check."""
    if rows is not None:
        R, out = rows_of(R, out, rows)
    bad = torch.zeros(R["ref"].shape[0], dtype=torch.bool)
    for b, _ in elementwise(R, out).values():
        bad |= b.any(1)
    return bad


# --------------------------------------------------------------------------------------------------------------- the by-design roundings
def pair64(t, fmt):
    """(hi, lo) of an fp64 value as the stored pair, fp64."""
    if fmt == "f16":
        t = t.clamp(-65504.0, 65504.0)
    hi = GR.rnd(t, fmt)
    return hi, GR.rnd(t - hi, fmt)


def _norm(v, Rg, fmt, gform, *, gamma_lo=True, sq_lo=True):
    """n of the pair epilogue on conv outputs ``v`` (P, C): the squares as pairs under their scaling, gamma' as a pair (strict form) or single,
    gamma'_lo sq_lo dropped."""
    gp, bp = Rg["gp"], Rg["bp"]
    f16 = fmt == "f16"
    if f16 and gform != "out1":
        c = dyn_scale(v)
        sh, sl = pair64((v * c) ** 2, fmt)
        sh, sl = sh / c ** 2, sl / c ** 2
    elif f16:
        sh, sl = pair64(v * v / 64.0, fmt)
        sh, sl = sh * 64.0, sl * 64.0
    else:
        sh, sl = pair64(v * v, fmt)
    g = 64.0 if f16 and gform != "out1" else 1.0                          # the OUT1 image holds gamma' plain: its conv values carry the scale
    gh, gl = pair64(gp * g, fmt)
    gh, gl = gh / g, gl / g
    if not sq_lo:
        sl = torch.zeros_like(sl)
    n = (sh + sl) @ gh.T + bp
    if gform == "pair" and gamma_lo:
        n = n + sh @ gl.T
    return n


def _store(R, y, y32=None):
    fmt = R["fmt"]
    if not R["pair_out"]:
        return {"y": Fz.r16(y, fmt)} if y32 is None else {"y32": y32}
    hi, lo = pair64(y, fmt)
    out = {"hi": hi, "lo": lo}
    if y32 is not None:
        out["y32"] = y32
    return out


def _chain(R, v, **kw):
    """The outputs a launch stores for conv outputs ``v`` (P, C)."""
    fmt = R["fmt"]
    if R["kind"] == "gdn":
        n = _norm(v, R["Rg"], fmt, R["gform"], **kw)
        return _store(R, v * (n.sqrt() if R["inverse"] else n.rsqrt()))
    y32 = act64(v.float().double(), R["act"]).float().double()            # the accumulator, then 0.01f * v, are fp32 values
    y32_out = y32 if R["out"] in ("f32", "both") else None
    return _store(R, y32.abs() if R["y_abs"] else y32, y32_out)


def emulate(R, fmt=None, mut=None, where=0):
    """The outputs evaluated in fp64 with exactly the roundings the launch makes by design and, with ``mut``, one defect on tile ``where``
    (``tiles(R)``).  Returns the outputs, and with ``mut`` also the bool (P,) mask of the pixels the defect touches."""
    assert fmt is None or fmt == R["fmt"]
    Rc = R["Rc"]
    out = _chain(R, to_pc(Rc["v"]))
    if mut is None:
        return out
    return mutate(R, out, mut, where)


MUTATIONS = ("unwritten_tile", "tile_late", "drop_halo_col", "drop_xlo_whi", "drop_xhi_wlo", "gamma_lo_dropped", "sq_lo_dropped", "halves_swapped",
             "lo_of_neighbour", "lo_zero", "scale_after_bias", "abs_after_split", "kslice_dropped")
TILE_LATE_STRIDE = 16


def _tiles(R, plan):
    plan = R.get("plan") if plan is None else plan
    cache = R.setdefault("_tiles", {})
    if plan not in cache:
        cache[plan] = tiles(R, plan)
    return cache[plan]


def _full(R, key, fn):
    """A mutation's full-map outputs, evaluated once per reference."""
    cache = R.setdefault("_full", {})
    if key not in cache:
        cache[key] = fn()
    return cache[key]


def tiles(R, plan=None):
    """The pixel tiles of a launch as a list of (pixel index tensor, channel slice).  Image stage (``plan`` None): wave tiles of 2 x 16 output
    pixels; implicit GEMM: ``plan`` = (pixel tile, cout tile) with igemm_plan's TH x TW patch."""
    B, C, Ho, Wo = R["shape"]
    if plan is None:
        n = ((Wo + 15) // 16) * ((Ho + 1) // 2) * B
        return [(torch.tensor(sorted(Fz.image_tile_pixels(R["shape"], t).values())), slice(0, C)) for t in range(n)]
    bm, bn = plan[:2]
    tw = 16
    while tw > 1 and tw // 2 >= Wo:
        tw //= 2
    tw = min(32 if (bm == 128 and Wo >= 32 and Ho < 8) else tw, bm)
    th = bm // tw
    out = []
    for b in range(B):
        for ty in range(-(-Ho // th)):
            for tx in range(-(-Wo // tw)):
                oy, ox = torch.meshgrid(torch.arange(ty * th, min(ty * th + th, Ho)), torch.arange(tx * tw, min(tx * tw + tw, Wo)), indexing="ij")
                pix = ((b * Ho + oy) * Wo + ox).reshape(-1)
                out += [(pix, slice(n0, min(n0 + bn, C))) for n0 in range(0, C, bn)]
    return out


def positions(n):
    """The tile positions a mutation is applied to: the first, a middle one and the last (all of them up to 8 tiles)."""
    return list(range(n)) if n <= 8 else [0, n // 2 + 1, n - 1]


def mutations_of(R, flags=()):
    """The mutations a reference has; ``flags``: what its operands were built for ("loheavy", "dominant", "isolation").  See the module
    docstring for what is left out and why."""
    kind, fmt, pair, Rc = R["kind"], R["fmt"], R["pair_out"], R["Rc"]
    image = kind == "gdn" and Rc["hh"].shape[1] == 128 and Rc["w"][0].shape[1] == 3
    small_n = image or fmt == "bf16"
    same = "both" == R["out"] and pair and kind == "plain"
    out = ["unwritten_tile", "tile_late", "drop_halo_col"]
    if "loheavy" in flags and image or "isolation" in flags:
        out += ["drop_xlo_whi"] if Rc["lh"] is not None else []
        out += ["drop_xhi_wlo"] if Rc["hl"] is not None else []
    if kind == "gdn":
        if R["gform"] == "pair" and "loheavy" in flags and small_n:
            out.append("gamma_lo_dropped")
        if "dominant" in flags and R["gform"] == "pair" and small_n:
            out.append("sq_lo_dropped")
    if pair:
        out.append("halves_swapped")
        if small_n or same:
            out += ["lo_of_neighbour", "lo_zero"]
    if Rc["acc_scale"] != 1.0 and Rc["b"] is not None:
        out.append("scale_after_bias")
    if R["y_abs"] and (small_n or same):
        out.append("abs_after_split")
    if R.get("ksplit", 1) > 1:
        out.append("kslice_dropped")
    return out


def _last_column_part(Rc):
    """What the last input column contributes to v: (delta (B, C, Ho, Wo'), first output column it covers)."""
    s, p = Rc["geom"]
    (xh, xl), (wh, wl) = Rc["x"], Rc["w"]
    W = xh.shape[-1]
    k = wh.shape[-1]
    w0 = s * max(0, (W - 2 * k) // s)
    last = lambda t: torch.cat((torch.zeros_like(t[..., w0:W - 1]), t[..., W - 1:]), -1)
    d = _c64(last(xh), wh, Rc["geom"])
    if xl is not None:
        d = d + _c64(last(xl), wh, Rc["geom"])
    if wl is not None:
        d = d + _c64(last(xh), wl, Rc["geom"])
    return d * Rc["acc_scale"], w0 // s


def mutate(R, out, mut, where, plan=None):
    """``out`` (``emulate``'s) with one defect on tile ``where`` of ``tiles(R, plan)``; ``plan`` defaults to R["plan"].  Returns (outputs, touched)."""
    Rc, fmt = R["Rc"], R["fmt"]
    v = to_pc(Rc["v"])
    pix, cs = _tiles(R, plan)[where]
    touched = torch.zeros(v.shape[0], dtype=torch.bool)
    touched[pix] = True
    out = {k: t.clone() for k, t in out.items()}

    def put(new):
        for k in out:
            out[k][pix, cs] = new[k][pix, cs]

    if mut == "unwritten_tile":
        for k in out:
            out[k][pix, cs] = 0.0
    elif mut == "tile_late":                              # the tile holds what an earlier tile's pixels computed
        all_tiles = _tiles(R, plan)
        assert len(all_tiles) > 1, "tile_late needs a second tile"
        per_pix = max(1, R["shape"][1] // (cs.stop - cs.start))             # cout tiles of the same pixels are neighbours in the list
        step = TILE_LATE_STRIDE * per_pix
        src, _ = all_tiles[where - step if where >= step else (where + per_pix) % len(all_tiles)]
        assert len(all_tiles) > per_pix, "tile_late needs a second pixel tile"
        for k in out:
            rows = out[k][src[torch.arange(len(pix)) % len(src)]]
            out[k][pix, cs] = rows[:, cs]
    elif mut == "drop_halo_col":                          # the last input column is not read (the tile is ignored: the line is the geometry's)
        d, c0 = _full(R, "last_col", lambda: _last_column_part(Rc))

        def dropped():
            v4 = Rc["v"].clone()
            v4[..., c0:] -= d
            return _chain(R, to_pc(v4))
        new = _full(R, mut, dropped)
        sel = torch.zeros(R["shape"][0], R["shape"][2], R["shape"][3], dtype=torch.bool)
        sel[..., c0:] = (d != 0).any(1)
        touched = sel.reshape(-1)
        for k in out:
            out[k][touched] = new[k][touched]
    elif mut in ("drop_xlo_whi", "drop_xhi_wlo"):
        put(_full(R, mut, lambda: _chain(R, to_pc(value(Rc, drop=("lh",) if mut == "drop_xlo_whi" else ("hl",))))))
    elif mut == "gamma_lo_dropped":
        put(_full(R, mut, lambda: _chain(R, v, gamma_lo=False)))
    elif mut == "sq_lo_dropped":
        put(_full(R, mut, lambda: _chain(R, v, sq_lo=False)))
    elif mut == "halves_swapped":
        out["hi"][pix, cs], out["lo"][pix, cs] = out["lo"][pix, cs].clone(), out["hi"][pix, cs].clone()
    elif mut == "lo_of_neighbour":
        if v.shape[0] == 1:                               # a one-pixel map: the neighbouring channel's
            out["lo"][pix, cs] = torch.roll(out["lo"][pix], 1, 1)[:, cs]
        else:
            nb = pix[(torch.arange(len(pix)) + 1) % len(pix)] if len(pix) > 1 else (pix + 1) % v.shape[0]
            out["lo"][pix, cs] = out["lo"][nb][:, cs]
    elif mut == "lo_zero":
        out["lo"][pix, cs] = 0.0
    elif mut == "scale_after_bias":                       # acc_scale (conv + b) in the place of acc_scale conv + b
        b = Rc["b"].view(1, -1)
        put(_full(R, mut, lambda: _chain(R, v - b + b * Rc["acc_scale"])))
    elif mut == "abs_after_split":                        # the split of v, then |.| of each half
        hi, lo = _full(R, mut, lambda: pair64(act64(v.float().double(), R["act"]).float().double(), fmt))
        out["hi"][pix, cs], out["lo"][pix, cs] = hi.abs()[pix, cs], lo.abs()[pix, cs]
    elif mut == "kslice_dropped":                         # the last K slice's partial tile never reaches the sum: the last taps of the walk
        (xh, xl), (wh, wl) = Rc["x"], Rc["w"]
        taps = wh.shape[-1] * wh.shape[-2]
        first = taps - max(1, taps // R["ksplit"])
        keep = torch.zeros(taps)
        keep[first:] = 1.0
        keep = keep.view(1, 1, wh.shape[-2], wh.shape[-1])
        d = _c64(xh, wh * keep, Rc["geom"])
        if xl is not None:
            d = d + _c64(xl, wh * keep, Rc["geom"])
        if wl is not None:
            d = d + _c64(xh, wl * keep, Rc["geom"])
        put(_chain(R, v - to_pc(d) * Rc["acc_scale"]))
    else:
        raise KeyError(mut)
    return out, touched

"""fp64 reference with a per-element error model for the 32-channel enhancement kernels of hesic_amd/csrc/enh.hip (a plain module, not a
conftest): c32_conv3x3_kernel (bf16 / f16 NHWC and fp32 planar forms), c32_conv6_kernel, pack_images_c32_kernel, c32_resblock_r3_kernel and
c32_wgrad_kernel + c32_wgrad_finish_kernel.  Built on tests/conv_grad_ref.py (``reference``, ``bars``, ``check``, ``C_BAR = 8``) and on the
format table of tests/gdn_ref.py.

One conv (``conv_reference``):  ref = act(conv(x, w) + b) + r1 + r2 in fp64 on exactly the operands the kernel multiplies -- x and the
residuals at 16-bit values, w rounded to the 16-bit format as the kernels do when they load it, the bias and a planar residual in fp32.  S_e is the
same map on absolute values (|b|, |r1|, |r2| included), n = 288 (54 for the 6-channel input layer), and

    bar_e = 8 sqrt(n) 2^-24 S_e + u |ref_e| (+ h)       u = 2^-8 (bf16) or 2^-11 (f16, h = 2^-25) for a 16-bit output, u = h = 0 for fp32 planar

exactly 0 where S_e == 0.  ``pack_images_c32`` has no arithmetic: the whole tensor is compared bit for bit.

ResidualBlock (``resblock_reference``): the kernel rounds the intermediate map to 16 bits BY DESIGN, so the reference's intermediate is the 16-bit
rounding of the fp64 act(conv1), zero outside the image.  An intermediate whose fp32 value lies on the other side of a rounding boundary moves the
outputs around it by an intermediate ulp times |w2|, which no bar of the output's own arithmetic covers.  Two bars, both asserted:
  hard   every element: the intermediate's bar (8 sqrt(288) 2^-24 S1 + u |mid| (+ h)) pushed through |w2|, plus the output's own bar;
  tight  the output's own bar, as if the intermediate were exact: at most ``TIGHT_CAP`` = 5e-4 of the elements may lie outside it.  The CPU fp32
         emulation (``emulate_resblock``) stays under a quarter of that for every case of the table (tests/test_enh_ref_cpu.py).

Weight gradient: ``conv_grad_ref.reference`` as it is (k = 3, stride 1, pad 1); for the sparse multi-trip case n_e is the number of NON-ZERO terms of
element e (the indicators (x != 0), (g != 0) pushed through the same map): a zero product adds exactly, so sqrt(n_e) 2^-24 S_e is still the bound of
the fp32 sum.  A prefilled slot (accumulate = 1) adds |previous| to S and one term to n, as ``conv_grad_ref.combine`` does.

Ratios measured on an MI355X (max over elements of |err| / unit bound, after taking off the storage term) are in profiles/enh_parity.json and, rounded,
in [brackets] behind the table rows below: the largest over the row's shapes, bf16 / f16.
"""
import functools
import math

import torch
import torch.nn.functional as F

import conv_grad_ref as G
from gdn_ref import FMT
from hesic_amd import synthetic

C_BAR = G.C_BAR
U24 = G.U24
ACT_NONE, ACT_RELU, ACT_LEAKY = G.ACT_NONE, G.ACT_RELU, G.ACT_LEAKY
TIGHT_CAP = 5e-4               # share of a ResidualBlock's outputs that may lie outside the tight bar
EMU_CAP = TIGHT_CAP / 4        # what the CPU fp32 emulation must stay under

# launch geometry, copied from the host code of enh.hip (a change there must be followed here: the multi-trip shapes are built around it)
TH, TW, FWD_BLOCKS = 16, 32, 512              # c32_conv3x3_kernel / c32_conv6_kernel: tile, persistent blocks
RB_TH, RB_TW, RB_BLOCKS = 14, 30, 256         # c32_resblock_r3_kernel
STRIP, WG_WAVES, WG_PARTS = 64, 1024, 256     # c32_wgrad_kernel: pixels per strip, waves (4 per block), block partials


def tiles(shape, th=TH, tw=TW):
    B, H, W = shape
    return B * (-(-H // th)) * (-(-W // tw))


def strips(shape):
    B, H, W = shape
    return B * H * (-(-W // STRIP))


def nparts(shape):
    return min(-(-strips(shape) // 4), WG_PARTS)


def r16(t, fmt):
    """``t`` rounded to the 16-bit format, in fp64."""
    return t.to(FMT[fmt]["dtype"]).double()


def q16(t, fmt):
    """``t`` rounded to the 16-bit format, in fp32."""
    return t.to(FMT[fmt]["dtype"]).float()


def act_fwd(pre, act):
    if act == ACT_RELU:
        return torch.relu(pre)
    if act == ACT_LEAKY:
        return torch.where(pre > 0, pre, pre * G.LEAKY32)
    return pre


def _R(ref, S, n, fmt, out16):
    f = FMT[fmt]
    return {"ref": {"y": ref}, "S": {"y": S}, "n": {"y": n}, "y16": out16, "dx16": True, "u16": f["u"], "h16": f["h"], "fmt": fmt}


def conv_reference(x, w, b, act, r1, r2, fmt, out16=True, n=288, padding=1):
    """act(conv3x3(x, w16) + b) + r1 + r2 with its sums of absolute terms; x (B, Cin, H, W) and r at 16-bit values, w, b fp32."""
    w16, x64 = r16(w, fmt), x.double()
    b64 = None if b is None else b.double()
    ref = act_fwd(F.conv2d(x64, w16, b64, padding=padding), act)
    S = F.conv2d(x64.abs(), w16.abs(), None if b is None else b64.abs(), padding=padding)
    for r in (r1, r2):
        if r is not None:
            ref, S = ref + r.double(), S + r.double().abs()
    return _R(ref, S, n, fmt, out16)


def pack_reference(xa, xb, fmt):
    """Channels 0..5 = the 16-bit rounding of cat(xa, xb), channels 6..31 zero (as the 16-bit dtype: compared with torch.equal)."""
    B, _, H, W = xa.shape
    out = torch.zeros(B, 32, H, W, dtype=FMT[fmt]["dtype"])
    out[:, :6] = torch.cat((xa, xb), 1).to(FMT[fmt]["dtype"])
    return out


def mid_bar(S1, mid, fmt):
    f = FMT[fmt]
    return C_BAR * math.sqrt(288) * U24 * S1 + f["u"] * mid.abs() + f["h"] * (S1 > 0)


def resblock_reference(x, w1, b1, w2, b2, act, r2, fmt, mid_override=None):
    """act(conv2(mid) + b2) + x + r2 with mid = the 16-bit rounding of act(conv1(x) + b1), zero outside the image.  Returns the forward R of the
    output (its ``bars`` are the TIGHT bars) plus ``push``: the intermediate's bar through |w2| (hard bar = tight + push).  ``mid_override``:
    an (H + 2, W + 2) intermediate including its ring (the mutation tests put conv1's extrapolation there)."""
    w1_16, w2_16, x64 = r16(w1, fmt), r16(w2, fmt), x.double()
    b1_64 = None if b1 is None else b1.double()
    S1 = F.conv2d(x64.abs(), w1_16.abs(), None if b1 is None else b1_64.abs(), padding=1)
    mid = r16(act_fwd(F.conv2d(x64, w1_16, b1_64, padding=1), act), fmt)
    if mid_override is None:
        R = conv_reference(mid, w2, b2, act, x, r2, fmt)
    else:                                 # the ring is part of the map: conv2 without padding
        R = conv_reference(mid_override, w2, b2, act, x, r2, fmt, padding=0)
    R["mid"], R["S1"] = mid, S1
    R["push"] = F.conv2d(mid_bar(S1, mid, fmt), w2_16.abs(), None, padding=1)
    return R


def resblock_check(R, got):
    """{"ok_hard", "ratio_hard" (max |err| / hard bar), "share_tight", "ratio" (unit ratio, as ``check``), "msg"}: every element against the hard
    bar, the share of elements outside the tight bar."""
    ref = R["ref"]["y"]
    got = got.detach().double().cpu().reshape(ref.shape)
    err = (got - ref).abs()
    tight = G.bars(R, "y")
    hard = tight + R["push"]
    bad = ~(err <= hard)
    out_t = ~(err <= tight)
    live = hard > 0
    ratio_hard = float((err[live] / hard[live]).max()) if bool(live.any()) else 0.0
    u = G.unit(R, "y")
    ul = u > 0
    ratio = float(((err - G.storage_term(R, "y")).clamp_min(0)[ul] / u[ul]).max()) if bool(ul.any()) else 0.0
    msg = ""
    if bool(bad.any()):
        idx = torch.nonzero(bad)
        worst = tuple(int(i) for i in idx[torch.argmax((err - hard)[bad])])
        msg = (f"y: {int(bad.sum())} of {bad.numel()} elements outside the hard bar; worst at {worst}: got {float(got[worst]):.9g} "
               f"ref {float(ref[worst]):.9g} bar {float(hard[worst]):.3g}; first index per dim {[int(i) for i in idx.min(0).values]} "
               f"last {[int(i) for i in idx.max(0).values]}")
    return {"ok_hard": not bool(bad.any()), "ratio_hard": ratio_hard, "share_tight": float(out_t.double().mean()), "ratio": ratio, "msg": msg,
            "bad_hard": bad, "bad_tight": out_t}


def conv_by_taps(x32, w16, b):
    """conv3x3 summed as c32_roll sums it: the fp32 accumulator starts from the bias (0 without one) and takes the nine taps in raster order, one
    v_mfma_f32_16x16x32 (K = 32 = all input channels of the tap) each.  The MFMA is modelled as the exact sum of its 32 exact products (fp64 holds
    them) added to the accumulator with ONE fp32 rounding: nine roundings per output, where a plain fp32 conv makes 288."""
    B, _, H, W = x32.shape
    xp = F.pad(x32.double(), (1, 1, 1, 1))
    w64 = w16.double()
    acc = torch.zeros(B, w16.shape[0], H, W) if b is None else b.float().view(1, -1, 1, 1).expand(B, -1, H, W).contiguous()
    for ky in range(3):
        for kx in range(3):
            acc = (acc.double() + torch.einsum("oc,bchw->bohw", w64[:, :, ky, kx], xp[:, :, ky:ky + H, kx:kx + W])).float()
    return acc


def emulate_resblock(x, w1, b1, w2, b2, act, r2, fmt, with_mid=False):
    """The kernel's arithmetic on the CPU: both convs summed tap by tap in fp32 (``conv_by_taps``), the intermediate rounded to 16 bits, the
    epilogue of c32_pack8 (act, then + (x + r2) in fp32), the output rounded to 16 bits.  ``with_mid``: (y, intermediate)."""
    x32 = x.float()
    mid = q16(act_fwd(conv_by_taps(x32, q16(w1, fmt), b1), act), fmt)
    y = act_fwd(conv_by_taps(mid, q16(w2, fmt), b2), act)
    y = q16(y + (x32 if r2 is None else x32 + r2.float()), fmt)
    return (y, mid) if with_mid else y


def nonzero_counts(x, g, wshape):
    """{"dw", "db"}: per element, the number of non-zero terms of its sum -- the indicators (x != 0), (g != 0) through the gradient's own map."""
    ix, ig = (x != 0).double(), (g != 0).double()
    return {"dw": torch.nn.grad.conv2d_weight(ix, wshape, ig, padding=1).round(), "db": ig.sum((0, 2, 3))}


def wgrad_reference(x, g, w, b, sparse_n=False, prev=None):
    """dw / db of conv3x3(x[:, :Cin], w) for the gradient g[:, :Cout] (``conv_grad_ref.reference``); ``sparse_n``: per-element counts of non-zero
    terms; ``prev`` = (dw0, db0): the slots' previous contents (accumulate = 1)."""
    cout, cin = w.shape[:2]
    xs, gs = x[:, :cin], g[:, :cout]
    R = G.reference(xs, w, b, gs, stride=1, pad=1)
    if sparse_n:
        R["n"] = dict(R["n"], **nonzero_counts(xs, gs, tuple(w.shape)))
    if prev is not None:
        for q, p in zip(("dw", "db"), prev):
            if p is None or R["ref"][q] is None:
                continue
            R["ref"][q] = R["ref"][q] + p.double()
            R["S"][q] = R["S"][q] + p.double().abs()
            R["n"] = dict(R["n"], **{q: R["n"][q] + 1})
    return R


# ------------------------------------------------------------------------------------------------------------------------------ operands
class Operands:
    """The operands of one (shape, format): x in [-2, 2] with exact zeros where |x| < 0.25 (``dense``: pushed out to +-0.25 instead), 16-bit
    residuals in [-1, 1], w uniform * sqrt(3 / fan_in) in fp32 (NOT pre-rounded: the kernels round it), biases up to +-0.2 in fp32, gy in [-1, 1] with
    exact zeros below 0.125 (``sparse_g``: non-zero at one pixel in 64 only), images and planar residuals fp32 at 16-bit values in [-1, 1]."""

    def __init__(self, shape, fmt, salt=0, dense=False, sparse_g=False):
        self.shape, self.fmt, self.salt, self.dense, self.sparse_g = tuple(shape), fmt, salt, dense, sparse_g

    def _u(self, name, shape, lo, hi):
        B, H, W = self.shape
        return synthetic._uniform(f"enh.{B}x{H}x{W}.{self.salt}.{name}", shape, lo, hi)

    def _map(self, name, c, lo=-1.0, hi=1.0):
        B, H, W = self.shape
        return q16(self._u(name, (B, c, H, W), lo, hi), self.fmt)

    @functools.cached_property
    def x(self):
        x = self._u("x", (self.shape[0], 32) + self.shape[1:], -2, 2)
        small = x.abs() < 0.25
        x = torch.where(small, torch.copysign(torch.full((), 0.25), x) if self.dense else torch.zeros(()), x)
        return q16(x, self.fmt)

    @functools.cached_property
    def gy(self):
        g = self._u("g", (self.shape[0], 32) + self.shape[1:], -1, 1)
        g = torch.where(g.abs() < 0.125, torch.zeros(()), g)
        if self.sparse_g:
            g = g * self.g_pixels
        return q16(g, self.fmt)

    @functools.cached_property
    def g_pixels(self):
        """(B, 1, H, W) bool: the pixels where the sparse gradient is non-zero (one in 64)."""
        B, H, W = self.shape
        return self._u("gmask", (B, 1, H, W), 0, 1) < 1.0 / 64

    r1 = functools.cached_property(lambda self: self._map("r1", 32))
    r2 = functools.cached_property(lambda self: self._map("r2", 32))
    img = functools.cached_property(lambda self: self._map("img", 4))          # planar residual: the first Cout planes
    xa = functools.cached_property(lambda self: self._map("xa", 3))
    xb = functools.cached_property(lambda self: self._map("xb", 3))

    def w(self, name, cout=32, cin=32):
        return synthetic._uniform(f"enh.w.{self.salt}.{name}", (cout, cin, 3, 3), -1, 1) * (3.0 / (cin * 9)) ** 0.5

    def b(self, name, cout=32):
        return synthetic._uniform(f"enh.b.{self.salt}.{name}", (cout,), -0.2, 0.2)


# ------------------------------------------------------------------------------------------------------------------------------ the case tables
SMALL = [(2, 5, 3), (1, 16, 32), (2, 17, 33), (2, 37, 45)]          # less than a tile; exactly one tile; four tiles, three ragged; 12 tiles
RB_SMALL = SMALL + [(1, 14, 30), (2, 15, 31), (2, 29, 61)]          # exactly one 14 x 30 tile; four tiles, three ragged; 18 tiles
MULTI_FWD = (130, 33, 65)          # 1170 tiles of 16 x 32 > 2 x 512: blocks 0 .. 145 make three trips; ragged right and bottom; 9 tiles per image
MULTI_RB = (57, 29, 61)            # 513 tiles of 14 x 30 > 2 x 256: block 0 makes three trips
MULTI_WG = (11, 65, 130)           # 2145 strips > 2 x 1024: waves 0 .. 96 take three; the last strip of a row holds 2 pixels
ZERO_TILE = (2, 37, 45)            # "zero_tile": x == 0 on tile (0, 0) of the last image and its halo, no bias: S_e == 0 on the whole tile
FORMATS = ("bf16", "f16")

# kind: the variant of hesic_conv3x3_c32_forward / _img6 / hesic_pack_images_c32.  [largest measured ratio over the row's shapes, bf16 / f16]
FWD_KINDS = {
    "plain":           dict(cout=32, bias=True, act=ACT_NONE, r1=False, r2=False),          # <0,0>; [y 0.001 / 0.008]
    "res1":            dict(cout=32, bias=True, act=ACT_LEAKY, r1=True, r2=False),          # <0,1>; [y 0.000 / 0.009]
    "res12":           dict(cout=32, bias=False, act=ACT_LEAKY, r1=True, r2=True),          # <0,2>; [y 0.000 / 0.004]
    "res2_only":       dict(cout=32, bias=True, act=ACT_RELU, r1=False, r2=True),           # the host's swap: <0,1> on res2; [y 0.001 / 0.004]
    "zero_tile":       dict(cout=32, bias=False, act=ACT_LEAKY, r1=False, r2=False),        # [y 0.000 / 0.006]
    "planar3":         dict(cout=3, bias=True, act=ACT_NONE, r1=True, r2=False),            # <1,0>, the residual requested with the halo; [y 0.038 / 0.044]
    "planar3_nores":   dict(cout=3, bias=True, act=ACT_LEAKY, r1=False, r2=False),          # <1,0>, res1 == NULL; [y 0.024 / 0.045]
    "planar1":         dict(cout=1, bias=True, act=ACT_NONE, r1=True, r2=False),            # [y 0.034 / 0.044]
    "planar2":         dict(cout=2, bias=False, act=ACT_RELU, r1=True, r2=False),           # [y 0.026 / 0.039]
    "planar4":         dict(cout=4, bias=True, act=ACT_NONE, r1=True, r2=False),            # <1,1>: in-loop residual loads; [y 0.038 / 0.047]
    "planar4_nores":   dict(cout=4, bias=True, act=ACT_NONE, r1=False, r2=False),           # [y 0.033 / 0.048]
    "img6":            dict(img6=True, bias=True, act=ACT_NONE),                            # [y 0.000 / 0.000]
    "img6_nobias_act": dict(img6=True, bias=False, act=ACT_LEAKY),                          # [y 0.000 / 0.000]
    "pack":            dict(pack=True),                                                     # bit-exact
}
MULTI_FWD_KINDS = ("res12", "planar3", "planar4", "img6")          # [res12 0.009 / 0.021, planar3 0.055 / 0.069, planar4 0.055 / 0.069, img6 0.024 / 0.030]
# ResidualBlock variants: (act, outer skip, biases).  Recorded: the largest |err| / hard bar (bar 1) and the largest tight-bar share (cap 5e-4) over
# the small shapes, then those of the multi-trip shape, bf16 / f16
RB_KINDS = {
    "leaky":       dict(act=ACT_LEAKY, r2=False, bias=True),          # <false, true>; [hard 0.47 / 0.37, share 8.8e-06 / 1.0e-04; multi-trip hard 0.51 / 0.39, share 2.8e-05 / 5.7e-05]
    "leaky_skip":  dict(act=ACT_LEAKY, r2=True, bias=True),           # <true, true>; [hard 0.44 / 0.39, share 2.7e-05 / 7.4e-05; multi-trip hard 0.52 / 0.43, share 2.1e-05 / 5.4e-05]
    "relu_skip":   dict(act=ACT_RELU, r2=True, bias=True),            # <true, false>; [hard 0.50 / 0.43, share 8.8e-06 / 1.5e-04; multi-trip hard 0.51 / 0.42, share 2.4e-05 / 5.2e-05]
    "none":        dict(act=ACT_NONE, r2=False, bias=False),          # <false, false>, b1 == b2 == NULL; [hard 0.31 / 0.28, share 2.4e-04 / 6.2e-05; multi-trip hard 0.33 / 0.29, share 3.9e-05 / 6.6e-05]
}
MULTI_RB_KINDS = ("leaky", "leaky_skip", "relu_skip", "none")
WG_WEIGHTS = ((32, 32), (32, 6), (3, 32))          # [small shapes, both formats: dw <= 0.246, db 0.000; multi-trip: dw 0.004, db 0.000]
# strip counts that give the finish kernel nparts = 1, 2, 3, 4, 5, 7 (its unroll-by-4 loop and tail) and the cap 256
FINISH_SHAPES = {1: (1, 3, 40), 2: (1, 5, 64), 3: (1, 9, 33), 4: (1, 13, 33), 5: (1, 17, 33), 7: (1, 13, 65), 256: (4, 128, 66)}          # [dw <= 0.078, db <= 0.012]


def fwd_cases():
    out = {}
    for fmt in FORMATS:
        for kind in FWD_KINDS:
            for shape in ([ZERO_TILE] if kind == "zero_tile" else SMALL):
                out["%s_%dx%dx%d_%s" % ((kind,) + shape + (fmt,))] = (kind, shape, fmt)
    return out


def rb_cases():
    return {"rb_%s_%dx%dx%d_%s" % ((kind,) + shape + (fmt,)): (kind, shape, fmt) for fmt in FORMATS for kind in RB_KINDS for shape in RB_SMALL}


FWD_CASES = fwd_cases()
RB_CASES = rb_cases()
MULTI_FWD_CASES = {"multi_%s_%s" % (kind, fmt): (kind, MULTI_FWD, fmt) for fmt in FORMATS for kind in MULTI_FWD_KINDS}
MULTI_RB_CASES = {"multi_rb_%s_%s" % (kind, fmt): (kind, MULTI_RB, fmt) for fmt in FORMATS for kind in MULTI_RB_KINDS}


def fwd_operands(kind, shape, fmt):
    """{"x" | "xa", "xb", "w", "b", "act", "r1", "r2", "cout"} of a forward case (CPU tensors: maps fp32 holding 16-bit values)."""
    k, o = FWD_KINDS[kind], Operands(shape, fmt)
    if k.get("pack"):
        return {"xa": o.xa, "xb": o.xb}
    if k.get("img6"):
        return {"xa": o.xa, "xb": o.xb, "w": o.w("w6", 32, 6), "b": o.b("b6") if k["bias"] else None, "act": k["act"]}
    x = o.x
    if kind == "zero_tile":
        x = x.clone()
        x[-1, :, :TH + 1, :TW + 1] = 0
    cout = k["cout"]
    r1 = None if not k["r1"] else (o.r1 if cout == 32 else o.img[:, :cout].contiguous())
    return {"x": x, "w": o.w("w", 32)[:cout].contiguous(), "b": o.b("b")[:cout].contiguous() if k["bias"] else None, "act": k["act"], "r1": r1,
            "r2": o.r2 if k["r2"] else None, "cout": cout}


def fwd_reference(kind, shape, fmt):
    k, a = FWD_KINDS[kind], fwd_operands(kind, shape, fmt)
    if k.get("pack"):
        return pack_reference(a["xa"], a["xb"], fmt)
    if k.get("img6"):
        return conv_reference(torch.cat((a["xa"], a["xb"]), 1), a["w"], a["b"], a["act"], None, None, fmt, n=54)
    return conv_reference(a["x"], a["w"], a["b"], a["act"], a["r1"], a["r2"], fmt, out16=a["cout"] == 32)


def rb_operands(kind, shape, fmt):
    k, o = RB_KINDS[kind], Operands(shape, fmt)
    return {"x": o.x, "w1": o.w("w1"), "b1": o.b("b1") if k["bias"] else None, "w2": o.w("w2"), "b2": o.b("b2") if k["bias"] else None,
            "act": k["act"], "r2": o.r2 if k["r2"] else None}


def rb_reference(kind, shape, fmt):
    a = rb_operands(kind, shape, fmt)
    return resblock_reference(a["x"], a["w1"], a["b1"], a["w2"], a["b2"], a["act"], a["r2"], fmt)


def wg_operands(shape, fmt, cout=32, cin=32, multi=False):
    """x, g (32-channel maps), w (Cout, Cin, 3, 3), b (Cout,): the multi-trip case has a dense x and a gradient that is non-zero at one pixel in 64."""
    o = Operands(shape, fmt, dense=multi, sparse_g=multi)
    return {"x": o.x, "g": o.gy, "w": r16(o.w("wg", 32)[:cout, :cin], fmt).float().contiguous(), "b": o.b("bg")[:cout].contiguous(), "pixels": o.g_pixels if multi else None}


@functools.lru_cache(maxsize=3)
def cached_wg_reference(shape, fmt, cout, cin, multi=False):
    """The weight-gradient reference of a case, computed once, shared, left unchanged."""
    a = wg_operands(shape, fmt, cout, cin, multi)
    return wgrad_reference(a["x"], a["g"], a["w"], a["b"], sparse_n=multi)


@functools.lru_cache(maxsize=2)
def cached_multi_reference(tag):
    """The reference of a multi-trip forward / ResidualBlock case: computed once, shared by the plain and the guarded run, left unchanged.  Two
    entries are enough (and sixteen would hold 3 GB): the tests' ``guard`` parameter varies fastest, so a tag's two runs are adjacent."""
    if tag in MULTI_FWD_CASES:
        return fwd_reference(*MULTI_FWD_CASES[tag])
    return rb_reference(*MULTI_RB_CASES[tag])


def clear_cache():
    cached_wg_reference.cache_clear()
    cached_multi_reference.cache_clear()


def previous_slots(shape, cout=32, cin=32, salt=0):
    """Non-zero previous contents of a (dw, db) gradient slot pair for accumulate = 1: what an earlier backward pass of the same layer left there,
    i.e. of a gradient's own magnitude -- a sum of B H W terms of random sign, sqrt(B H W) times a term."""
    scale = math.sqrt(shape[0] * shape[1] * shape[2])
    return (synthetic._uniform(f"enh.prev.dw.{salt}", (cout, cin, 3, 3), -1, 1) * scale, synthetic._uniform(f"enh.prev.db.{salt}", (cout,), -1, 1) * scale)


def strip_of(shape, s):
    """(image, row, first column, live pixels, wave, trip) of strip ``s`` of c32_wgrad_kernel's walk."""
    B, H, W = shape
    sx_n = -(-W // STRIP)
    q, sx = divmod(s, sx_n)
    b, y = divmod(q, H)
    nw = min(-(-strips(shape) // 4), WG_PARTS) * 4
    return b, y, sx * STRIP, min(STRIP, W - sx * STRIP), s % nw, s // nw

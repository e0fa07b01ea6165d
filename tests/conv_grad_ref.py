"""fp64 reference with a per-element error model for the conv / deconv gradients of the 16-bit path (a plain module, not a conftest).

For one conv case ``reference()`` returns, all in fp64 on the CPU:

  ref   y, dx, dw, db by torch autograd.  The operands are exactly what the kernels receive (x, w and gy hold bf16-representable
        values, the bias is fp32), so no rounding hides in the comparison.
  S     the same four quantities with every operand replaced by its absolute value: S_e = sum_i |t_i| over the terms of element e.
  n     the nominal term count: dw B*QH*QW, db B*Ho*Wo, y Cin*KH*KW, dx Cout*KH*KW.

and ``bars()`` turns them into  bar_e = c * sqrt(n) * 2^-24 * S_e  (+ 2^-8 * |ref_e| where the output is stored in bf16).  The unit bound
sqrt(n) * 2^-24 * S_e is the statistical bound of an fp32 sum of n exact products in any order; c = 8 (``C_BAR``) leaves room for MFMA block
accumulation, split-K partials and float atomics.  torch's own fp32 evaluation of the same gradients stays below 1.0 of the unit bound
(tests/test_conv_grad_ref_cpu.py asserts it for every case).  Where S_e == 0 (dead taps of a mask, taps that never meet a 1x1 / 2x2 map, x == 0
under in_abs) the bar is 0: the kernel's value must be exactly 0.  No element is left out of a comparison.

Roundings the kernels make BY DESIGN and that are therefore part of the reference's operands:
  * an activation's backward (``hesic_act_backward``) stores gy * act'(y) in y's storage type: g = bf16(gy) for y > 0, bf16(0.01f * gy)
    (LEAKY, product in fp32) or 0 (RELU) otherwise.  act'(y) is taken from the y the backward pass saved (``y_saved``) when the caller has
    it -- the sign of an output within its own bar of 0 is not the gradient's business.
"""
import functools
import math

import torch
import torch.nn.functional as F

from hesic_amd import synthetic

C_BAR = 8.0
U24 = 2.0 ** -24
U8 = 2.0 ** -8
ACT_NONE, ACT_RELU, ACT_LEAKY = 0, 1, 2
LEAKY32 = float(torch.tensor(0.01, dtype=torch.float32))          # the kernels' 0.01f


def bf(t):
    return t.to(torch.bfloat16).to(t.dtype)


def out_hw(H, W, k, stride, pad, transposed, out_pad=None):
    if transposed:
        op = stride - 1 if out_pad is None else out_pad
        f = lambda n: (n - 1) * stride - 2 * pad + k + op
    else:
        f = lambda n: (n + 2 * pad - k) // stride + 1
    return f(H), f(W)


def _conv(x, w, b, stride, pad, transposed, out_pad):
    if transposed:
        return F.conv_transpose2d(x, w, b, stride=stride, padding=pad, output_padding=out_pad)
    return F.conv2d(x, w, b, stride=stride, padding=pad)


def act_grad(gy, y, act, g16):
    """gy * act'(y) as ``_ConvFn.backward`` stores it (fp64 tensor holding the stored values)."""
    if act == ACT_NONE:
        return gy.double()
    pos = y > 0
    if act == ACT_RELU:
        return torch.where(pos, gy.double(), torch.zeros((), dtype=torch.float64))
    neg = gy.float() * torch.tensor(0.01, dtype=torch.float32)            # one fp32 product, as in the kernel
    if g16:
        neg = bf(neg)
    return torch.where(pos, gy.double(), neg.double())


def reference(x, w, b, gy, *, stride, pad, transposed=False, out_pad=None, mask=None, in_abs=False, act=ACT_NONE, y_saved=None,
              y16=True, dx16=True):
    """x (B, Cin, H, W), w in PyTorch layout, b (Cout,) or None, gy shaped like y.  Returns {"ref", "S", "n", "y16", "dx16"}."""
    k = w.shape[-1]
    if transposed and out_pad is None:
        out_pad = stride - 1
    x64, w64, gy64 = x.double(), w.double(), gy.double()
    b64 = None if b is None else b.double()
    m64 = None if mask is None else mask.double()
    Cin, Cout = (w.shape[0], w.shape[1]) if transposed else (w.shape[1], w.shape[0])
    B, _, H, W = x.shape

    def run(xv, wv, bv, g_of_y):
        xl, wl = xv.clone().requires_grad_(), wv.clone().requires_grad_()
        bl = None if bv is None else bv.clone().requires_grad_()
        xe = xl.abs() if in_abs else xl
        we = wl if m64 is None else wl * m64
        pre = _conv(xe, we, bl, stride, pad, transposed, out_pad)
        g = g_of_y(pre.detach())
        grads = torch.autograd.grad(pre, [xl, wl] + ([bl] if bl is not None else []), g)
        return pre.detach(), grads[0], grads[1], (grads[2] if bl is not None else None)

    def act_fwd(pre):
        if act == ACT_RELU:
            return torch.relu(pre)
        if act == ACT_LEAKY:
            return torch.where(pre > 0, pre, pre * LEAKY32)
        return pre

    keep = {}

    def g_ref(pre):
        y = act_fwd(pre)
        ys = y if y_saved is None else y_saved.double()
        keep["g"] = act_grad(gy, ys, act, y16)
        return keep["g"]

    pre, dx, dw, db = run(x64, w64, b64, g_ref)
    ref = {"y": act_fwd(pre), "dx": dx, "dw": dw, "db": db}
    g_abs = keep["g"].abs()
    # the sums of absolute terms: |x|, |w|, |b|, |g| through the same (linear) maps; under in_abs the data gradient keeps sign(x)'s zeros
    Sy, Sdx, Sdw, Sdb = run(x64.abs(), w64.abs(), None if b64 is None else b64.abs(), lambda pre_: g_abs)
    if in_abs:
        Sdx = Sdx.abs()
    # (|act(pre)| <= |pre|: the linear part's sum of absolute terms bounds the activated output too)
    S ={"y": Sy, "dx": Sdx, "dw": Sdw, "db": Sdb}
    QH, QW = (H, W) if transposed else tuple(pre.shape[-2:])
    n = {"dw": B * QH * QW, "db": B * pre.shape[-2] * pre.shape[-1], "y": Cin * k * k, "dx": Cout * k * k}
    return {"ref": ref, "S": S, "n": n, "y16": y16, "dx16": dx16, "g": keep["g"]}


def combine(a, b_):
    """The reference of two gradients added into one buffer (one weight used twice): sums, sums of absolute terms and term counts add."""
    out = {"ref": {}, "S": {}, "n": {}, "y16": a["y16"], "dx16": a["dx16"]}
    for q in ("dw", "db"):
        out["ref"][q] = a["ref"][q] + b_["ref"][q]
        out["S"][q] = a["S"][q] + b_["S"][q]
        out["n"][q] = a["n"][q] + b_["n"][q]
    return out


def unit(R, q):
    """sqrt(n) * 2^-24 * S_e: the unit bound of output ``q`` (n: one count per output, or a tensor of per-element counts)."""
    n = R["n"][q]
    return (n.double().sqrt() if torch.is_tensor(n) else math.sqrt(n)) * U24 * R["S"][q]


def storage_term(R, q):
    """What storing output ``q`` in 16 bits may add to its error: u |ref_e| (+ h for a format with subnormals) where S_e > 0, else 0.  bf16
    (u = 2^-8, h = 0) unless the reference names another format (``u16``, ``h16``: tests/enh_ref.py)."""
    ref = R["ref"][q]
    if not ((q == "y" and R["y16"]) or (q == "dx" and R["dx16"])):
        return torch.zeros_like(ref)
    h = R.get("h16", 0.0)
    return R.get("u16", U8) * ref.abs() + (h * (R["S"][q] > 0) if h else 0.0)


def bars(R, q, c=C_BAR):
    return c * unit(R, q) + storage_term(R, q)


def check(R, q, got, c=C_BAR):
    """(ok, ratio, message): every element of ``got`` within bar_e of the reference; ratio = max_e |err_e| / (sqrt(n) 2^-24 S_e) over the
    elements with S_e > 0 (for a bf16-stored output the 2^-8 |ref_e| storage term is taken off the error first)."""
    ref = R["ref"][q]
    got = got.detach().double().cpu().reshape(ref.shape)
    err = (got - ref).abs()
    bar = bars(R, q, c)
    u = unit(R, q)
    live = u > 0
    store = storage_term(R, q)
    ratio = float(((err - store).clamp_min(0)[live] / u[live]).max()) if bool(live.any()) else 0.0
    bad = ~(err <= bar)                              # NaN counts as a miss
    msg = ""
    if bool(bad.any()):
        idx = torch.nonzero(bad)
        worst = idx[torch.argmax((err - bar)[bad])]
        msg = (f"{q}: {int(bad.sum())} of {bad.numel()} elements outside their bar; worst at {tuple(int(i) for i in worst)}: "
               f"got {float(got[tuple(worst)]):.9g} ref {float(ref[tuple(worst)]):.9g} bar {float(bar[tuple(worst)]):.3g}; "
               f"first index per dim {[int(i) for i in idx.min(0).values]} last {[int(i) for i in idx.max(0).values]}; "
               f"dead elements hit {int((bad & ~live).sum())}")
    return not bool(bad.any()), ratio, msg


# ------------------------------------------------------------------------------------------------------------------------ the case table
# tag: (Cin, Cout, k, stride, pad, transposed, (B, H, W), options).  Ratios measured on an MI355X (max over elements of |err| / unit bound;
# y / dx after taking off the bf16 storage term) are recorded in profiles/conv_grad_parity.json and, rounded, in [brackets] behind each case:
# 0.000 means the fp32 sums came out exact.  The bar is 8; no case needed a kernel change.
WIDE = {
    "c5s2_128":        (128, 128, 5, 2, 2, 0, (2, 32, 32), {}),                    # Q = 512: two K slices of 256; [y 0.000 dx 0.001 dw 0.020 db 0.000]
    "c5s2_64_72":      (64, 72, 5, 2, 2, 0, (1, 10, 6), {}),                       # ragged ci / co tiles, Q = 15; strided data gradient; [y 0.000 dx 0.000 dw 0.000 db 0.000]
    "c5s1_320_128":    (320, 128, 5, 1, 2, 0, (1, 12, 12), {}),   # [y 0.000 dx 0.000 dw 0.053 db 0.000]
    "c5s1_128_960":    (128, 960, 5, 1, 2, 0, (1, 8, 8), {}),   # [y 0.000 dx 0.000 dw 0.000 db 0.000]
    "c3s1_288_384":    (288, 384, 3, 1, 1, 0, (1, 8, 8), {}),   # [y 0.000 dx 0.000 dw 0.000 db 0.000]
    "c1_768_640":      (768, 640, 1, 1, 0, 0, (2, 4, 4), {}),   # [y 0.000 dx 0.000 dw 0.000 db 0.000]
    "c5s2_tiny":       (128, 128, 5, 2, 2, 0, (2, 2, 2), {}),                      # one K slice; most taps never meet the map; [y 0.000 dx 0.000 dw 0.000 db 0.000]
    "d5s2_128":        (128, 128, 5, 2, 2, 1, (2, 16, 16), {}),   # [y 0.002 dx 0.000 dw 0.019 db 0.000]
    "d5s2_192_128":    (192, 128, 5, 2, 2, 1, (1, 4, 4), {}),   # [y 0.000 dx 0.000 dw 0.000 db 0.000]
    "d5s2_1x1":        (128, 128, 5, 2, 2, 1, (2, 1, 1), {}),   # [y 0.000 dx 0.000 dw 0.000 db 0.000]
    "d5s1_bias_tap":   (128, 128, 5, 1, 2, 1, (1, 7, 9), {}),                      # stride 1 transposed: a single bias tap; [y 0.000 dx 0.001 dw 0.000 db 0.000]
    "d5s2_128_288":    (128, 288, 5, 2, 2, 1, (1, 8, 4), {}),   # [y 0.000 dx 0.000 dw 0.000 db 0.000]
    "c5s2_ragged_k":   (128, 128, 5, 2, 2, 0, (1, 46, 50), {}),                    # Q = 575: slices of 320 + 255 pixels; [y 0.001 dx 0.001 dw 0.016 db 0.000]
    "c5s2_128_nobias": (128, 128, 5, 2, 2, 0, (2, 32, 32), {"bias": False}),   # [y 0.000 dx 0.001 dw 0.018]
    "mask_A_taps":     (192, 384, 5, 1, 2, 0, (1, 8, 8), {"mask": "A", "tap_mask": (1 << 12) - 1}),   # [y 0.000 dx 0.000 dw 0.000 db 0.000]
    "mask_B_taps":     (192, 384, 5, 1, 2, 0, (1, 8, 8), {"mask": "B", "tap_mask": (1 << 13) - 1}),   # [y 0.000 dx 0.000 dw 0.000 db 0.000]
    "mask_A_plain":    (192, 384, 5, 1, 2, 0, (1, 8, 8), {"mask": "A"}),           # no tap_mask: all taps computed, dw * mask; [y 0.001 dx 0.000 dw 0.000 db 0.000]
    "abs_relu":        (192, 128, 5, 1, 2, 0, (2, 8, 8), {"in_abs": True, "act": ACT_RELU}),   # [y 0.000 dx 0.000 dw 0.000 db 0.000]
    "leaky_c3":        (128, 128, 3, 1, 1, 0, (1, 8, 8), {"act": ACT_LEAKY}),   # [y 0.000 dx 0.000 dw 0.259 db 0.000]
}
# image side: images are fp32 tensors holding bf16-representable values, so the MFMA routes (bf16 operands) and the fp32 routes see one operand
IMAGE = {
    "conv1_fused":     (3, 128, 5, 2, 2, 0, (2, 64, 128), {}),                     # QW = 64; [y 0.000 dx 0.007 dw 0.003 db 0.000]
    "conv1_im2col":    (3, 128, 5, 2, 2, 0, (2, 50, 70), {}),   # [y 0.008 dx 0.007 dw 0.004 db 0.000]
    "conv1_odd":       (3, 128, 5, 2, 2, 0, (1, 51, 71), {}),                      # generic atomics (dw varies run to run), generic data gradient; [y 0.019 dx 0.019 dw 0.033 db 0.000]
    "conv1_2x2":       (3, 128, 5, 2, 2, 0, (1, 2, 2), {}),   # [y 0.000 dx 0.003 dw 0.000 db 0.000]
    "conv1_nhwc":      (3, 128, 5, 2, 2, 0, (2, 50, 70), {"x_nhwc": True}),   # [y 0.000 dx 0.006 dw 0.005 db 0.000]
    "deconv4_fused":   (128, 3, 5, 2, 2, 1, (2, 32, 64), {}),   # [y 0.007 dx 0.000 dw 0.003 db 0.000]
    "deconv4_im2col":  (128, 3, 5, 2, 2, 1, (2, 23, 37), {}),   # [y 0.008 dx 0.000 dw 0.006 db 0.000]
    "deconv4_1x1":     (128, 3, 5, 2, 2, 1, (1, 1, 1), {}),   # [y 0.003 dx 0.000 dw 0.000 db 0.000]
    "pre_5x3":         (6, 3, 5, 1, 2, 0, (1, 5, 3), {}),   # [y 0.045 dx 0.065 dw 0.000 db 0.000]
    "pre_16x64":       (6, 3, 5, 1, 2, 0, (1, 16, 64), {}),   # [y 0.056 dx 0.085 dw 0.005 db 0.000]
    "pre_17x130":      (6, 3, 5, 1, 2, 0, (1, 17, 130), {}),                       # Wo >= 64 and Wo >= 128 forward / data-gradient kernels; [y 0.071 dx 0.136 dw 0.003 db 0.000]
    "after_5x3":       (6, 3, 5, 1, 2, 1, (1, 5, 3), {}),   # [y 0.026 dx 0.039 dw 0.000 db 0.000]
    "after_16x64":     (6, 3, 5, 1, 2, 1, (1, 16, 64), {}),   # [y 0.057 dx 0.144 dw 0.002 db 0.000]
    "after_17x130":    (6, 3, 5, 1, 2, 1, (1, 17, 130), {}),   # [y 0.078 dx 0.084 dw 0.002 db 0.000]
}
# direct C-ABI calls (weight / bias gradient only)
DIRECT = {
    "d4s2_colsum":     (128, 128, 4, 2, 0, 1, (2, 6, 5), {"out_pad": 0}),          # k = 4, pad 0: the bias-in-GEMM tap set does not exist; [dw 0.000 db 0.000]
    "conv1_nw_kernel": (3, 128, 5, 2, 2, 0, (2, 18, 34), {}),                      # hesic_sconv2d_wgrad without a workspace; [dw 0.017 db 0.000]
}
CASES = {**WIDE, **IMAGE, **DIRECT}
# hesic_conv2d_wgrad (the packed-layout entry; weight / bias gradient only), in bf16 and in fp32.  Kept out of CASES: the CPU mutation tests
# size their one-dropped-product argument for Q <= 4096 (see operands()).
PACKED = {
    "packed_c5s2":     (128, 128, 5, 2, 2, 0, (1, 16, 16), {}),                    # Q = 64: one K slice, the plain reduce; [dw 0.000 db 0.000]
    "packed_c1_wide":  (128, 128, 1, 1, 0, 0, (1, 96, 96), {}),                    # Q = 9216, one tap: >= 32 K slices, the slice-parallel reduce; [dw 0.003 db 0.000]
    "packed_mask12":   (128, 128, 5, 1, 2, 0, (1, 8, 8), {"mask": "A", "tap_mask": (1 << 12) - 1}),      # 13 dead taps must come back 0; [dw 0.000 db 0.000]
}


def case(tag):
    return CASES[tag] if tag in CASES else PACKED[tag]


def make_mask(kind, wshape):
    """MaskedConv2d's mask (compressai/layers/layers.py): rows below the centre and, in the centre row, the centre (A) / what follows it."""
    m = torch.ones(wshape)
    h, w = wshape[-2:]
    m[:, :, h // 2, w // 2 + (kind == "B"):] = 0
    m[:, :, h // 2 + 1:] = 0
    return m


def storage(tag):
    """(y16, dx16): which of the two map outputs the 16-bit path stores in bf16."""
    Cin, Cout = case(tag)[0], case(tag)[1]
    return (Cout > 8), (Cin > 8)


@functools.lru_cache(maxsize=None)
def operands(tag, salt=0):
    """x, w, b, gy (+ mask) of a case: fp32 tensors holding bf16-representable values (the bias: plain fp32).  x has both signs (images in
    [0, 1] would hide sign errors) and exact zeros where |x| < 0.25 (one in eight).  The threshold is also what lets ONE dropped product show
    at the largest pixel count of the table (Q = 4096, conv1_fused): the bar is 8 * sqrt(Q) * 2^-24 * Q * mean|x gy| = mean|x gy| / 8 there,
    and with |x| in [0.25, 2], |gy| in [0, 1] uniform, P(|x gy| < mean / 8) = 0.0615 * ln(8) / 1.75 = 7 %; with |x| down to 0 it is 14 %."""
    Cin, Cout, k, s, p, tr, (B, H, W), opt = case(tag)
    name = f"cgp.{tag}.{salt}."
    wshape = (Cin, Cout, k, k) if tr else (Cout, Cin, k, k)
    fan = Cin * k * k / (s * s if tr else 1)
    x = synthetic._uniform(name + "x", (B, Cin, H, W), -2, 2)
    x = bf(torch.where(x.abs() < 0.25, torch.zeros(()), x))
    w = bf(synthetic._uniform(name + "w", wshape, -1, 1) * (3.0 / fan) ** 0.5)
    b = synthetic._uniform(name + "b", (Cout,), -0.1, 0.1) if opt.get("bias", True) else None
    Ho, Wo = out_hw(H, W, k, s, p, tr, opt.get("out_pad"))
    gy = synthetic._uniform(name + "g", (B, Cout, Ho, Wo), -1, 1)
    gy = bf(torch.where(gy.abs() < 0.125, torch.zeros(()), gy))          # likewise: no term far below the mean, exact zeros instead
    mask = make_mask(opt["mask"], wshape) if "mask" in opt else None
    return {"x": x, "w": w, "b": b, "gy": gy, "mask": mask}


def reference_of(tag, salt=0, y_saved=None):
    Cin, Cout, k, s, p, tr, _, opt = case(tag)
    o = operands(tag, salt)
    y16, dx16 = storage(tag)
    return reference(o["x"], o["w"], o["b"], o["gy"], stride=s, pad=p, transposed=bool(tr), out_pad=opt.get("out_pad"), mask=o["mask"],
                     in_abs=opt.get("in_abs", False), act=opt.get("act", ACT_NONE), y_saved=y_saved, y16=y16, dx16=dx16)


@functools.lru_cache(maxsize=None)
def cached_reference(tag, salt=0):
    """The reference of a case without an activation (its backward does not depend on a saved y): computed once, shared, left unchanged."""
    return reference_of(tag, salt)

"""The fp64 reference and error model of tests/enh_ref.py, checked on the CPU for the cases of tests/test_gpu_enh_parity.py:

  (a) the reference agrees with fp64 autograd of the oracle composition (one conv with residuals, leaky(conv2(leaky(conv1 x))) + x + r2, the
      weight gradient re-assembled pixel by pixel);
  (b) torch's own fp32 evaluation stays within the UNIT bound sqrt(n) 2^-24 S_e (ratio <= 1) for every case, so the bar c = 8 is more than eight
      times the error of an honest fp32 evaluation (the sparse multi-trip weight gradient with its non-zero term counts: 0.008);
  (c) the fp32 emulation of the ResidualBlock (the kernel's summation order, 16-bit intermediate and output) passes the hard bar everywhere and leaves at most
      ``EMU_CAP`` = 1.25e-4 of the elements outside the tight bar (a quarter of the device's cap 5e-4);
  (d) each failure class of the persistent kernels leaves its bar.  A mutation is applied to the reference output at a position (a tile, a tile
      edge, a strip, a block partial, ...) and the same ``check`` runs: it must fail at EVERY sampled position (at least 32 per class where the
      class has that many).  "mutation <class> <format>: detected a of a" is printed per class.

The emulation of (c) sums as the kernel does (``enh_ref.conv_by_taps``: the accumulator starts from the bias and takes nine taps, each the exact
32-channel dot product of one MFMA, with one fp32 rounding per tap).  Figures, share outside the tight bar / share of flipped intermediates / worst
element against the hard bar: bfloat16 <= 1.22e-4 ((2, 37, 45) ``none``: 13 of 106,560 elements) / <= 1.0e-4 / 0.52; float16 <= 1.15e-4
((2, 29, 61) ``none``) / 0.7 - 5e-4 (1e-3 of the 960 elements of (2, 5, 3)) / 0.43; multi-trip (57, 29, 61) 1.9 - 2.2e-5 (bf16), 2.6 - 3.3e-5 (f16);
0 elements outside in 47 of the 64 cases, (1, 14, 30) and (2, 15, 31) among them.  torch's own fp32 conv in its place (288 roundings per sum, in
an order the library chooses) flips four to five times as many float16 intermediates and left up to 9.7e-4 of (1, 14, 30) outside: that is the
arithmetic of no kernel here and is not what (c) asserts.
"""
import pytest
import torch
import torch.nn.functional as F

import conv_grad_ref as G
import enh_ref as E

MUT_FWD = (5, 33, 65)            # 45 tiles of 16 x 32, nine per image: every class has 32 positions; ragged right (1 column) and bottom (1 row)
MUT_RB = (8, 29, 61)           # 18 tiles of 14 x 30 per image; 8 images x 4 sides = 32 positions of the ring mutation
NPOS = 32


def _pick(items, n=NPOS):
    """``n`` of ``items``, evenly spread (all of them if there are fewer)."""
    items = list(items)
    if len(items) <= n:
        return items
    return [items[(i * len(items)) // n] for i in range(n)]


# ---------------------------------------------------------------------------------------------------------------- (a) reference against autograd
@pytest.mark.parametrize("fmt", E.FORMATS)
def test_reference_agrees_with_fp64_autograd_of_the_oracle_composition(fmt):
    o = E.Operands((2, 17, 33), fmt)
    w1, w2, b1, b2 = o.w("w1"), o.w("w2"), o.b("b1"), o.b("b2")
    lk = lambda t: F.leaky_relu(t, G.LEAKY32)
    x64 = o.x.double().requires_grad_()
    w16 = E.r16(w1, fmt).requires_grad_()
    b64 = b1.double().requires_grad_()
    y = lk(F.conv2d(x64, w16, b64, padding=1)) + o.r1.double() + o.r2.double()
    R = E.conv_reference(o.x, w1, b1, E.ACT_LEAKY, o.r1, o.r2, fmt)
    assert float((R["ref"]["y"] - y.detach()).abs().max()) < 1e-12
    # S is the same map on absolute values: the gradient of sum(y) w.r.t. a unit scaling of every |term| -- here simply recomputed by hand
    S = F.conv2d(o.x.double().abs(), w16.detach().abs(), b1.double().abs(), padding=1) + o.r1.double().abs() + o.r2.double().abs()
    assert torch.equal(R["S"]["y"], S) and bool((S >= R["ref"]["y"].abs() - 1e-12).all())
    # the weight gradient of that conv by autograd against conv_grad_ref.reference on the same g (ACT_NONE: no stored act' rounding)
    g = o.gy.double()
    dx, dw, db = torch.autograd.grad(F.conv2d(x64, w16, b64, padding=1), [x64, w16, b64], g)
    Rw = E.wgrad_reference(o.x, o.gy, w16.detach().float(), b1)
    assert float((Rw["ref"]["dw"] - dw).abs().max()) < 1e-9 and float((Rw["ref"]["db"] - db).abs().max()) < 1e-9
    assert float((Rw["ref"]["dx"] - dx).abs().max()) < 1e-9
    # the ResidualBlock without the by-design rounding ("f32": the intermediate keeps 24 bits) against the plain composition
    Rb = E.resblock_reference(o.x, w1, b1, w2, b2, E.ACT_LEAKY, o.r2, "f32")
    comp = lk(F.conv2d(lk(F.conv2d(o.x.double(), w1.double(), b1.double(), padding=1)), w2.double(), b2.double(), padding=1)) + o.x.double() + o.r2.double()
    assert float((Rb["ref"]["y"] - comp).abs().max()) < 1e-6
    # and with it: the intermediate is zero outside the image (conv2 pads the intermediate, not conv1's extrapolation)
    ext = E.r16(lk(F.conv2d(o.x.double(), E.r16(w1, fmt), b1.double(), padding=2)), fmt)
    assert torch.equal(ext[:, :, 1:-1, 1:-1], E.resblock_reference(o.x, w1, b1, w2, b2, E.ACT_LEAKY, o.r2, fmt)["mid"])
    assert float(ext[:, :, 0].abs().max()) > 0


def test_leaky_training_form_agrees_with_autograd_up_to_the_stored_gradient():
    """conv_grad_ref.reference with act = LEAKY stores act'(y) gy in bf16 by design: dw differs from plain autograd by at most 2^-8 of the
    negative side's terms (0.01 |gy| |x|), summed."""
    o = E.Operands((2, 17, 33), "bf16")
    w, b = E.r16(o.w("w"), "bf16").float(), o.b("b")
    R = G.reference(o.x, w, b, o.gy, stride=1, pad=1, act=G.ACT_LEAKY)
    x64, w64, b64 = o.x.double().requires_grad_(), w.double().requires_grad_(), b.double().requires_grad_()
    y = F.leaky_relu(F.conv2d(x64, w64, b64, padding=1), G.LEAKY32)
    dx, dw, db = torch.autograd.grad(y, [x64, w64, b64], o.gy.double())
    assert float((R["ref"]["y"] - y.detach()).abs().max()) < 1e-12
    for q, t in (("dx", dx), ("dw", dw), ("db", db)):
        assert bool(((R["ref"][q] - t).abs() <= 2.0 ** -8 * R["S"][q] + 1e-12).all()), q


# ---------------------------------------------------------------------------------------------------------------- (b) fp32 under the unit bound
def _fp32_forward(kind, shape, fmt):
    k, a = E.FWD_KINDS[kind], E.fwd_operands(kind, shape, fmt)
    if k.get("img6"):
        x = torch.cat((a["xa"], a["xb"]), 1)
        return E.act_fwd(F.conv2d(x, E.q16(a["w"], fmt), a["b"], padding=1), a["act"])
    y = E.act_fwd(F.conv2d(a["x"], E.q16(a["w"], fmt), a["b"], padding=1), a["act"])
    for r in (a["r1"], a["r2"]):
        if r is not None:
            y = y + r
    return y


FWD_ARITH = {t: c for t, c in E.FWD_CASES.items() if c[0] != "pack"}


@pytest.mark.parametrize("tag", list(FWD_ARITH) + list(E.MULTI_FWD_CASES))
def test_fp32_forward_is_within_the_unit_bound(tag):
    kind, shape, fmt = (FWD_ARITH.get(tag) or E.MULTI_FWD_CASES[tag])
    R = dict(E.fwd_reference(kind, shape, fmt), y16=False)
    ok, ratio, msg = G.check(R, "y", _fp32_forward(kind, shape, fmt), c=1.0)
    print(f"enh_ref_cpu {tag} y fp32 ratio {ratio:.3f}")
    assert ok and ratio <= 1.0, msg
    if kind == "zero_tile":
        dead = R["S"]["y"] == 0
        assert int(dead[-1, :, :E.TH, :E.TW].sum()) == 32 * E.TH * E.TW and bool((R["ref"]["y"][dead] == 0).all())
        ok, _, msg = G.check(E.fwd_reference(kind, shape, fmt), "y", R["ref"]["y"] + dead * 1e-30)
        assert not ok and "dead elements hit" in msg


def test_pack_reference_is_the_16_bit_rounding_of_the_images():
    for fmt in E.FORMATS:
        a = E.fwd_operands("pack", (2, 5, 3), fmt)
        ref = E.fwd_reference("pack", (2, 5, 3), fmt)
        assert torch.equal(ref[:, :6].float(), torch.cat((a["xa"], a["xb"]), 1)) and float(ref[:, 6:].float().abs().max()) == 0
        assert bool((ref[:, :6].float() < 0).any()) and bool((ref[:, :6].float() > 0).any())


ALL_RB = {**E.RB_CASES, **E.MULTI_RB_CASES}


@pytest.mark.parametrize("tag", list(ALL_RB))
def test_resblock_fp32_second_conv_is_within_the_unit_bound(tag):
    """With the reference's own intermediate the output is one conv: fp32 under the unit bound."""
    kind, shape, fmt = ALL_RB[tag]
    a, R = E.rb_operands(kind, shape, fmt), E.rb_reference(kind, shape, fmt)
    y = E.act_fwd(F.conv2d(R["mid"].float(), E.q16(a["w2"], fmt), a["b2"], padding=1), a["act"]) + a["x"]
    if a["r2"] is not None:
        y = y + a["r2"]
    ok, ratio, msg = G.check(dict(R, y16=False), "y", y, c=1.0)
    print(f"enh_ref_cpu {tag} y fp32 ratio {ratio:.3f}")
    assert ok and ratio <= 1.0, msg


def _fp32_wgrad(a, cout, cin):
    x, g = a["x"][:, :cin].contiguous(), a["g"][:, :cout].contiguous()
    return torch.nn.grad.conv2d_weight(x, (cout, cin, 3, 3), g, padding=1), g.sum((0, 2, 3))


WG_CPU = [(s, "bf16", co, ci, False) for s in E.SMALL + list(E.FINISH_SHAPES.values()) for co, ci in ((32, 32),)] + \
         [((2, 17, 33), "f16", 32, 32, False)] + [(E.MULTI_WG, "bf16", co, ci, True) for co, ci in E.WG_WEIGHTS]


@pytest.mark.parametrize("shape,fmt,cout,cin,multi", WG_CPU, ids=["%dx%dx%d_%s_%dx%d" % (s + (f, co, ci)) for s, f, co, ci, _ in WG_CPU])
def test_fp32_weight_gradient_is_within_the_unit_bound(shape, fmt, cout, cin, multi):
    a = E.wg_operands(shape, fmt, cout, cin, multi)
    R = E.cached_wg_reference(shape, fmt, cout, cin, multi)
    dw, db = _fp32_wgrad(a, cout, cin)
    for q, t in (("dw", dw), ("db", db)):
        ok, ratio, msg = G.check(R, q, t, c=1.0)
        print(f"enh_ref_cpu wgrad {shape} {fmt} {cout}x{cin} {q} fp32 ratio {ratio:.3f}")
        assert ok and ratio <= 1.0, msg
    if multi:
        n = R["n"]["dw"]
        print(f"enh_ref_cpu wgrad {shape} non-zero terms per element: {int(n.min())} .. {int(n.max())}")
        assert float(n.max()) < 0.05 * shape[0] * shape[1] * shape[2]


# ---------------------------------------------------------------------------------------------------------------- (c) the emulation under its caps
@pytest.mark.parametrize("tag", list(ALL_RB))
def test_resblock_emulation_is_under_the_caps(tag):
    """Hard bar everywhere, at most EMU_CAP = 1.25e-4 of the outputs outside the tight bar, for the emulation that sums tap by tap as the kernel
    does.  The cap is a condition on every case: a case of 13 k elements holds it only with at most one element outside."""
    kind, shape, fmt = ALL_RB[tag]
    a, R = E.rb_operands(kind, shape, fmt), E.rb_reference(kind, shape, fmt)
    emu, mid = E.emulate_resblock(a["x"], a["w1"], a["b1"], a["w2"], a["b2"], a["act"], a["r2"], fmt, with_mid=True)
    c = E.resblock_check(R, emu)
    flipped = float((mid.double() != R["mid"]).double().mean())
    print(f"enh_ref_cpu {tag} emulation: outside tight {c['share_tight']:.2e} flipped intermediates {flipped:.2e} worst / hard bar {c['ratio_hard']:.3f}")
    assert c["ok_hard"], c["msg"]
    assert c["share_tight"] <= E.EMU_CAP, f"{tag}: {c['share_tight']:.3g} of the emulation's outputs outside the tight bar (cap {E.EMU_CAP:.3g})"


# ---------------------------------------------------------------------------------------------------------------- (d) mutations, forward kernels
class _Fwd:
    """One conv with every feature (bias, LeakyReLU, two residuals) on MUT_FWD, its reference and the pieces the mutations are made of."""
    _cache = {}

    def __new__(cls, fmt):
        if fmt not in cls._cache:
            self = super().__new__(cls)
            o = E.Operands(MUT_FWD, fmt)
            self.fmt, self.x, self.w, self.b, self.r1, self.r2 = fmt, o.x.double(), E.r16(o.w("w"), fmt), o.b("b").double(), o.r1.double(), o.r2.double()
            self.R = E.conv_reference(o.x, o.w("w"), o.b("b"), E.ACT_LEAKY, o.r1, o.r2, fmt)
            self.pre = self.conv(self.x)
            B, H, W = MUT_FWD
            self.ty_n, self.tx_n = -(-H // E.TH), -(-W // E.TW)
            self.tiles = [(b, ty, tx) for b in range(B) for ty in range(self.ty_n) for tx in range(self.tx_n)]
            cls._cache[fmt] = self
        return cls._cache[fmt]

    def conv(self, x, padding=1):
        return F.conv2d(x, self.w, self.b, padding=padding)

    def out(self, pre):
        return E.act_fwd(pre, E.ACT_LEAKY) + self.r1 + self.r2

    def sl(self, t):
        b, ty, tx = t
        return (b, slice(None), slice(ty * E.TH, min((ty + 1) * E.TH, MUT_FWD[1])), slice(tx * E.TW, min((tx + 1) * E.TW, MUT_FWD[2])))

    def detected(self, y):
        return not G.check(self.R, "y", y)[0]

    def ref(self):
        return self.R["ref"]["y"].clone()


def _report(name, fmt, hits):
    n = sum(hits)
    print(f"mutation {name} {fmt}: detected {n} of {len(hits)}")
    assert len(hits) >= 1 and n == len(hits), f"{name}: only {n} of {len(hits)} positions detected"


def _fwd_positions(c, name):
    last_y, last_x = c.ty_n - 1, c.tx_n - 1
    B = MUT_FWD[0]
    if name in ("unwritten", "no_bias", "slope_0"):
        return _pick(c.tiles)
    if name == "previous_halo":
        return _pick(t for t in c.tiles if t[0] >= 1)
    if name == "neighbour_image":
        return _pick(t for t in c.tiles if t[0] < B - 1)
    if name == "missing_halo":
        return _pick([(t, "top") for t in c.tiles if t[1] >= 1] + [(t, "bottom") for t in c.tiles if t[1] < last_y] +
                     [(t, "left") for t in c.tiles if t[2] >= 1] + [(t, "right") for t in c.tiles if t[2] < last_x])
    if name == "nonzero_pad":
        return _pick([(t, "top") for t in c.tiles if t[1] == 0 and t[0] >= 1] + [(t, "bottom") for t in c.tiles if t[1] == last_y and t[0] < B - 1] +
                     [(t, "left") for t in c.tiles if t[2] == 0] + [(t, "right") for t in c.tiles if t[2] == last_x])
    if name == "channels_swapped":
        return _pick([(t, (7 * i) % 32, (7 * i + 1 + i % 5) % 32) for i, t in enumerate(c.tiles)])
    if name == "residual_missing":
        return _pick([(t, side, r) for t in c.tiles for side in ("bottom", "right") for r in ("r1", "r2")
                      if (side == "bottom" and t[1] == last_y) or (side == "right" and t[2] == last_x)])
    raise KeyError(name)


def _edge(sl, side):
    """The tile's first / last live row or column as slices."""
    b, cc, ys, xs = sl
    if side == "top":
        return (b, cc, slice(ys.start, ys.start + 1), xs)
    if side == "bottom":
        return (b, cc, slice(ys.stop - 1, ys.stop), xs)
    if side == "left":
        return (b, cc, ys, slice(xs.start, xs.start + 1))
    return (b, cc, ys, slice(xs.stop - 1, xs.stop))


def _fwd_variants(c):
    """Whole-tensor outputs of the wrong computations the edge mutations splice from (computed once per format)."""
    if hasattr(c, "var"):
        return c.var
    B, H, W = MUT_FWD
    x = c.x
    v = {}
    rows_above = [y - 1 for y in range(E.TH, H, E.TH)]          # the halo row above / below, the halo column left / right of an interior tile edge
    cols_left = [xx - 1 for xx in range(E.TW, W, E.TW)]
    for key, dim, idx in (("top", 2, rows_above), ("bottom", 2, [y + 1 for y in rows_above]), ("left", 3, cols_left), ("right", 3, [xx + 1 for xx in cols_left])):
        xz = x.clone()
        xz.index_fill_(dim, torch.tensor(idx), 0.0)
        v["halo_" + key] = c.out(c.conv(xz))
    # a pad that is what lies next to the image in memory instead of zero: the neighbouring image's row above / below, the previous / next row's
    # end / start left / right
    xv = x.transpose(0, 1).reshape(1, 32, B * H, W)
    pv = c.conv(xv).reshape(32, B, H, W).transpose(0, 1)
    v["pad_top"] = v["pad_bottom"] = c.out(pv)
    xh = F.pad(x, (1, 1, 0, 0))
    xh[:, :, 1:, 0] = x[:, :, :-1, -1]
    xh[:, :, :-1, -1] = x[:, :, 1:, 0]
    v["pad_left"] = v["pad_right"] = c.out(F.conv2d(xh, c.w, c.b, padding=(1, 0)))
    c.var = v
    return v


def _fwd_mutant(c, name, pos):
    y = c.ref()
    ref = c.R["ref"]["y"]
    if name == "unwritten":
        y[c.sl(pos)] = 0
    elif name == "previous_halo":          # the tile computed from the halo of the block's previous trip (here: the same tile of the image before)
        s, p = c.sl(pos), c.sl((pos[0] - 1,) + pos[1:])
        y[s] = E.act_fwd(c.pre[p], E.ACT_LEAKY) + c.r1[s] + c.r2[s]
    elif name == "neighbour_image":
        y[c.sl((pos[0] + 1,) + pos[1:])] = ref[c.sl(pos)]
    elif name in ("missing_halo", "nonzero_pad"):
        t, side = pos
        e = _edge(c.sl(t), side)
        y[e] = _fwd_variants(c)[("halo_" if name == "missing_halo" else "pad_") + side][e]
    elif name == "channels_swapped":
        t, c0, c1 = pos
        b, _, ys, xs = c.sl(t)
        y[b, c0, ys, xs], y[b, c1, ys, xs] = ref[b, c1, ys, xs], ref[b, c0, ys, xs]
    elif name == "no_bias":
        s = c.sl(pos)
        y[s] = E.act_fwd(c.pre[s] - c.b.view(-1, 1, 1), E.ACT_LEAKY) + c.r1[s] + c.r2[s]
    elif name == "slope_0":
        s = c.sl(pos)
        y[s] = torch.relu(c.pre[s]) + c.r1[s] + c.r2[s]
    elif name == "residual_missing":
        t, side, r = pos
        e = _edge(c.sl(t), side)
        y[e] = y[e] - getattr(c, r)[e]
    return y


FWD_MUTATIONS = ["unwritten", "previous_halo", "neighbour_image", "missing_halo", "nonzero_pad", "channels_swapped", "no_bias", "slope_0",
                 "residual_missing"]


@pytest.mark.parametrize("fmt", E.FORMATS)
@pytest.mark.parametrize("name", FWD_MUTATIONS)
def test_forward_mutation_leaves_its_bar(name, fmt):
    c = _Fwd(fmt)
    assert c.detected(c.ref() + 1.0) and not c.detected(c.ref())
    pos = _fwd_positions(c, name)
    assert len(pos) >= NPOS, (name, len(pos))
    _report(name, fmt, [c.detected(_fwd_mutant(c, name, p)) for p in pos])


@pytest.mark.parametrize("fmt", E.FORMATS)
def test_resblock_ring_of_extrapolated_intermediates_leaves_its_bars(fmt):
    """The intermediate ring outside the image holding act(conv1) of the zero-padded input instead of zero: only the image's border outputs change.
    Every side of every image is detected, and more than a quarter of the border elements fail the HARD bar."""
    a = E.rb_operands("leaky_skip", MUT_RB, fmt)
    R = E.rb_reference("leaky_skip", MUT_RB, fmt)
    x64 = a["x"].double()
    ext = E.r16(E.act_fwd(F.conv2d(x64, E.r16(a["w1"], fmt), a["b1"].double(), padding=2), a["act"]), fmt)
    mut = E.resblock_reference(a["x"], a["w1"], a["b1"], a["w2"], a["b2"], a["act"], a["r2"], fmt, mid_override=ext)["ref"]["y"]
    B, H, W = MUT_RB
    border = torch.zeros(B, 32, H, W, dtype=torch.bool)
    border[:, :, 0], border[:, :, -1], border[:, :, :, 0], border[:, :, :, -1] = True, True, True, True
    assert torch.equal(mut[~border], R["ref"]["y"][~border])
    c = E.resblock_check(R, mut)
    hard, tight = float(c["bad_hard"][border].double().mean()), float(c["bad_tight"][border].double().mean())
    print(f"mutation resblock_ring {fmt}: {hard:.3f} of the border elements outside the hard bar, {tight:.3f} outside the tight bar")
    assert hard > 0.25 and not c["ok_hard"]
    hits = []
    for b in range(B):
        for side in (slice(0, 1), slice(H - 1, H)):
            y = R["ref"]["y"].clone()
            y[b, :, side, 1:-1] = mut[b, :, side, 1:-1]
            hits.append(not E.resblock_check(R, y)["ok_hard"])
        for side in (slice(0, 1), slice(W - 1, W)):
            y = R["ref"]["y"].clone()
            y[b, :, 1:-1, side] = mut[b, :, 1:-1, side]
            hits.append(not E.resblock_check(R, y)["ok_hard"])
    assert len(hits) >= NPOS
    _report("resblock_ring", fmt, hits)


# ---------------------------------------------------------------------------------------------------------------- (d) mutations, weight gradient
class _Wg:
    """The sparse multi-trip weight-gradient case and the contribution of any set of pixels to dw / db."""
    _one = None

    def __new__(cls):
        if cls._one is None:
            self = super().__new__(cls)
            a = E.wg_operands(E.MULTI_WG, "bf16", multi=True)
            self.R = E.cached_wg_reference(E.MULTI_WG, "bf16", 32, 32, True)
            self.xp, self.g = F.pad(a["x"].double(), (1, 1, 1, 1)), a["g"].double()
            B, H, W = E.MULTI_WG
            self.pix = torch.nonzero(a["pixels"][:, 0] & (self.g != 0).any(1))          # (P, 3): image, row, column
            sx_n = -(-W // E.STRIP)
            self.strip = (self.pix[:, 0] * H + self.pix[:, 1]) * sx_n + self.pix[:, 2] // E.STRIP
            cls._one = self
        return cls._one

    def contrib(self, pix, taps=None):
        """(dw, db) of the pixels ``pix`` (P, 3); ``taps``: only these kx."""
        dw, db = torch.zeros(32, 32, 3, 3, dtype=torch.float64), torch.zeros(32, dtype=torch.float64)
        if pix.numel() == 0:
            return dw, db
        b, y, xx = pix[:, 0], pix[:, 1], pix[:, 2]
        gp = self.g[b, :, y, xx]
        for ky in range(3):
            for kx in (range(3) if taps is None else taps):
                dw[:, :, ky, kx] = gp.t() @ self.xp[b, :, y + ky, xx + kx]
        return dw, gp.sum(0)

    def of_strips(self, ss):
        return self.pix[torch.isin(self.strip, torch.tensor(list(ss)))]

    def detected(self, dw, db=None):
        hit = not G.check(self.R, "dw", dw)[0]
        return hit if db is None else (hit, not G.check(self.R, "db", db)[0])


def test_sparse_gradient_positions_cover_the_walk_of_every_wave():
    """The non-zero pixels of the multi-trip gradient hold the first, second and third strip of a wave, the first and the last pixel of a strip and
    the 2-pixel last strip of a row; the reference re-assembled from those pixels alone IS the reference."""
    c = _Wg()
    B, H, W = E.MULTI_WG
    assert E.strips(E.MULTI_WG) > 2 * E.WG_WAVES and W % E.STRIP == 2 and E.nparts(E.MULTI_WG) == E.WG_PARTS
    info = [E.strip_of(E.MULTI_WG, int(s)) for s in c.strip]
    trips = {t for *_, t in info}
    assert trips == {0, 1, 2}
    col = c.pix[:, 2]
    first = (col % E.STRIP == 0)
    last = (col % E.STRIP == E.STRIP - 1)
    ragged = col >= (W // E.STRIP) * E.STRIP
    assert int(first.sum()) >= 1 and int(last.sum()) >= 1 and int(ragged.sum()) >= 1, (int(first.sum()), int(last.sum()), int(ragged.sum()))
    share = c.pix.shape[0] / (B * H * W)
    assert 1 / 96 < share < 1 / 48, share
    dw, db = c.contrib(c.pix)
    assert float((dw - c.R["ref"]["dw"]).abs().max()) < 1e-9 and float((db - c.R["ref"]["db"]).abs().max()) < 1e-9
    assert c.detected(c.R["ref"]["dw"], c.R["ref"]["db"]) == (False, False)


WG_MUTATIONS = ["dropped_pixel", "dropped_strip", "other_lds_buffer", "x_column_missing", "block_partial_left_out"]


@pytest.mark.parametrize("name", WG_MUTATIONS)
def test_weight_gradient_mutation_leaves_its_bar(name):
    c = _Wg()
    ref_dw, ref_db = c.R["ref"]["dw"], c.R["ref"]["db"]
    nw = E.WG_WAVES
    live = sorted(set(int(s) for s in c.strip))
    hits, hits_db = [], []
    if name == "dropped_pixel":
        for i in _pick(range(c.pix.shape[0]), 41):
            dw, db = c.contrib(c.pix[i:i + 1])
            changed = dw != 0
            caught = (dw.abs() > G.bars(c.R, "dw"))[changed]
            hits.append(bool(caught.all()) and c.detected(ref_dw - dw))
            hits_db.append(c.detected(ref_dw - dw, ref_db - db)[1])
    elif name == "dropped_strip":
        for s in _pick(live):
            dw, db = c.contrib(c.of_strips([s]))
            hits.append(c.detected(ref_dw - dw))
            hits_db.append(c.detected(ref_dw - dw, ref_db - db)[1])
    elif name == "other_lds_buffer":          # strip s computed from the buffer that still holds the wave's previous strip s - 1024
        both = [s for s in range(nw, E.strips(E.MULTI_WG)) if s in set(live) or (s - nw) in set(live)]
        for s in _pick(both):
            d0, b0 = c.contrib(c.of_strips([s]))
            d1, b1 = c.contrib(c.of_strips([s - nw]))
            hits.append(c.detected(ref_dw - d0 + d1))
    elif name == "x_column_missing":          # the halo column x0 - 1 (tap column 0 of a strip's first pixel) or x0 + 64 (tap column 2 of its last)
        W = E.MULTI_WG[2]
        col = c.pix[:, 2]
        left = c.pix[(col % E.STRIP == 0) & (col > 0)]
        right = c.pix[(col % E.STRIP == E.STRIP - 1) & (col + 1 < W)]
        assert left.shape[0] + right.shape[0] >= NPOS, (left.shape, right.shape)
        for p in _pick(range(left.shape[0]), NPOS // 2):
            hits.append(c.detected(ref_dw - c.contrib(left[p:p + 1], taps=(0,))[0]))
        for p in _pick(range(right.shape[0]), NPOS // 2):
            hits.append(c.detected(ref_dw - c.contrib(right[p:p + 1], taps=(2,))[0]))
    elif name == "block_partial_left_out":          # block k's partial: the strips of its four waves, every trip
        for k in _pick(range(E.WG_PARTS)):
            ss = [s for s in live if (s % nw) // 4 == k]
            dw, db = c.contrib(c.of_strips(ss))
            hits.append(c.detected(ref_dw - dw))
            hits_db.append(c.detected(ref_dw - dw, ref_db - db)[1])
    assert len(hits) >= NPOS
    if hits_db:
        print(f"mutation {name} bf16: bias gradient detected {sum(hits_db)} of {len(hits_db)}")
        assert all(hits_db)
    _report(name, "bf16", hits)


@pytest.mark.parametrize("np_", list(E.FINISH_SHAPES))
def test_finish_mutations_leave_their_bar(np_):
    """On the finish-kernel shapes (nparts = 1 .. 7 and 256, dense operands): every block partial left out, and ``accumulate`` ignoring the
    slots' previous contents."""
    shape = E.FINISH_SHAPES[np_]
    assert E.nparts(shape) == np_
    a = E.wg_operands(shape, "bf16")
    R = E.cached_wg_reference(shape, "bf16", 32, 32, False)
    g = a["g"].double()
    nw = np_ * 4
    hits = []
    for k in _pick(range(np_)):
        gk = torch.zeros_like(g)
        for s in range(E.strips(shape)):
            if (s % nw) // 4 == k:
                b, y, x0, n, _, _ = E.strip_of(shape, s)
                gk[b, :, y, x0:x0 + n] = g[b, :, y, x0:x0 + n]
        dw = torch.nn.grad.conv2d_weight(a["x"].double(), (32, 32, 3, 3), gk, padding=1)
        hits.append(not G.check(R, "dw", R["ref"]["dw"] - dw)[0] and not G.check(R, "db", R["ref"]["db"] - gk.sum((0, 2, 3)))[0])
    _report(f"finish_partial_left_out_nparts_{np_}", "bf16", hits)
    hits = []
    for salt in range(4):
        prev = E.previous_slots(shape, salt=salt)
        Ra = E.wgrad_reference(a["x"], a["g"], a["w"], a["b"], prev=prev)
        assert G.check(Ra, "dw", Ra["ref"]["dw"])[0]
        hits.append(not G.check(Ra, "dw", R["ref"]["dw"])[0] and not G.check(Ra, "db", R["ref"]["db"])[0])
    _report(f"accumulate_ignored_nparts_{np_}", "bf16", hits)


def test_the_multi_trip_shapes_pass_their_launch_caps():
    """More than two trips' worth of tiles / strips, ragged on the right and at the bottom, images ending in mid-loop (the tile count per image does
    not divide the grid).  The caps are copied from the host code of enh.hip; a change there must be followed in enh_ref.py."""
    B, H, W = E.MULTI_FWD
    assert E.tiles(E.MULTI_FWD) > 2 * E.FWD_BLOCKS and H % E.TH and W % E.TW and E.FWD_BLOCKS % (E.tiles(E.MULTI_FWD) // B)
    B, H, W = E.MULTI_RB
    assert E.tiles(E.MULTI_RB, E.RB_TH, E.RB_TW) > 2 * E.RB_BLOCKS and H % E.RB_TH and W % E.RB_TW and E.RB_BLOCKS % (E.tiles(E.MULTI_RB, E.RB_TH, E.RB_TW) // B)
    assert [E.nparts(s) for s in E.FINISH_SHAPES.values()] == list(E.FINISH_SHAPES)
    assert E.tiles((1, 16, 32)) == 1 and E.tiles((2, 17, 33)) == 8 and E.tiles((1, 14, 30), E.RB_TH, E.RB_TW) == 1


def teardown_module():
    E.clear_cache()
    _Fwd._cache.clear()
    _Wg._one = None

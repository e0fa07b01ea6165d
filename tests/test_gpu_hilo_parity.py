"""Per-element fp64 parity of the hi/lo ("pair", bf16x3) analysis kernels on a real MI355X, in both 16-bit libraries: the image stage
(csrc/sconv_hilo.hip: ``n2w_gdn_hilo_kernel<INV, OUT1>`` x 4 with the weight image of ``n2w_hilo_pack_kernel``), ``im2col_hilo_kernel``
(csrc/glue.hip), the HL = 1 / 2 main loop of ``igemm_glds_kernel`` with its GDN = 3 / 4 epilogue at the 32 / 64 / 128 / 256 pixel tiles, the
HL = 0 form behind ``hesic_conv2d_gdn_forward_hilo_out``, the plain pair epilogue (y_hilo, y_abs, y32, acc_scale; cout tile 64) and
``splitk_reduce_kernel``'s pair outputs (csrc/conv_igemm.hip).

Every case of tests/hilo_ref.py's tables runs through the wrappers the models use (``Fn.sconv_gdn_hilo`` + ``PackedN2wHiLo``,
``Fn.im2col_hilo``, ``Fn.conv2d_hilo`` + ``PackedWeightHiLo`` / ``PackedGdnLo``, ``Fn.conv2d_gdn_hilo_out``); the class-isolation launches
pack their hand-built weight halves through the C ABI (``hesic_pack_conv_weight``) and the acc_scale case names its factor itself
(``hesic_conv2d_hilo_set_acc_scale``, through the wrapper's attribute).  EVERY element of every output is checked (tests/hilo_ref.py: sum,
pair, abs, y32, same), every wide and plain case asserts its planned tile through ``hesic_conv2d_hilo_variant`` before it runs, and the
multi-trip image cases, one wide case per tile size and one split-K case run once more inside guarded and poisoned allocations
(tests/memguard.py).  tests/test_hilo_ref_cpu.py shows on the CPU which defects these checks fail.

Each case prints  "hilo_parity <case> <output> <ratio>"  before anything is asserted.  The values measured when the tests were written are
in profiles/hilo_parity.json."""
import contextlib
import ctypes as C

import pytest
import torch

import conv_grad_ref as G
import fused_gdn_ref as Fz
import hilo_ref as Hz
import memguard as MG

pytestmark = pytest.mark.gpu
DEV = "cuda"
CL = torch.channels_last
NAMES = Hz.NAMES


@contextlib.contextmanager
def _library(fmt):
    import hesic_amd
    hesic_amd.set_compute_dtype(Hz.FMT[fmt]["dtype"])
    try:
        yield
    finally:
        hesic_amd.set_compute_dtype(torch.bfloat16)
        hesic_amd.set_compute_dtype(torch.float32)


class _Placer:
    """Operands to the device -- inside NaN guards when ``guard`` is set."""

    def __init__(self, fmt, guard):
        self.dt, self.guard, self.kept = Hz.FMT[fmt]["dtype"], guard, []

    def put(self, t, name, dtype=None, nhwc=False):
        if t is None:
            return None
        t = t.to(DEV, dtype or t.dtype)
        t = t.contiguous(memory_format=CL) if nhwc else t.contiguous()
        if self.guard:
            t = MG.guarded(t, name=name)
            self.kept.append(t)
        return t

    def pair(self, hi, lo, name):
        """The [hi | lo] NHWC tensor of two fp32 tensors holding 16-bit-exact values."""
        return self.put(torch.cat((hi, lo), 1), name, self.dt, nhwc=True)

    def check(self):
        MG.check_all(self.kept)


def _allocations(guard):
    from hesic_amd import functional
    return MG.poisoned_allocations([functional]) if guard else contextlib.nullcontext([None])


def _report(case, res):
    """Print every figure, then assert: ``res`` = {check: (ok, ratio, message)}."""
    for q, (ok, ratio, msg) in res.items():
        print(f"hilo_parity {case} {q} {ratio:.4f}")
    for q, (ok, ratio, msg) in res.items():
        assert ok, f"{case} {msg}"


def _finite(case, guard, *ts):
    if guard:
        for t in ts:
            assert t is None or bool(torch.isfinite(t.float()).all()), f"{case}: poison in an output"


def _outputs(R, y, y32=None):
    """The (P, C) fp64 outputs ``Hz.check`` reads."""
    C_ = R["shape"][1]
    out = {}
    if y is not None:
        assert y.is_contiguous(memory_format=CL) and tuple(y.shape) == (R["shape"][0], (2 if R["pair_out"] else 1) * C_) + R["shape"][2:]
        if R["pair_out"]:
            out["hi"], out["lo"] = Hz.halves(y, C_)
        else:
            out["y"] = Hz.to_pc(y.detach().cpu().double())
    if y32 is not None:
        assert y32.dtype == torch.float32 and tuple(y32.shape) == R["shape"]
        out["y32"] = Hz.to_pc(y32.detach().cpu().double())
    return out


def _gdn_packs(Fn, beta, gamma):
    gp, bp = Fn.PackedGdn().get(beta, gamma, 1e-6)
    return gp, Fn.PackedGdnLo().get(gamma), bp


def _assert_plan(cin, cout, k, s, shape, products, gdn, want):
    from hesic_amd import _lib as L
    B, H, W = shape
    Ho, Wo = G.out_hw(H, W, k, s, k // 2, False)
    d = L.ConvDesc(B, H, W, cin, Ho, Wo, cout, k, k, s, k // 2, 0, L.H16, 0, 0, (1 if products == 1 else 2) * cin, 0, 2 * cout, 0, 0)
    v = (C.c_int * 4)()
    L.call("hesic_conv2d_hilo_variant", C.byref(d), products, gdn, v)
    assert tuple(v)[:len(want)] == tuple(want), f"planned {tuple(v)}, the case table says {want}"


# ------------------------------------------------------------------------------------------------------------------------ image stage
def _run_image(tag, fmt, form, inverse, guard=False):
    from hesic_amd import functional as Fn
    (B, H, W), opt = Hz.IMAGE[tag]
    o = Hz.image_operands(tag, fmt, form, Hz.image_scaled(fmt, form, inverse))
    out1 = form == "out1"
    case = f"{tag}_{fmt}_{form}_{NAMES[inverse]}" + ("_guarded" if guard else "")
    with _library(fmt):
        P = _Placer(fmt, guard)
        top, left = o["crop"]
        x = P.put(o["full"], "x")[:, :, top:top + H, left:left + W]
        w, b = P.put(o["w"], "w"), P.put(o["b"], "b")
        beta, gamma = P.put(o["beta"], "beta"), P.put(o["gamma"], "gamma")
        assert Fn.sconv_gdn_hilo_ok(x, w) and (x.is_contiguous() == ("crop" not in opt))
        with _allocations(guard) as rec, torch.no_grad():
            _, bp = Fn.PackedGdn().get(beta, gamma, 1e-6)
            y = Fn.sconv_gdn_hilo(x, Fn.PackedN2wHiLo().get(w, gamma, out1=out1, inverse=inverse), b, bp, inverse, out1=out1)
            torch.cuda.synchronize()
        assert rec, "no allocation of the package was guarded"
        P.check()
    assert y.dtype == Hz.FMT[fmt]["dtype"]
    _finite(case, guard, y)
    R = Hz.image_reference(tag, fmt, form, inverse)
    out = _outputs(R, y)
    _report(case, Hz.check(R, out))
    if opt.get("zero_corner"):
        dead = R["dead"]
        assert int(dead.sum()) >= 128 * 2 * 19 * 19
        for t in out.values():
            assert bool((t[dead] == 0).all()), f"{case}: a half that is not exactly 0 behind an all-zero receptive field"


IMAGE_RUNS = [(t, f, m, i) for f in Hz.FORMATS for t, m, i in Hz.image_runs()]


@pytest.mark.parametrize("tag,fmt,form,inverse", IMAGE_RUNS, ids=[f"{t}-{f}-{m}-{NAMES[i]}" for t, f, m, i in IMAGE_RUNS])
def test_image_stage(tag, fmt, form, inverse):
    if tag in Hz.IMAGE_TRIPS:
        tiles, grid, per_trip = Fz.image_tiles(Hz.IMAGE[tag][0])
        assert tiles > per_trip * (Hz.IMAGE_TRIPS[tag] - 1)
    _run_image(tag, fmt, form, inverse)


@pytest.mark.parametrize("fmt", Hz.FORMATS)
@pytest.mark.parametrize("tag", [t for t, c in Hz.IMAGE.items() if c[1].get("guard")])
def test_image_stage_multi_trip_guarded(tag, fmt):
    for form in Hz.IMAGE_FORMS:
        _run_image(tag, fmt, form, False, guard=True)


# ------------------------------------------------------------------------------------------------------------------------ im2col route
@pytest.mark.parametrize("fmt", Hz.FORMATS)
@pytest.mark.parametrize("tag", list(Hz.IM2COL))
def test_im2col_route(tag, fmt):
    """The columns bit for bit against the host split (pad columns and out-of-image taps exactly 0), then the 1 x 1 pair conv + (I)GDN on them."""
    from hesic_amd import functional as Fn
    o = Hz.im2col_operands(tag, fmt)
    B, _, H, W = o["x"].shape
    Ho, Wo = G.out_hw(H, W, 5, 2, 2, False)
    with _library(fmt):
        P = _Placer(fmt, False)
        x = P.put(o["x"], "x", nhwc=o["nhwc"])
        w, b = P.put(o["w"], "w"), P.put(o["b"], "b")
        beta, gamma = P.put(o["beta"], "beta"), P.put(o["gamma"], "gamma")
        _assert_plan(Hz.KP, 128, 1, 1, (B, Ho, Wo), 3, 3, Hz.IM2COL_PLAN)
        with torch.no_grad():
            cols = Fn.im2col_hilo(x, 5, 2, 2, Hz.KP)
            wp = Fn.PackedWeightHiLo().get(w, as_1x1=True, kp=Hz.KP)
            assert getattr(wp, "hesic_acc_scale", 1.0) == o["acc_scale"]
            gp, glo, bp = _gdn_packs(Fn, beta, gamma)
            ys = {inv: Fn.conv2d_hilo(cols, wp, b, Hz.KP, 128, kernel_size=1, stride=1, padding=0, gdn=(gp, glo, bp, inv)) for inv in (False, True)}
            torch.cuda.synchronize()
    assert tuple(cols.shape) == (B, 2 * Hz.KP, Ho, Wo) and cols.is_contiguous(memory_format=CL)
    got = cols.float().cpu()
    want = torch.cat((o["ch"], o["cl"]), 1)
    assert torch.equal(got, want), f"{tag}_{fmt}: {int((got != want).sum())} column values differ from the host split"
    assert bool((got[:, 75:Hz.KP] == 0).all()) and bool((got[:, Hz.KP + 75:] == 0).all()) and bool((got[:, 0, 0, 0] == 0).all())
    for inv, y in ys.items():
        R = Hz.im2col_reference(tag, fmt, inv)
        _report(f"{tag}_{fmt}_{NAMES[inv]}", Hz.check(R, _outputs(R, y)))


# ------------------------------------------------------------------------------------------------------------------------ wide stage
def _run_wide(tag, fmt, products, inverse, guard=False):
    from hesic_amd import functional as Fn
    Cin, k, s, shape, _, opt = Hz.WIDE[tag]
    o = Hz.wide_operands("wide", tag, fmt, products)
    case = f"{tag}_{fmt}_x{products}_{NAMES[inverse]}" + ("_guarded" if guard else "")
    with _library(fmt):
        P = _Placer(fmt, guard)
        x = P.pair(o["xh"], o["xl"], "x")
        w, b = P.put(o["w"], "w"), P.put(o["b"], "b")
        beta, gamma = P.put(o["beta"], "beta"), P.put(o["gamma"], "gamma")
        _assert_plan(Cin, 128, k, s, shape, products, 4 if inverse else 3, Hz.wide_plan(tag, products, inverse))
        with _allocations(guard) as rec, torch.no_grad():
            wp = Fn.PackedWeightHiLo().get(w, single=(products == 2))
            assert getattr(wp, "hesic_acc_scale", 1.0) == o["acc_scale"]
            y = Fn.conv2d_hilo(x, wp, b, Cin, 128, kernel_size=k, stride=s, padding=k // 2, gdn=_gdn_packs(Fn, beta, gamma) + (inverse,),
                               products=products)
            torch.cuda.synchronize()
        assert rec, "no allocation of the package was guarded"
        P.check()
    _finite(case, guard, y)
    R = Hz.wide_reference(tag, fmt, products, inverse)
    _report(case, Hz.check(R, _outputs(R, y)))


WIDE_RUNS = [(t, f, p, i) for f in Hz.FORMATS for t, p, i in Hz.wide_runs()]


@pytest.mark.parametrize("tag,fmt,products,inverse", WIDE_RUNS, ids=[f"{t}-{f}-x{p}-{NAMES[i]}" for t, f, p, i in WIDE_RUNS])
def test_wide_stage(tag, fmt, products, inverse):
    _run_wide(tag, fmt, products, inverse)


@pytest.mark.parametrize("fmt", Hz.FORMATS)
@pytest.mark.parametrize("tag", [t for t, c in Hz.WIDE.items() if c[5].get("guard")])
def test_wide_stage_guarded(tag, fmt):
    """One case per pixel tile (32 / 64 / 128 / 256), three products, GDN."""
    _run_wide(tag, fmt, 3, False, guard=True)


def _run_hilo_out(tag, fmt, inverse, guard=False):
    from hesic_amd import functional as Fn
    Cin, k, s, shape, plan, _ = Hz.HILO_OUT[tag]
    o = Hz.wide_operands("out", tag, fmt, 1)
    case = f"{tag}_{fmt}_{NAMES[inverse]}" + ("_guarded" if guard else "")
    with _library(fmt):
        P = _Placer(fmt, guard)
        x = P.put(o["xh"], "x", P.dt, nhwc=True)
        w, b = P.put(o["w"], "w"), P.put(o["b"], "b")
        beta, gamma = P.put(o["beta"], "beta"), P.put(o["gamma"], "gamma")
        _assert_plan(Cin, 128, k, s, shape, 1, 4 if inverse else 3, plan)
        with _allocations(guard) as rec, torch.no_grad():
            wp = Fn.PackedWeight().get(w, None, 128, Cin, k, k, False, False, x.dtype)
            y = Fn.conv2d_gdn_hilo_out(x, wp, b, Cin, kernel_size=k, stride=s, padding=k // 2, gdn=_gdn_packs(Fn, beta, gamma) + (inverse,))
            torch.cuda.synchronize()
        assert rec, "no allocation of the package was guarded"
        P.check()
    _finite(case, guard, y)
    R = Hz.hilo_out_reference(tag, fmt, inverse)
    _report(case, Hz.check(R, _outputs(R, y)))


OUT_RUNS = [(t, f, i) for f in Hz.FORMATS for t, i in Hz.hilo_out_runs()]


@pytest.mark.parametrize("tag,fmt,inverse", OUT_RUNS, ids=[f"{t}-{f}-{NAMES[i]}" for t, f, i in OUT_RUNS])
def test_hilo_out(tag, fmt, inverse):
    _run_hilo_out(tag, fmt, inverse)


@pytest.mark.parametrize("fmt", Hz.FORMATS)
def test_hilo_out_guarded(fmt):
    _run_hilo_out("o_c32_t64", fmt, False, guard=True)


# ------------------------------------------------------------------------------------------------------------------------ plain pair conv
def _conv_plain(Fn, x, wp, b, cin, cout, k, s, opt, products):
    res = Fn.conv2d_hilo(x, wp, b, cin, cout, kernel_size=k, stride=s, padding=k // 2, act=opt.get("act", G.ACT_NONE), out=opt.get("out", "both"),
                         out_abs=opt.get("y_abs", False), products=products)
    out = opt.get("out", "both")
    return res if out == "both" else ((res, None) if out == "hilo" else (None, res))


def _run_plain(tag, fmt, products, guard=False, no_split=False):
    from hesic_amd import functional as Fn
    Cin, Cout, k, s, shape, plan, opt = Hz.PLAIN[tag]
    o = Hz.wide_operands("plain", tag, fmt, products)
    case = f"{tag}_{fmt}_x{products}" + ("_nosplit" if no_split else "") + ("_guarded" if guard else "")
    with _library(fmt):
        P = _Placer(fmt, guard)
        x = P.pair(o["xh"], o["xl"], "x")
        w, b = P.put(o["w"], "w"), P.put(o["b"], "b")
        _assert_plan(Cin, Cout, k, s, shape, products, 0, plan)
        with _allocations(guard) as rec, torch.no_grad(), (Fn.no_split_k() if no_split else contextlib.nullcontext()):
            wp = Fn.PackedWeightHiLo().get(w, single=(products == 2))
            if "acc" in opt:                              # weights times 1 / acc_scale, the factor named for this launch
                assert getattr(wp, "hesic_acc_scale", 1.0) == 1.0
                wp.hesic_acc_scale = opt["acc"]
            assert getattr(wp, "hesic_acc_scale", 1.0) == o["acc_scale"]
            y, y32 = _conv_plain(Fn, x, wp, b, Cin, Cout, k, s, opt, products)
            torch.cuda.synchronize()
        assert rec, "no allocation of the package was guarded"
        P.check()
    _finite(case, guard, y, y32)
    R = Hz.plain_reference(tag, fmt, products)
    _report(case, Hz.check(R, _outputs(R, y, y32)))


PLAIN_RUNS = Hz.plain_runs()


@pytest.mark.parametrize("tag,products,fmt", PLAIN_RUNS, ids=[f"{t}-x{p}-{f}" for t, p, f in PLAIN_RUNS])
def test_plain(tag, products, fmt):
    _run_plain(tag, fmt, products)
    if Hz.PLAIN[tag][6].get("no_split"):                  # the same launch without its workspace: one block per tile, (64, 64, 128)
        _run_plain(tag, fmt, products, no_split=True)


@pytest.mark.parametrize("fmt", Hz.FORMATS)
def test_plain_split_k_guarded(fmt):
    _run_plain("p_splitk", fmt, 3, guard=True)


# ------------------------------------------------------------------------------------------------------------------------ class isolation
def _pack_halves(L, wh, wl):
    """[w_hi | w_lo] of hand-built halves in the kernels' [tap][Cout][2 Cin] layout (what PackedWeightHiLo.get does behind its own split)."""
    w2 = torch.cat((wh, wl), 1).to(DEV).contiguous()
    cout, cin2, kh, kw = w2.shape
    wp = torch.empty(kh * kw * cout * cin2, dtype=L.h16_dtype(), device=DEV)
    L.call("hesic_pack_conv_weight", L.ptr(w2), None, L.ptr(wp), cout, cin2, kh, kw, 0, 0, L.H16, L.stream())
    return wp


@pytest.mark.parametrize("fmt", Hz.FORMATS)
@pytest.mark.parametrize("products", [3, 2])
def test_class_isolation(fmt, products):
    """The same launch four times on hand-built halves: (x_hi, 0) (w_hi, 0), (0, x_lo) (w_hi, 0), (x_hi, 0) (0, w_lo), (0, x_lo) (0, w_lo),
    the lo halves of ordinary size: each product class at full magnitude.  A class the form does not have returns exactly the bias; with
    two products the unread weight half, filled with large finite values, does not change a bit of the output."""
    from hesic_amd import functional as Fn, _lib as L
    Cin, Cout, k, s, shape = Hz.ISOLATION
    base = Hz.isolation_operands(fmt, products)
    with _library(fmt):
        _assert_plan(Cin, Cout, k, s, shape, products, 0, (128, 128, 64))
        P = _Placer(fmt, False)
        b = P.put(base["b"], "b")
        run = lambda x, wp: Fn.conv2d_hilo(x, wp, b, Cin, Cout, kernel_size=k, stride=s, padding=k // 2, out="both", products=products)
        for cls in Hz.ISO_CLASSES:
            R, (xh, xl, wh, wl) = Hz.isolation_reference(fmt, products, cls)
            with torch.no_grad():
                x = P.pair(xh, xl, "x")
                y, y32 = run(x, _pack_halves(L, wh, wl))
                if products == 2:
                    junk = torch.full_like(wl, 30000.0 if fmt == "f16" else 3.0e30)
                    y2, y32b = run(x, _pack_halves(L, wh, junk))
                    assert torch.equal(y, y2) and torch.equal(y32, y32b), f"iso_{cls}_{fmt}_x2: the unread weight half changes the output"
                torch.cuda.synchronize()
            out = _outputs(R, y, y32)
            _report(f"iso_{cls}_{fmt}_x{products}", Hz.check(R, out))
            if cls == "ll" or (products == 2 and cls == "hl"):
                bias = base["b"].double().view(1, -1).expand_as(out["y32"])
                assert torch.equal(out["y32"], bias), f"iso_{cls}_{fmt}_x{products}: not exactly the bias"


def teardown_module():
    Hz.clear_cache()


def test_igdn_image_launch_refuses_a_scaled_weight_image():
    """GDN's quotient is invariant under the binary16 weight scaling of the pair image, IGDN's product is not: the IGDN launch takes the
    unscaled image (``PackedN2wHiLo.get(inverse=True)``) and the wrapper refuses the scaled one instead of returning y 4^s."""
    from hesic_amd import functional as Fn
    o = Hz.image_operands("img_6x6", "f16", "pair")
    with _library("f16"):
        P = _Placer("f16", False)
        x, w, b, beta, gamma = (P.put(o[k], k) for k in ("x", "w", "b", "beta", "gamma"))
        with torch.no_grad():
            _, bp = Fn.PackedGdn().get(beta, gamma, 1e-6)
            packer = Fn.PackedN2wHiLo()
            scaled, plain = packer.get(w, gamma), packer.get(w, gamma, inverse=True)
            assert scaled.hesic_wscale > 1.0 and plain.hesic_wscale == 1.0 and packer.get(w, gamma) is scaled
            with pytest.raises(ValueError, match="unscaled weight image"):
                Fn.sconv_gdn_hilo(x, scaled, b, bp, True)
            torch.cuda.synchronize()

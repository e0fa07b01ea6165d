"""Per-element fp64 parity of the warp kernels (csrc/warp.hip) and of the map / reduction half of csrc/glue.hip on a real MI355X.

Every case runs the bf16 library through ``hesic_amd.functional`` (or the C ABI where a route needs it: an unaligned pointer, no arg-max,
strided views, a destination offset) and checks every element against the fp64 reference and bar of tests/glue_ref.py; the copies, casts,
roundings, activation gradients and the spatial maximum are compared bit for bit / value for value.  The forward-only 16-bit cases (warp at
C = 128, upsample4 and upsample4_cat forward, copy_channels, cast, round, spatial_max without arg-max, sum_sq_diff with a 16-bit operand) also run
on the IEEE-half library.  tests/test_glue_ref_cpu.py shows on the CPU that the bars reject a dropped tap, a shifted block, a dropped n, dropped
remainder pixels, a wrong tie and the -inf of a signed-zero channel.  Each case prints  "glue_parity <case> <output> <ratio>"  (ratio = max_e
(|err_e| - storage term) / unit bound; 0 for an exact match, inf for a mismatch) before it asserts; the values measured when the tests were
written are in profiles/glue_parity.json."""
import ctypes as C
import math

import pytest
import torch

import glue_ref as G

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF, F16, F32 = torch.bfloat16, torch.float16, torch.float32
CL = torch.channels_last


@pytest.fixture(autouse=True)
def _bf16_library():
    import hesic_amd
    hesic_amd.set_compute_dtype(BF)
    yield
    hesic_amd.set_compute_dtype(BF)
    hesic_amd.set_compute_dtype(F32)


def _library(h16):
    """Select the 16-bit library for the rest of the test (the fixture restores bf16 / fp32)."""
    import hesic_amd
    hesic_amd.set_compute_dtype(h16)


def _imp():
    from hesic_amd import functional as Fn
    from hesic_amd import _lib as L
    return Fn, L


def _name(dt):
    return {BF: "bf16", F16: "f16", F32: "f32"}[dt]


def _bar(case, out, R, got, c=1.0):
    torch.cuda.synchronize()
    ok, ratio, msg = G.check(R, got, c=c, name=f"{case} {out}")
    print(f"glue_parity {case} {out} {ratio:.4f}")
    return ok, ratio, msg, c


def _assert_bars(results):
    for ok, ratio, msg, c in results:
        assert ok, msg
        assert ratio <= c, msg


def _exact(case, out, got, want, bits=True):
    torch.cuda.synchronize()
    same = G.same_bits(got, want) if bits else (got.shape == want.shape and torch.equal(got.cpu(), want))
    print(f"glue_parity {case} {out} {0.0 if same else math.inf:.4f}")
    return same, f"{case} {out}: not equal"


def _assert_exact(results):
    for same, msg in results:
        assert same, msg


# ------------------------------------------------------------------------------------------------------------------------ warp
def _warp_src(tag, h16=None):
    B, Cc, hw, dsize, ac, inv, layout, is16, _ = G.WARP[tag]
    o = G.warp_operands(tag)
    src = o["src"].to(DEV, h16 if is16 else F32)
    return (src.contiguous(memory_format=CL) if layout == "nhwc" else src), o["M"].to(DEV), o


@pytest.mark.parametrize("tag", G.WARP_FWD)
def test_warp_forward(tag):
    Fn, L = _imp()
    B, Cc, hw, dsize, ac, inv, layout, is16, _ = G.WARP[tag]
    res = []
    for h16 in ((BF, F16) if is16 else (None,)):
        if h16 is not None:
            _library(h16)
        src, M, _ = _warp_src(tag, h16)
        if layout == "nhwc":
            assert src.stride(3) == Cc
        with torch.no_grad():
            dst = Fn.warp_perspective(src, M, dsize, align_corners=ac, inverse_map=inv)
        assert dst.dtype == src.dtype and tuple(dst.shape) == (B, Cc, *dsize)
        res.append(_bar(f"warp_{tag}" + (f"_{_name(h16)}" if h16 else ""), "dst", G.warp_reference(tag, h16), dst))
    _assert_bars(res)


@pytest.mark.parametrize("tag", G.WARP_BWD)
def test_warp_backward_source_gradient(tag):
    Fn, L = _imp()
    B, Cc, hw, dsize, ac, inv, *_ = G.WARP[tag]
    src, M, o = _warp_src(tag)
    src.requires_grad_()
    Fn.warp_perspective(src, M, dsize, align_corners=ac, inverse_map=inv).backward(o["g"].to(DEV))
    assert src.grad.dtype == F32
    _assert_bars([_bar(f"warp_{tag}", "dsrc", G.warp_backward_reference(tag), src.grad, c=G.C_BAR)])


# ------------------------------------------------------------------------------------------------------------------- upsample4
@pytest.mark.parametrize("dt", [F32, BF, F16], ids=_name)
@pytest.mark.parametrize("tag", list(G.UPSAMPLE))
def test_upsample4_forward(tag, dt):
    Fn, L = _imp()
    if dt != F32:
        _library(dt)
    R = G.upsample_reference(tag, dt)
    with torch.no_grad():
        up = Fn.upsample4(R["z"].to(DEV, dt))
    assert up.dtype == dt
    _assert_bars([_bar(f"upsample4_{tag}_{_name(dt)}", "y", R["fwd"], up)])


@pytest.mark.parametrize("dt", [F32, BF], ids=_name)
@pytest.mark.parametrize("tag", list(G.UPSAMPLE))
def test_upsample4_backward(tag, dt):
    Fn, L = _imp()
    R = G.upsample_reference(tag, dt)
    z = R["z"].to(DEV, dt).requires_grad_()
    Fn.upsample4(z).backward(R["g"].to(DEV, dt))
    assert z.grad.dtype == dt
    _assert_bars([_bar(f"upsample4_{tag}_{_name(dt)}", "dz", R["bwd"], z.grad, c=G.C_BAR)])


@pytest.mark.parametrize("dt", [F32, BF], ids=_name)
@pytest.mark.parametrize("tag", list(G.CAT))
def test_upsample4_cat_forward_and_backward(tag, dt):
    """The interpolated half against the bars, the copied half (and its gradient) bit for bit."""
    Fn, L = _imp()
    Cz, Cy = G.CAT[tag]
    R = G.upsample_reference(tag, dt)
    B, _, H, W = R["z"].shape
    y1 = G.grid16(f"cat.{tag}.y", (B, Cy, 4 * H, 4 * W)).to(dt)
    gy = G.grid16(f"cat.{tag}.gy", (B, Cy, 4 * H, 4 * W)).to(dt)
    z, yd = R["z"].to(DEV, dt).requires_grad_(), y1.to(DEV).requires_grad_()
    cat = Fn.upsample4_cat(z, yd)
    assert cat.dtype == dt and cat.shape[1] == Cz + Cy
    case = f"upsample4_cat_{tag}_{_name(dt)}"
    bars = [_bar(case, "y", R["fwd"], cat[:, :Cz])]
    exact = [_exact(case, "copied", cat[:, Cz:].detach(), y1)]
    cat.backward(torch.cat((R["g"].to(dt), gy), 1).to(DEV))
    bars.append(_bar(case, "dz", R["bwd"], z.grad, c=G.C_BAR))
    exact.append(_exact(case, "dy1", yd.grad, gy))
    _assert_bars(bars)
    _assert_exact(exact)


@pytest.mark.parametrize("h16", [BF, F16], ids=_name)
@pytest.mark.parametrize("tag", list(G.CAT))
def test_upsample4_cat_forward_16bit(tag, h16):
    """The inference form (no graph) on both 16-bit libraries: the interpolated half against its bar, the copied half bit for bit."""
    Fn, L = _imp()
    _library(h16)
    Cz, Cy = G.CAT[tag]
    R = G.upsample_reference(tag, h16)
    B, _, H, W = R["z"].shape
    y1 = G.grid16(f"cat.{tag}.y", (B, Cy, 4 * H, 4 * W)).to(h16)
    with torch.no_grad():
        cat = Fn.upsample4_cat(R["z"].to(DEV, h16), y1.to(DEV))
    assert cat.dtype == h16 and cat.shape[1] == Cz + Cy
    case = f"upsample4_cat_{tag}_{_name(h16)}_nograd"
    bars = [_bar(case, "y", R["fwd"], cat[:, :Cz])]
    exact = [_exact(case, "copied", cat[:, Cz:], y1)]
    _assert_bars(bars)
    _assert_exact(exact)


def test_upsample4_grid_stride_loops():
    """More work items than 2048 blocks hold in upsample4_fwd_v8_kernel (bf16 forward) and in upsample4_bwd_kernel (fp32 backward)."""
    Fn, L = _imp()
    (tag, (B, Cc, H, W)), = G.UPSAMPLE_LOOPS.items()
    assert Cc % 8 == 0 and 16 * B * H * W * Cc // 8 > 2048 * 256 and B * H * W * Cc > 2048 * 256
    R = G.upsample_reference(tag)
    with torch.no_grad():
        up = Fn.upsample4(R["z"].to(DEV, BF))
    res = [_bar(f"upsample4_{tag}_bf16", "y", dict(R["fwd"], store=G.storage(R["fwd"]["ref"], BF)), up)]
    z = R["z"].to(DEV).requires_grad_()
    Fn.upsample4(z).backward(R["g"].to(DEV))
    res.append(_bar(f"upsample4_{tag}_f32", "dz", R["bwd"], z.grad, c=G.C_BAR))
    _assert_bars(res)


# --------------------------------------------------------------------------------- copy_channels, cast, round, act_backward
# (P, C, xps, xco, yps, yco, dtype): whole 16-byte chunks with offsets; C * es % 16 != 0; a destination offset that breaks the 16-byte
# alignment of a chunkable copy; above 524288 work items in the chunked (2 chunks a pixel) and the scalar kernel
COPIES = {
    "chunks_h16":    (37, 8, 8, 0, 24, 16, BF),
    "chunks_f32":    (37, 4, 12, 4, 8, 4, F32),
    "scalar_h16":    (37, 5, 7, 1, 9, 3, BF),
    "scalar_f32":    (37, 3, 4, 1, 5, 2, F32),
    "misaligned":    (37, 8, 8, 0, 24, 4, BF),
    "chunks_stride": (300000, 8, 8, 0, 8, 0, F32),
    "scalar_stride": (105000, 5, 5, 0, 5, 0, BF),
}


COPY_FORMS = [(t, h) for t, c in COPIES.items() for h in ((BF, F16) if c[6] == BF else (None,))]


@pytest.mark.parametrize("tag,h16", COPY_FORMS, ids=[t + (f"-{_name(h)}" if h else "") for t, h in COPY_FORMS])
def test_copy_channels_is_bit_exact(tag, h16):
    Fn, L = _imp()
    P, Cc, xps, xco, yps, yco, dt = COPIES[tag]
    if h16 is not None:
        _library(h16)
        dt = h16
    x = G.grid16(f"copy.{tag}", (P, xps)).to(dt)
    want = torch.full((P, yps), 7.0, dtype=dt)
    want[:, yco:yco + Cc] = x[:, xco:xco + Cc]
    xd, yd = x.to(DEV), torch.full((P, yps), 7.0, dtype=dt, device=DEV)
    L.call("hesic_copy_channels", L.ptr(xd), L.ptr(yd), P, Cc, xps, xco, yps, yco, L.dt(dt), L.stream())
    _assert_exact([_exact(f"copy_channels_{tag}" + (f"_{_name(h16)}" if h16 is F16 else ""), "y", yd, want)])


CAST_FORMS = [("f32_to_h16", BF), ("f32_to_h16", F16), ("h16_to_f32", BF), ("h16_to_f32", F16), ("f32_to_f32", None)]
# signed zeros; bf16 ties (1 + 2^-8 to even, -(1 + 3 * 2^-8) to odd + 1); IEEE half ties (1 + 2^-11, -(1 + 3 * 2^-11)); IEEE half's subnormal
# step 2^-24: half of it (a tie, to 0), 1.5 steps (a tie, to 2 steps), -1 step, 2.25 steps, the largest subnormal + half a step
CAST_SPECIAL = [0.0, -0.0, 1.00390625, -1.01171875, 1 + 2.0 ** -11, -(1 + 3 * 2.0 ** -11),
                2.0 ** -25, 1.5 * 2.0 ** -24, -2.0 ** -24, 2.25 * 2.0 ** -24, 1023.5 * 2.0 ** -24]


@pytest.mark.parametrize("n", [1027, 600001])
@pytest.mark.parametrize("dirn,h16", CAST_FORMS, ids=[d + (f"-{_name(h)}" if h else "") for d, h in CAST_FORMS])
def test_cast_is_bit_exact(dirn, h16, n):
    Fn, L = _imp()
    if h16 is not None:
        _library(h16)
    sdt, ddt = {"f32_to_h16": (F32, h16), "h16_to_f32": (h16, F32), "f32_to_f32": (F32, F32)}[dirn]
    x = G.synthetic._uniform(f"glue.cast.{dirn}.{n}", (n,), -6, 6).to(sdt)          # arbitrary fp32: the narrowing rounds to nearest even
    x[:len(CAST_SPECIAL)] = torch.tensor(CAST_SPECIAL).to(sdt)                       # (as a 16-bit source: what those round to, subnormals included)
    xd, yd = x.to(DEV), torch.empty(n, dtype=ddt, device=DEV)
    L.call("hesic_cast", L.ptr(xd), L.dt(sdt), L.ptr(yd), L.dt(ddt), n, L.stream())
    _assert_exact([_exact(f"cast_{dirn}_{n}" + (f"_{_name(h16)}" if h16 is F16 else ""), "y", yd, x.to(ddt))])


def _round_operand(name, n):
    x = G.synthetic._uniform("glue.round." + name, (n,), -6, 6)
    k = torch.arange(-6.0, 7.0)
    special = torch.cat((k + 0.5, k - 0.5, torch.tensor([0.0, -0.0, 0.3, -0.3, 0.49999997, -0.49999997])))     # halves at even and odd k, +-0
    x[:len(special)] = special
    return x


# n % 8 != 0: the element-wise kernel; n % 8 == 0: eight values a thread; one size above 524288 work items each; fp32 -> fp32 as well
@pytest.mark.parametrize("n,ddt", [(45, BF), (1024, BF), (45, F32), (524291, BF), (8 * 524289, BF), (45, F16), (1024, F16), (524291, F16), (8 * 524289, F16)],
                         ids=lambda v: _name(v) if isinstance(v, torch.dtype) else str(v))
def test_round_half_even_is_bit_exact(n, ddt):
    Fn, L = _imp()
    if ddt == F16:
        _library(F16)
    x = _round_operand(f"{n}.{_name(BF if ddt == F16 else ddt)}", n)                 # the same operand for both 16-bit libraries
    y = Fn.round_to(x.to(DEV), ddt)
    assert y.dtype == ddt
    _assert_exact([_exact(f"round_{n}_{_name(ddt)}", "y", y, torch.round(x).to(ddt))])


@pytest.mark.parametrize("n", [1027, 524291])
@pytest.mark.parametrize("dt", [F32, BF], ids=_name)
@pytest.mark.parametrize("act", [1, 2], ids=["relu", "leaky"])
def test_act_backward_is_bit_exact(act, dt, n):
    """dx = dy * act'(y) stored in y's type; y holds +0, -0, the smallest positive subnormal and normal values of its type and their negatives."""
    Fn, L = _imp()
    y = G.grid16(f"actb.y.{n}", (n,)).to(dt)
    tiny = torch.finfo(dt).tiny
    sub = torch.tensor([1], dtype=torch.int32).view(F32) if dt == F32 else torch.tensor([1], dtype=torch.int16).view(BF)
    y[:6] = torch.cat((torch.tensor([0.0, -0.0, tiny, -tiny], dtype=dt), sub, -sub))
    dy = G.synthetic._uniform(f"glue.actb.g.{n}", (n,), -2, 2).to(dt)
    pos = y.float() > 0
    assert bool(pos[2]) and bool(pos[4]) and not bool(pos[0]) and not bool(pos[1])
    low = torch.zeros(n) if act == 1 else G.LEAK * dy.float()
    want = torch.where(pos, dy.float(), low).to(dt)
    yd, gd = y.to(DEV), dy.to(DEV)
    dx = torch.empty_like(yd)
    L.call("hesic_act_backward", L.ptr(yd), L.ptr(gd), L.ptr(dx), n, act, L.dt(dt), L.stream())
    _assert_exact([_exact(f"act_backward_{'relu' if act == 1 else 'leaky'}_{_name(dt)}_{n}", "dx", dx, want)])


# ----------------------------------------------------------------------------------------------------------------- spatial max
def _spatial_device(x, dt):
    """x (B, C, HW) as the (B, C, 1, HW) channels-last map the path pools."""
    B, Cc, HW = x.shape
    return x.permute(0, 2, 1).contiguous().to(DEV, dt).reshape(B, 1, HW, Cc).permute(0, 3, 1, 2)


@pytest.mark.parametrize("leaky", [False, True], ids=["plain", "leaky"])
@pytest.mark.parametrize("dt", [F32, BF], ids=_name)
@pytest.mark.parametrize("tag", [t for t, c in G.SPATIAL.items() if c[3]])
def test_spatial_max_with_argmax_and_backward(tag, dt, leaky):
    """Values and arg-max exact (ties to the lowest pixel index, -0.0 == +0.0), and the backward's dx bit for bit."""
    Fn, L = _imp()
    B, Cc, HW, _ = G.SPATIAL[tag]
    x, g = G.spatial_operands(tag)
    val, arg = G.spatial_max_ref(x, leaky)
    xd = _spatial_device(x, dt)
    assert xd.is_contiguous(memory_format=CL)
    out = torch.empty((B, Cc), dtype=F32, device=DEV)
    am = torch.full((B, Cc), -1, dtype=torch.int32, device=DEV)
    L.call("hesic_spatial_max", L.ptr(xd), L.ptr(out), L.ptr(am), B, HW, Cc, L.dt(dt), int(leaky), L.stream())
    case = f"spatial_max_{tag}_{_name(dt)}_{'leaky' if leaky else 'plain'}"
    res = [_exact(case, "out", out, val, bits=False), _exact(case, "argmax", am.long(), arg, bits=False)]
    xg = xd.detach().requires_grad_()
    o2 = Fn.spatial_max(xg, leaky=leaky)
    o2.backward(g.to(DEV).reshape(B, Cc, 1, 1))
    res.append(_exact(case, "out_autograd", o2.detach().reshape(B, Cc), val, bits=False))
    want = G.spatial_max_backward_ref(g, val, arg, HW, leaky, dt)
    res.append(_exact(case, "dx", xg.grad.permute(0, 2, 3, 1).reshape(B, HW, Cc), want))
    _assert_exact(res)


@pytest.mark.parametrize("leaky", [False, True], ids=["plain", "leaky"])
@pytest.mark.parametrize("dt", [F32, BF, F16], ids=_name)
@pytest.mark.parametrize("tag", [t for t, c in G.SPATIAL.items() if not c[3]])
def test_spatial_max_without_argmax(tag, dt, leaky):
    """The inference route: HW >= 256 splits the pixels over blocks and merges the partial maxima through an integer atomic; HW = 255 stays
    on the one-block form.  A channel that is -0.0 at every pixel must come out as 0, not as the -inf the accumulator is filled with."""
    Fn, L = _imp()
    if dt == F16:
        _library(F16)
    B, Cc, HW, _ = G.SPATIAL[tag]
    x, _ = G.spatial_operands(tag)
    val, _ = G.spatial_max_ref(x, leaky)
    with torch.no_grad():
        out = Fn.spatial_max(_spatial_device(x, dt), leaky=leaky)
    case = f"spatial_max_{tag}_{_name(dt)}_{'leaky' if leaky else 'plain'}"
    res = [_exact(case, "out", out.reshape(B, Cc), val, bits=False)]
    print(f"glue_parity {case} signed_zero_channel {float(out.reshape(B, Cc)[:, 2].abs().max()):.4f}")
    _assert_exact(res)
    assert bool((out.reshape(B, Cc)[:, 2] == 0).all())


# ------------------------------------------------------------------------------------------------ pooled linear, softmax over K
MIX = {"3x960": (5, 192), "9x100": (5, 20), "8x5": (5, 1), "17x33": (3, 11)}


@pytest.mark.parametrize("tag", list(G.POOLED))
def test_pooled_linear_forward_backward_and_mix_weights(tag):
    Fn, L = _imp()
    B, N = G.POOLED[tag]
    R = G.pooled_reference(tag)
    p = R["p"].to(DEV).reshape(B, N, 1, 1).requires_grad_()
    w = R["w"].to(DEV).reshape(N, N, 1, 1).requires_grad_()
    b = R["b"].to(DEV).requires_grad_()
    y = Fn.pooled_linear(p, w, b)
    y.backward(R["g"].to(DEV).reshape(B, N, 1, 1))
    case = f"pooled_linear_{tag}"
    res = [_bar(case, "y", R["y"], y, c=G.C_BAR), _bar(case, "dp", R["dp"], p.grad, c=G.C_BAR), _bar(case, "dw", R["dw"], w.grad, c=G.C_BAR),
           _bar(case, "db", R["db"], b.grad, c=G.C_BAR)]
    K, M = MIX[tag]
    with torch.no_grad():
        mw = Fn.mix_weights(p.detach(), w.detach(), b.detach(), K, M)
    Rm = G.softmax_ref(R["y"]["ref"], K, M, logit_unit=R["y"]["unit"])           # c = C_BAR below allows the logits their own bar, C_BAR units, once
    res.append(_bar(f"mix_weights_{tag}", "weights", Rm, mw, c=G.C_BAR))
    _assert_bars(res)
    assert bool(torch.isfinite(mw).all())


@pytest.mark.parametrize("tag", list(G.SOFTMAX))
def test_softmax_k_forward_and_backward(tag):
    """One column of equal logits (exactly 1/K up to the bar) and one with a spread of 80: no overflow, no NaN, the small weights ~1e-35."""
    Fn, L = _imp()
    K, M = G.SOFTMAX[tag]
    l = G.softmax_logits(tag)
    B = l.shape[0]
    ld = l.to(DEV).reshape(B, K * M, 1, 1).requires_grad_()
    w = Fn.softmax_k(ld, K, M)
    g = G.grid16(f"sm.{tag}.g", (B, K * M))
    w.backward(g.to(DEV).reshape(B, K * M, 1, 1))
    wc = w.detach().reshape(B, K * M).cpu()
    case = f"softmax_k_{tag}"
    res = [_bar(case, "weights", G.softmax_ref(l, K, M), wc, c=G.C_BAR),
           _bar(case, "dlogits", G.softmax_backward_ref(wc, g, K, M), ld.grad, c=G.C_BAR)]
    _assert_bars(res)
    w3 = wc.reshape(B, K, M)
    assert bool(torch.isfinite(wc).all()) and bool(torch.isfinite(ld.grad).all())
    assert float(w3[:, 0, 1].max()) < 1e-34 and float(w3[:, -1, 1].min()) > 0.99


# ------------------------------------------------------------------------------------------------------------------ reductions
@pytest.mark.parametrize("tag", list(G.SUM_LOG2))
def test_sum_log2(tag):
    """n = 1, 3: the scalar tail alone; 1027: 16-byte lanes + a tail of 3; a pointer off by one element: no 16-byte lanes at all; 300000:
    more lanes of work than 128 blocks hold."""
    Fn, L = _imp()
    n, off = G.SUM_LOG2[tag]
    lik = G.likelihoods(tag)
    ld = lik.to(DEV)
    out = torch.zeros(1, dtype=torch.float64, device=DEV)
    addr = ld.data_ptr() + 4 * off
    assert (addr % 16 != 0) == bool(off)
    L.call("hesic_sum_log2", C.c_void_p(addr), n, L.ptr(out), L.stream())
    _assert_bars([_bar(f"sum_log2_{tag}", "sum", G.sum_log2_ref(lik[off:]), out)])


def _sq_views(tag, form, h16=BF):
    """(a, b) on the device: ``form`` picks the layouts / storage types the pair arrives in."""
    a, b = G.sq_diff_operands(tag)
    ad, bd = a.to(DEV), b.to(DEV)
    if form == "nchw_nhwc":
        bd = bd.contiguous(memory_format=CL)
    elif form == "f32_h16":
        bd = bd.to(h16).contiguous(memory_format=CL)
    elif form == "h16_f32":
        ad = ad.to(h16)
    elif form == "view":                       # a: a window of a wider, taller buffer (row stride W + 3)
        B, Cc, H, W = a.shape
        buf = torch.full((B, Cc, H + 2, W + 3), 9.0, device=DEV)
        buf[:, :, 1:H + 1, 2:W + 2] = ad
        ad = buf[:, :, 1:H + 1, 2:W + 2]
        assert not ad.is_contiguous()
    return ad, bd


SQ_FORMS = [(t, f) for t in G.SQ_DIFF for f in (("dense", "nchw_nhwc") if t == "big" else ("dense", "nchw_nhwc", "f32_h16", "h16_f32", "view"))]


SQ_SUM_FORMS = [(t, f, h) for t, f in SQ_FORMS for h in ((BF, F16) if "h16" in f else (None,))]


@pytest.mark.parametrize("tag,form,h16", SQ_SUM_FORMS, ids=[f"{t}-{f}" + (f"-{_name(h)}" if h else "") for t, f, h in SQ_SUM_FORMS])
def test_sum_sq_diff(tag, form, h16):
    Fn, L = _imp()
    if h16 is not None:
        _library(h16)
    a, b = G.sq_diff_operands(tag)
    ad, bd = _sq_views(tag, form, h16 or BF)
    out = Fn.sum_sq_diff(ad, bd)
    _assert_bars([_bar(f"sum_sq_diff_{tag}_{form}" + (f"_{_name(h16)}" if h16 is F16 else ""), "sum", G.sum_sq_diff_ref(a, b), out)])


@pytest.mark.parametrize("tag,form", SQ_FORMS, ids=[f"{t}-{f}" for t, f in SQ_FORMS])
def test_sq_diff_backward(tag, form):
    """g = scale * (a - b) as a dense NCHW fp32 map: the 16-byte fast path (both operands dense fp32, n % 4 == 0) and the strided path."""
    Fn, L = _imp()
    a, b = G.sq_diff_operands(tag)
    B, Cc, H, W = a.shape
    ad, bd = _sq_views(tag, form)
    scale = float(torch.tensor(0.37, dtype=F32))
    g = torch.full((B, Cc, H, W), 7.0, device=DEV)
    sa, sb = (C.c_int64 * 4)(*ad.stride()), (C.c_int64 * 4)(*bd.stride())
    L.call("hesic_sq_diff_backward", L.ptr(ad), L.dt(ad), sa, L.ptr(bd), L.dt(bd), sb, B, Cc, H, W, scale, L.ptr(g), L.stream())
    fast = form == "dense" and (B * Cc * H * W) % 4 == 0
    assert fast == (tag in ("50x100", "2x2", "big") and form == "dense")
    ref = G.elementwise_ref(scale * (a.double() - b.double()))          # a - b is exact on the grid: one rounding
    _assert_bars([_bar(f"sq_diff_backward_{tag}_{form}", "g", ref, g)])


@pytest.mark.parametrize("n", [1027, 600001])
def test_log_backward(n):
    Fn, L = _imp()
    lik = G.likelihoods("n300000")[:n] if n <= 300000 else torch.cat((G.likelihoods("n300000"), G.likelihoods("n300000") * 0.5 + 0.25, G.likelihoods("n1")))
    assert lik.numel() == n
    scale = float(torch.tensor(-0.37, dtype=F32))
    ld = lik.to(DEV)
    g = torch.empty_like(ld)
    L.call("hesic_log_backward", L.ptr(ld), scale, L.ptr(g), n, L.stream())
    _assert_bars([_bar(f"log_backward_{n}", "g", G.elementwise_ref(scale / lik.double(), roundings=2), g)])      # a division within one ulp


def _rd_jobs(n_lik, n_sq):
    """Likelihood maps of at most two blocks each (two fp64 partials add to the same bits in either order; three need not) and image pairs
    on the 1/16 grid (every fp64 partial sum is exact)."""
    sizes = [1027, 3, 1, 700, 64, 2044, 513, 250][:n_lik]
    liks = [G.likelihoods("n300000")[1000 * i:1000 * i + n].clone().to(DEV) for i, n in enumerate(sizes)]
    pairs = []
    for tag, form in (("50x100", "f32_h16"), ("c19", "nchw_nhwc"))[:n_sq]:
        pairs.append(_sq_views(tag, form))
    return liks, pairs


@pytest.mark.parametrize("n_lik,n_sq", [(1, 0), (0, 1), (8, 2)])
def test_rd_sums_match_the_single_job_entry_points_bit_for_bit(n_lik, n_sq):
    Fn, L = _imp()
    liks, pairs = _rd_jobs(n_lik, n_sq)
    z = lambda: torch.zeros(1, dtype=torch.float64, device=DEV)
    lo, so = [z() for _ in liks], [z() for _ in pairs]
    Fn.rd_sums(liks, lo, pairs, so)
    res = []
    for i, l in enumerate(liks):
        res.append(_exact(f"rd_sums_{n_lik}_{n_sq}", f"lik{i}", lo[i], Fn.sum_log2(l)))
    for i, (a, b) in enumerate(pairs):
        res.append(_exact(f"rd_sums_{n_lik}_{n_sq}", f"sq{i}", so[i], Fn.sum_sq_diff(a, b)))
    _assert_exact(res)
    for i, l in enumerate(liks):
        _assert_bars([_bar(f"rd_sums_{n_lik}_{n_sq}", f"lik{i}_value", G.sum_log2_ref(l.cpu()), lo[i])])


def test_rd_sums_with_a_capped_likelihood_job():
    """A likelihood map of 300000 values wants 293 blocks and gets the cap of 128: the jobs behind it start at block 129.  Its fp64 partials may
    add in any order, so it is held by the sum_log2 bar; the small jobs around it and the image pair stay bit-identical to the single-job entry
    points, which they can only be if start[] / nb place every block of the capped job and of its neighbours."""
    Fn, L = _imp()
    big = G.likelihoods("n300000")
    assert big.numel() // 4 + 1 > 128 * 256
    liks = [G.likelihoods("n1027").to(DEV), big.to(DEV), G.likelihoods("n3").to(DEV)]
    pairs = [_sq_views("50x100", "nchw_nhwc")]
    z = lambda: torch.zeros(1, dtype=torch.float64, device=DEV)
    lo, so = [z() for _ in liks], [z() for _ in pairs]
    Fn.rd_sums(liks, lo, pairs, so)
    res = [_exact("rd_sums_capped", "lik0", lo[0], Fn.sum_log2(liks[0])), _exact("rd_sums_capped", "lik2", lo[2], Fn.sum_log2(liks[2])),
           _exact("rd_sums_capped", "sq0", so[0], Fn.sum_sq_diff(*pairs[0]))]
    bars = [_bar("rd_sums_capped", f"lik{i}_value", G.sum_log2_ref(l.cpu()), lo[i]) for i, l in enumerate(liks)]
    _assert_exact(res)
    _assert_bars(bars)

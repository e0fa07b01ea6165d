"""Per-element fp64 parity of the 16-bit conv gradient kernels (csrc/wgrad.hip, conv_igemm.hip, sconv.hip) on a real MI355X.

Every case runs the bf16 library through ``Fn.conv2d`` under autograd (or the C ABI where a route needs it) and checks y, dx, dw and db
element by element against the fp64 reference and bar of tests/conv_grad_ref.py:  |err_e| <= 8 sqrt(n) 2^-24 S_e  (+ 2^-8 |ref_e| for a
bf16-stored output), exactly 0 where S_e == 0.  tests/test_conv_grad_ref_cpu.py shows on the CPU that this bar fails a gradient with one
dropped pixel, channel, ragged K tail or leaking dead tap.  Each case prints  max_e |err_e| / (sqrt(n) 2^-24 S_e)  per output
("conv_grad_parity <case> <output> <ratio>"); the values measured when the tests were written are in profiles/conv_grad_parity.json.
Nothing is asserted about which kernel ran beyond the public size queries."""
import ctypes as C

import pytest
import torch

import conv_grad_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF = torch.bfloat16
CL = torch.channels_last


def _bf16_library(fn):
    import functools

    @functools.wraps(fn)
    def run(*a, **kw):
        import hesic_amd
        hesic_amd.set_compute_dtype(BF)
        try:
            return fn(*a, **kw)
        finally:
            hesic_amd.set_compute_dtype(torch.float32)
    return run


def _assert_all(tag, ref, got):
    """Every output of ``got`` against its bars; the ratios are printed before anything is asserted."""
    res = {q: R.check(ref, q, t) for q, t in got.items() if t is not None}
    for q, (ok, ratio, msg) in res.items():
        print(f"conv_grad_parity {tag} {q} {ratio:.4f}")
    for q, (ok, ratio, msg) in res.items():
        assert ok, f"{tag} {msg}"
        assert ratio <= R.C_BAR, f"{tag} {q}: ratio {ratio:.3f}"


def _device_operands(tag, salt=0):
    """The case's operands as the 16-bit path takes them: wide maps bf16 NHWC, 3- / 6-channel images fp32 (planar unless the case says
    NHWC), weights and bias fp32."""
    Cin, Cout, k, s, p, tr, _, opt = R.CASES[tag]
    o = R.operands(tag, salt)
    x = o["x"].to(DEV, BF).contiguous(memory_format=CL) if Cin > 8 else o["x"].to(DEV)
    if opt.get("x_nhwc"):
        x = x.contiguous(memory_format=CL)
    gy = o["gy"].to(DEV, BF) if Cout > 8 else o["gy"].to(DEV)
    return x, o["w"].to(DEV), (None if o["b"] is None else o["b"].to(DEV)), gy, (None if o["mask"] is None else o["mask"].to(DEV))


def _conv_fwd_bwd(tag):
    from hesic_amd import functional as Fn
    Cin, Cout, k, s, p, tr, _, opt = R.CASES[tag]
    x, w, b, gy, mask = _device_operands(tag)
    x.requires_grad_(), w.requires_grad_()
    if b is not None:
        b.requires_grad_()
    y = Fn.conv2d(x, w, b, kernel_size=k, stride=s, padding=p, transposed=bool(tr), act=opt.get("act", 0), in_abs=opt.get("in_abs", False),
                  tap_mask=opt.get("tap_mask", 0), mask=mask)
    y16, dx16 = R.storage(tag)
    assert y.dtype == (BF if y16 else torch.float32) and tuple(y.shape) == tuple(gy.shape)
    y.backward(gy)
    torch.cuda.synchronize()
    assert x.grad.dtype == (BF if dx16 else torch.float32) and w.grad.dtype == torch.float32
    # an activation's backward reads act'(y) off the y it saved: the reference takes the same y (conv_grad_ref.py)
    ref = R.reference_of(tag, y_saved=y.detach().float().cpu()) if opt.get("act") else R.cached_reference(tag)
    _assert_all(tag, ref, {"y": y, "dx": x.grad, "dw": w.grad, "db": None if b is None else b.grad})


@pytest.mark.parametrize("tag", list(R.WIDE))
@_bf16_library
def test_wide_conv_gradients(tag):
    _conv_fwd_bwd(tag)


@pytest.mark.parametrize("tag", list(R.IMAGE))
@_bf16_library
def test_image_side_conv_gradients(tag):
    _conv_fwd_bwd(tag)


def _wgrad_desc(tag, dtype=None):
    from hesic_amd import _lib as L
    Cin, Cout, k, s, p, tr, (B, H, W), opt = R.case(tag)
    Ho, Wo = R.out_hw(H, W, k, s, p, tr, opt.get("out_pad"))
    return L.ConvDesc(B, H, W, Cin, Ho, Wo, Cout, k, k, s, p, int(tr), L.BF16 if dtype is None else dtype, 0, int(opt.get("in_abs", False)), Cin, 0, Cout, 0,
                      opt.get("tap_mask", 0))


@_bf16_library
def test_the_table_has_a_ragged_split_k_case_and_a_single_slice_case():
    from hesic_amd import _lib as L
    Cin, Cout, k, s, p, tr, (B, H, W), _ = R.CASES["c5s2_ragged_k"]
    assert (Cin, Cout, k, s, tr) == (128, 128, 5, 2, 0)
    d = _wgrad_desc("c5s2_ragged_k")
    nsplit = int(L.lib().hesic_conv2d_wgrad_nsplit(C.byref(d), 0))
    Q = B * d.Ho * d.Wo
    assert nsplit >= 2 and Q % nsplit != 0, (nsplit, Q)
    d1 = _wgrad_desc("c5s2_tiny")
    assert int(L.lib().hesic_conv2d_wgrad_nsplit(C.byref(d1), 0)) == 1


@pytest.mark.parametrize("deferred", [False, True], ids=["direct", "deferred"])
@_bf16_library
def test_twice_used_weight_adds_into_its_gradient_slots(deferred):
    """One weight, two convs, gradient slots registered: both weight gradients and both bias gradients add into the slots (the finishing pass
    accumulates); the reference is the sum of the two gradients, the bar that of the combined sum.  "deferred" is the Trainer's form: the
    split-K launches and finishing passes are queued and issued by the batched calls (with their own K-slice count)."""
    from hesic_amd import functional as Fn
    tag = "c5s2_128"
    Cin, Cout, k, s, p, tr, _, opt = R.CASES[tag]
    o0, o1 = R.operands(tag, 0), R.operands(tag, 1)
    _, w, b, _, _ = _device_operands(tag)
    w.requires_grad_(), b.requires_grad_()
    sw, sb = Fn.GradSlot(torch.zeros_like(w), "w"), Fn.GradSlot(torch.zeros_like(b), "b")
    keys = Fn.register_grad_slots([(w, sw), (b, sb)])
    prev = Fn.grad_slots_active(True)
    defer = Fn.defer_wgrad_finish(deferred)
    try:
        for o in (o0, o1):
            x = o["x"].to(DEV, BF).contiguous(memory_format=CL)
            Fn.conv2d(x, w, b, kernel_size=k, stride=s, padding=p).backward(o["gy"].to(DEV, BF))
    finally:
        Fn.defer_wgrad_finish(defer)          # flushes what is queued
        Fn.grad_slots_active(prev)
        Fn.clear_grad_slots(keys)
    torch.cuda.synchronize()
    assert w.grad is None and b.grad is None and sw.writes == 2 and sb.writes == 2
    refs = [R.reference(o["x"], o0["w"], o0["b"], o["gy"], stride=s, pad=p) for o in (o0, o1)]
    _assert_all("slots_c5s2_128_twice_" + ("deferred" if deferred else "direct"), R.combine(*refs), {"dw": sw.grad, "db": sb.grad})


@_bf16_library
def test_direct_wgrad_of_a_k4_transposed_conv_sums_the_bias_in_column_blocks():
    """k = 4, pad 0, stride 2 transposed: the output is larger than H * stride, so no tap set of the GEMM covers dY once and the bias gradient
    comes from the separate column-sum blocks of the finishing pass.  The call overwrites dw / db."""
    from hesic_amd import _lib as L
    tag = "d4s2_colsum"
    Cin, Cout, k, s, p, tr, _, _ = R.CASES[tag]
    x, _, _, gy, _ = _device_operands(tag)
    gy = gy.contiguous(memory_format=CL)
    d = _wgrad_desc(tag)
    assert d.Ho > d.H * s
    nws = int(L.lib().hesic_conv2d_wgrad_ws_bytes(C.byref(d)))
    ws = torch.empty(max(nws, 16), dtype=torch.uint8, device=DEV)
    dw = torch.full((Cin, Cout, k, k), 7.0, device=DEV)
    db = torch.full((Cout,), 7.0, device=DEV)
    L.call("hesic_conv2d_wgrad_direct", C.byref(d), L.ptr(x), L.ptr(gy), L.ptr(dw), L.ptr(db), 0, L.ptr(ws), nws, L.stream())
    torch.cuda.synchronize()
    _assert_all(tag, R.cached_reference(tag), {"dw": dw, "db": db})


@_bf16_library
def test_direct_narrow_wgrad_without_a_workspace():
    """hesic_sconv2d_wgrad with ws = NULL: g_a_conv1's weight gradient by the register-accumulating kernel (one atomic per weight and block),
    partial 8 x 16 tiles on both edges."""
    from hesic_amd import _lib as L
    tag = "conv1_nw_kernel"
    Cin, Cout, k, s, p, tr, (B, H, W), _ = R.CASES[tag]
    x, _, _, gy, _ = _device_operands(tag)
    gy = gy.contiguous(memory_format=CL)
    xs, ys = x.stride(), gy.stride()
    d = L.SConvDesc(B, H, W, Cin, H // 2, W // 2, Cout, k, k, s, p, 0, L.F32, L.BF16, 0, 0, xs[0], xs[1], xs[2], xs[3], ys[0], ys[1], ys[2], ys[3])
    assert int(L.lib().hesic_sconv2d_wgrad_ws_bytes(C.byref(d))) > 0          # the MFMA route exists for this shape: no workspace, no MFMA route
    dw = torch.full((Cout, Cin, k, k), 7.0, device=DEV)
    db = torch.full((Cout,), 7.0, device=DEV)
    L.call("hesic_sconv2d_wgrad", C.byref(d), L.ptr(x), L.ptr(gy), L.ptr(dw), L.ptr(db), None, 0, L.stream())
    torch.cuda.synchronize()
    _assert_all(tag, R.cached_reference(tag), {"dw": dw, "db": db})


def _packed_wgrad(tag, f32, with_bias):
    """hesic_conv2d_wgrad + hesic_unpack_conv_wgrad of a PACKED case: (dw in the PyTorch layout, db or None).  Every buffer the calls have to
    write starts out as 7 (the workspace as NaN)."""
    from hesic_amd import _lib as L
    Cin, Cout, k, s, p, tr, _, _ = R.case(tag)
    o = R.operands(tag)
    dt = torch.float32 if f32 else BF
    x, gy = (o[q].to(DEV, dt).contiguous(memory_format=CL) for q in ("x", "gy"))
    d = _wgrad_desc(tag, L.F32 if f32 else L.BF16)
    nws = int(L.lib().hesic_conv2d_wgrad_ws_bytes(C.byref(d)))
    ws = torch.full((max(nws, 16) // 4,), float("nan"), device=DEV)
    dwp = torch.full((k * k, Cout, Cin), 7.0, device=DEV)
    dw = torch.full((Cout, Cin, k, k), 7.0, device=DEV)
    db = torch.full((Cout,), 7.0, device=DEV) if with_bias else None
    L.call("hesic_conv2d_wgrad", C.byref(d), L.ptr(x), L.ptr(gy), L.ptr(dwp), None if db is None else L.ptr(db), L.ptr(ws), nws, L.stream())
    L.call("hesic_unpack_conv_wgrad", L.ptr(dwp), None, L.ptr(dw), Cout, Cin, k, k, int(tr), L.stream())
    torch.cuda.synchronize()
    return dw, db


@pytest.mark.parametrize("with_bias", [True, False], ids=["bias", "nobias"])
@pytest.mark.parametrize("f32", [False, True], ids=["bf16", "fp32"])
@pytest.mark.parametrize("tag", list(R.PACKED))
@_bf16_library
def test_packed_layout_wgrad(tag, f32, with_bias):
    """The packed-layout entry point, which no Python wrapper calls: its K-slice reduce (plain for few slices, slice-parallel for the one-tap
    layer with >= 32 slices, fused with the bias column sums when dbias is given) and the zero fill of a masked conv's dead taps."""
    from hesic_amd import _lib as L
    Cin, Cout, k, _, _, _, _, opt = R.case(tag)
    d = _wgrad_desc(tag, L.F32 if f32 else L.BF16)
    nsplit = int(L.lib().hesic_conv2d_wgrad_nsplit(C.byref(d), 0))
    taps = bin(opt["tap_mask"]).count("1") if "tap_mask" in opt else k * k
    wide_reduce = nsplit >= 32 and taps * Cout * Cin < 262144
    assert wide_reduce == (tag == "packed_c1_wide"), (nsplit, taps)
    dw, db = _packed_wgrad(tag, f32, with_bias)
    _assert_all(f"{tag}_{'fp32' if f32 else 'bf16'}_{'bias' if with_bias else 'nobias'}", R.cached_reference(tag), {"dw": dw, "db": db})

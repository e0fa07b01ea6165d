"""Stride-1 5 x 5 convs on 128 input channels (the 128 -> 960 output convs of the entropy-parameter nets, ywz/mywork/newnet1.py) with the
input patch resident in LDS (igemm_s1p_kernel, csrc/conv_igemm.hip) against the per-stage x-tile form (igemm_glds_kernel) and torch's conv.

Every case runs the same call with HESIC_IGEMM_S1_PATCH=0 (never) and =2 (whenever the shape is eligible).  The two kernels walk the taps,
channel chunks and k-substeps of an output value in the same order, so the bar between them is bit for bit; the oracle bar is the one of
test_gpu_phase_fusion.py (1.5e-2 of the output scale on 16-bit-rounded operands).  The calls run inside ``Fn.no_split_k()``: a split-K
launch (which small maps would otherwise get, in both modes) is not eligible, and the comparison would be vacuous.  Shapes are the smallest
at which the kernel can go wrong: one 16 x 16 tile whose whole patch border is padding, tiles that hang over rows and columns, a map smaller
than the tile, a ragged last cout tile with real neighbours in the patch border, groups / two activations / fp32-only output, a channel
slice of a wider input, a batch offset; and the workload's own launch (8 x 32 x 32, 2 x (128 -> 960) grouped, fp32-only), repeated."""
import ctypes as C
import os

import pytest
import torch
import torch.nn.functional as F

import hesic_amd
import memguard as MG
from hesic_amd import synthetic

pytestmark = pytest.mark.gpu
DEV = "cuda"
CL = torch.channels_last
ENV = "HESIC_IGEMM_S1_PATCH"
FMTS = {"bf16": torch.bfloat16, "f16": torch.float16}


def _imp():
    from hesic_amd import functional as Fn
    from hesic_amd import _lib as L
    return Fn, L


def rnd(name, shape, lo=-1.0, hi=1.0):
    return synthetic._uniform("s1p." + name, shape, lo, hi)


def rel_err(a, b):
    a, b = a.detach().float().cpu(), b.detach().float().cpu()
    return float((a - b).abs().max() / (b.abs().max() + 1e-12))


class _mode:
    """HESIC_IGEMM_S1_PATCH for the block (the library reads it on every call); the previous value comes back on exit."""

    def __init__(self, m):
        self.m = str(m)

    def __enter__(self):
        self.prev = os.environ.get(ENV)
        os.environ[ENV] = self.m

    def __exit__(self, *exc):
        if self.prev is None:
            os.environ.pop(ENV, None)
        else:
            os.environ[ENV] = self.prev


@pytest.fixture(params=list(FMTS))
def fmt(request):
    dt = FMTS[request.param]
    hesic_amd.set_compute_dtype(dt)
    try:
        yield dt
    finally:
        hesic_amd.set_compute_dtype(torch.float32)


def _variant(L, B, H, W, Cin, Cout, x_ps=None, x_co=0):
    d = L.ConvDesc(B, H, W, Cin, H, W, Cout, 5, 5, 1, 2, 0, L.H16, 0, 0, x_ps or Cin, x_co, Cout, 0, 0)
    v = (C.c_int32 * 4)()
    L.call("hesic_conv2d_variant", C.byref(d), v)
    return list(v)


def _both_modes(L, fn, vargs):
    """fn() under mode 0 and mode 2, with the check that only mode 2 selects the resident-patch kernel for the launch's descriptor."""
    Fn, _ = _imp()
    outs = []
    for m in (0, 2):
        with _mode(m), Fn.no_split_k(), torch.no_grad():
            v = _variant(L, *vargs)
            assert (v == [256, 128, 64, 1]) == (m == 2), (m, v)
            outs.append(fn())
    torch.cuda.synchronize()
    return outs


def _act_ref(y, act):
    return {"none": lambda t: t, "relu": torch.relu, "leaky": lambda t: F.leaky_relu(t, 0.01)}[act](y)


def _acts(L):
    return {"none": L.ACT_NONE, "relu": L.ACT_RELU, "leaky": L.ACT_LEAKY}


PLAIN_CASES = [
    # tag, Cout, (B, H, W), act, bias
    ("one_tile_all_borders", 128, (1, 16, 16), "none", True),
    ("ragged_tiles_batch", 128, (2, 24, 40), "relu", True),
    ("tiny_map", 128, (1, 5, 7), "leaky", True),
    ("ragged_cout_none", 960, (1, 32, 32), "none", True),
    ("ragged_cout_relu", 960, (1, 32, 32), "relu", True),
    ("ragged_cout_leaky", 960, (1, 32, 32), "leaky", True),
    ("ragged_cout_no_bias", 960, (1, 32, 32), "none", False),
]


def _plain_inputs(tag, Cout, bhw, dt, bias=True):
    B, H, W = bhw
    w = (rnd(tag + "_w", (Cout, 128, 5, 5)) * 0.03).to(dt).float()
    b = rnd(tag + "_b", (Cout,), -0.2, 0.2) if bias else None
    x = rnd(tag + "_x", (B, 128, H, W), -2, 2).to(dt).float()
    return x, w, b


@pytest.mark.parametrize("tag,Cout,bhw,act,bias", PLAIN_CASES, ids=[c[0] for c in PLAIN_CASES])
def test_resident_patch_equals_the_staged_form_bit_for_bit(tag, Cout, bhw, act, bias, fmt):
    Fn, L = _imp()
    B, H, W = bhw
    x, w, b = _plain_inputs(tag, Cout, bhw, fmt, bias)
    xd, wd, bd = x.to(DEV, fmt).contiguous(memory_format=CL), w.to(DEV), (b.to(DEV) if bias else None)
    staged, patch = _both_modes(L, lambda: Fn.conv2d(xd, wd, bd, kernel_size=5, stride=1, padding=2, act=_acts(L)[act]), (B, H, W, 128, Cout))
    assert patch.shape == (B, Cout, H, W) and torch.equal(patch, staged)
    assert rel_err(patch, _act_ref(F.conv2d(x, w, b, 1, 2), act)) < 1.5e-2


def _grouped_inputs(dt, B, H, W, branches):
    x = rnd("g_x", (B, 256, H, W), -2, 2).to(dt).float()
    ws = [(rnd(f"g_w{i}", (960, 128, 5, 5)) * 0.03).to(dt).float() for i in range(branches)]
    bs = [rnd(f"g_b{i}", (960,), -0.2, 0.2) for i in range(branches)]
    return x, ws, bs


def _grouped_ref(x, ws, bs, acts, shared):
    outs = []
    for i, (w, b, a) in enumerate(zip(ws, bs, acts)):
        xi = x[:, :128] if shared else x[:, 128 * i:128 * (i + 1)]
        outs.append(_act_ref(F.conv2d(xi, w, b, 1, 2), a))
    return outs


@pytest.mark.parametrize("form", ["f32_only", "h16", "shared_three"])
def test_grouped_launches(form, fmt):
    """Two groups of 128 -> 960 on their own halves of a 256-channel input (relu | none; fp32-only or 16-bit output), and three branches on a
    shared 128-channel slice of it: groups, act_split / act2, x_pix_stride > Cin, the 960 -> 1024 pad rows."""
    Fn, L = _imp()
    B, H, W = 1, 16, 16
    shared = form == "shared_three"
    n = 3 if shared else 2
    acts = ["relu", "none", "none"][:n]
    x, ws, bs = _grouped_inputs(fmt, B, H, W, n)
    xd, wd, bd = x.to(DEV, fmt).contiguous(memory_format=CL), [w.to(DEV) for w in ws], [b.to(DEV) for b in bs]
    kw = dict(kernel_size=5, stride=1, padding=2, shared_input=shared, acts=[_acts(L)[a] for a in acts],
              f32_out="only" if form == "f32_only" else None)
    offs = []

    def run():
        y, o = Fn.conv2d_grouped(xd, wd, bd, Fn.PackedGroup(), **kw)
        offs[:] = o
        return y
    staged, patch = _both_modes(L, run, (B, H, W, 128, 1024 * n, 256))
    assert patch.dtype == (torch.float32 if form == "f32_only" else fmt) and patch.shape == (B, 1024 * n, H, W)
    assert torch.equal(patch, staged)
    for off, ref in zip(offs, _grouped_ref(x, ws, bs, acts, shared)):
        assert rel_err(patch[:, off:off + 960], ref) < 1.5e-2
        assert not bool(patch[:, off + 960:off + 1024].float().abs().sum())          # pad rows: zero weights, zero bias


def test_channel_slice_of_a_wider_input(fmt):
    Fn, L = _imp()
    B, H, W = 1, 16, 16
    x = rnd("sl_x", (B, 384, H, W), -2, 2).to(fmt).float()
    w = (rnd("sl_w", (128, 128, 5, 5)) * 0.03).to(fmt).float()
    b = rnd("sl_b", (128,), -0.2, 0.2)
    xd, wd, bd = x.to(DEV, fmt).contiguous(memory_format=CL), w.to(DEV), b.to(DEV)
    staged, patch = _both_modes(L, lambda: Fn.conv2d_slice(xd, 256, wd, bd, kernel_size=5, stride=1, padding=2), (B, H, W, 128, 128, 384, 256))
    assert torch.equal(patch, staged)
    assert rel_err(patch, F.conv2d(x[:, 256:], w, b, 1, 2)) < 1.5e-2


def test_an_image_does_not_depend_on_its_batch(fmt):
    Fn, L = _imp()
    x, w, b = _plain_inputs("bi", 128, (3, 24, 40), fmt)
    xd, wd, bd = x.to(DEV, fmt).contiguous(memory_format=CL), w.to(DEV), b.to(DEV)
    one = xd[1:2].contiguous(memory_format=CL)
    with _mode(2), Fn.no_split_k(), torch.no_grad():
        assert _variant(L, 3, 24, 40, 128, 128)[0] == 256 and _variant(L, 1, 24, 40, 128, 128)[0] == 256
        y3 = Fn.conv2d(xd, wd, bd, kernel_size=5, stride=1, padding=2)
        y1 = Fn.conv2d(one, wd, bd, kernel_size=5, stride=1, padding=2)
    assert torch.equal(y3[1:2], y1)


@pytest.mark.parametrize("case", ["ragged", "grouped"])
def test_guarded_allocations(case, fmt):
    """Input, packed weights and outputs inside NaN-filled guards (tests/memguard.py): no guard byte moves, nothing non-finite reaches the
    output, and the output equals the unguarded run."""
    Fn, L = _imp()
    from hesic_amd import functional
    if case == "ragged":
        B, H, W = 2, 24, 40
        x, w, b = _plain_inputs("ragged_tiles_batch", 128, (B, H, W), fmt)
        ws, bs = [w], [b]
        vargs = (B, H, W, 128, 128)
    else:
        B, H, W = 1, 16, 16
        x, ws, bs = _grouped_inputs(fmt, B, H, W, 2)
        vargs = (B, H, W, 128, 2048, 256)
    xd = x.to(DEV, fmt).contiguous(memory_format=CL)
    wd, bd = [w.to(DEV) for w in ws], [b.to(DEV) for b in bs]

    def run(xt, wt, bt):
        if case == "ragged":
            return Fn.conv2d(xt, wt[0], bt[0], kernel_size=5, stride=1, padding=2, act=L.ACT_RELU)
        return Fn.conv2d_grouped(xt, wt, bt, Fn.PackedGroup(), kernel_size=5, stride=1, padding=2, shared_input=False,
                                 acts=[L.ACT_RELU, L.ACT_NONE], f32_out="only")[0]
    with _mode(2), Fn.no_split_k(), torch.no_grad():
        assert _variant(L, *vargs) == [256, 128, 64, 1]
        plain = run(xd, wd, bd)
        gx = MG.guarded(xd, name="x")
        gw = [MG.guarded(w, name="w") for w in wd]
        gb = [MG.guarded(b_, name="b") for b_ in bd]
        with MG.poisoned_allocations([functional]) as rec:
            out = run(gx, gw, gb)
        assert rec, "no allocation of the package was poisoned"
        MG.check_all([gx] + gw + gb)
    assert bool(torch.isfinite(out.float()).all())
    assert torch.equal(out, plain)


def test_the_workload_launch_repeats_bit_for_bit(fmt):
    """The benchmark's own launch (8 x 32 x 32, two groups of 128 -> 960, fp32-only: 512 blocks, every CU busy for two rounds) five times in
    auto mode, which must select the resident-patch kernel here, against the staged form: the load under which a store hazard shows
     and small shapes do not reach."""
    Fn, L = _imp()
    B, H, W = 8, 32, 32
    x = (rnd("full_x", (B, 256, H, W)) * 0.5).to(DEV, fmt).contiguous(memory_format=CL)
    wd = [(rnd(f"full_w{i}", (960, 128, 5, 5)) * 0.03).to(DEV) for i in range(2)]
    bd = [rnd(f"full_b{i}", (960,), -0.2, 0.2).to(DEV) for i in range(2)]
    packer = Fn.PackedGroup()

    def run():
        return Fn.conv2d_grouped(x, wd, bd, packer, kernel_size=5, stride=1, padding=2, shared_input=False, acts=[L.ACT_RELU, L.ACT_NONE],
                                 f32_out="only")[0].clone()
    with torch.no_grad():
        with _mode(1):
            assert _variant(L, B, H, W, 128, 2048, 256) == [256, 128, 64, 1], "auto mode did not select the resident-patch kernel"
            outs = [run() for _ in range(5)]
        with _mode(0):
            assert _variant(L, B, H, W, 128, 2048, 256)[0] != 256
            ref = run()
    torch.cuda.synchronize()
    assert bool(torch.isfinite(ref).all())
    for o in outs:
        assert torch.equal(o, ref)

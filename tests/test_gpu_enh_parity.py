"""Per-element fp64 parity of the 32-channel enhancement kernels (hesic_amd/csrc/enh.hip) on a real MI355X, in both 16-bit libraries.

Every case of tests/enh_ref.py's tables runs the kernels through their wrappers (``conv3x3_c32``, ``conv3x3_c32_img6``, ``pack_images_c32``,
``resblock_c32``, ``conv3x3_c32_train``, ``conv3x3_c32_out_train``) or through the C ABI (``hesic_conv3x3_c32_wgrad`` with accumulate = 1, without a
bias gradient, at chosen partial counts) and compares EVERY element with the fp64 reference:  |err_e| <= 8 sqrt(n) 2^-24 S_e (+ u |ref_e| for a
16-bit output), exactly 0 where S_e == 0; the ResidualBlock against its hard bar on every element and with at most 5e-4 of the elements outside
the tight bar (enh_ref.py's error model).  tests/test_enh_ref_cpu.py shows on the CPU that these bars fail an unwritten, stale, misplaced or
halo-starved tile, a non-zero pad, swapped channels, a missing bias or residual, a wrong slope, a non-zero intermediate ring, a dropped strip or
block partial, a strip read from the other LDS buffer and an ignored ``accumulate``.

What runs here for the first time in the suite: the persistent loops (a block's second and third tile with the halo prefetch in between, the
ResidualBlock's two-buffer pipeline past stage 1, a wave's second and third strip with the double-buffered LDS-DMA, tile indices that cross an
image in mid-loop), and the variants ``c32_resblock_r3_kernel<*, false>``, planar Cout = 1, 2, 4, planar without a residual, res2 without res1,
img6 without a bias and with an activation, accumulate = 1 onto non-zero slots, dbias == NULL, and the finish kernel's nparts = 1 .. 5, 7, 256.
The multi-trip launches run once more inside guarded and poisoned allocations (tests/memguard.py).

Each case prints  "enh_parity <case> <output> <figure>"  before anything is asserted: the largest |err| / unit bound of an output (after
taking off the storage term), for the ResidualBlock ``hard`` = the largest |err| / hard bar and ``tight_share``.  The values measured when the
tests were written are in profiles/enh_parity.json."""
import contextlib

import pytest
import torch

import conv_grad_ref as G
import enh_ref as E
import memguard as MG

pytestmark = pytest.mark.gpu
DEV = "cuda"
CL = torch.channels_last


@contextlib.contextmanager
def _library(fmt):
    import hesic_amd
    hesic_amd.set_compute_dtype(E.FMT[fmt]["dtype"])
    try:
        yield
    finally:
        hesic_amd.set_compute_dtype(torch.bfloat16)
        hesic_amd.set_compute_dtype(torch.float32)


class _Placer:
    """Operands to the device: 16-bit NHWC maps, fp32 planar images and parameters -- inside NaN guards when ``guard`` is set."""

    def __init__(self, fmt, guard):
        self.dt, self.guard, self.kept = E.FMT[fmt]["dtype"], guard, []

    def _g(self, t, name):
        if self.guard:
            t = MG.guarded(t, name=name)
            self.kept.append(t)
        return t

    def map16(self, t, name="map"):
        return None if t is None else self._g(t.to(DEV, self.dt).contiguous(memory_format=CL), name)

    def f32(self, t, name="f32"):
        return None if t is None else self._g(t.to(DEV).contiguous(), name)

    def check(self):
        MG.check_all(self.kept)


def _allocations(guard):
    from hesic_amd import functional
    return MG.poisoned_allocations([functional]) if guard else contextlib.nullcontext([None])


def _check_plain(tag, R, got):
    res = {q: G.check(R, q, t) for q, t in got.items() if t is not None}
    for q, (ok, ratio, msg) in res.items():
        print(f"enh_parity {tag} {q} {ratio:.4f}")
    for q, (ok, ratio, msg) in res.items():
        assert ok, f"{tag} {msg}"
        assert ratio <= E.C_BAR, f"{tag} {q}: ratio {ratio:.3f}"


def _run_forward(tag, kind, shape, fmt, guard=False, ref=None):
    from hesic_amd import functional as Fn
    k, a = E.FWD_KINDS[kind], E.fwd_operands(kind, shape, fmt)
    with _library(fmt):
        P = _Placer(fmt, guard)
        with _allocations(guard) as rec, torch.no_grad():
            if k.get("pack"):
                y = Fn.pack_images_c32(P.f32(a["xa"], "xa"), P.f32(a["xb"], "xb"))
            elif k.get("img6"):
                y = Fn.conv3x3_c32_img6(P.f32(a["xa"], "xa"), P.f32(a["xb"], "xb"), P.f32(a["w"], "w"), P.f32(a["b"], "b"), act=a["act"])
            else:
                x = P.map16(a["x"], "x")
                assert Fn.conv3x3_c32_ok(x, a["w"].to(DEV))
                r1 = P.map16(a["r1"], "r1") if a["cout"] == 32 else P.f32(a["r1"], "image")
                y = Fn.conv3x3_c32(x, P.f32(a["w"], "w"), P.f32(a["b"], "b"), act=a["act"], res1=r1, res2=P.map16(a["r2"], "r2"))
            torch.cuda.synchronize()
        assert rec, "no allocation of the package was guarded"
        P.check()
    if guard:
        assert bool(torch.isfinite(y.float()).all()), f"{tag}: poison in the output"
    ref = E.fwd_reference(kind, shape, fmt) if ref is None else ref
    if k.get("pack"):
        assert y.dtype == E.FMT[fmt]["dtype"] and y.is_contiguous(memory_format=CL)
        same = torch.equal(y.cpu().view(torch.int16), ref.view(torch.int16))
        print(f"enh_parity {tag} y {'0.0000' if same else 'differs'}")
        assert same, f"{tag}: pack_images_c32 is not bit-exact"
        return
    assert y.dtype == (E.FMT[fmt]["dtype"] if ref["y16"] else torch.float32) and tuple(y.shape) == tuple(ref["ref"]["y"].shape)
    _check_plain(tag, ref, {"y": y})
    if kind == "zero_tile":
        dead = ref["S"]["y"] == 0
        assert int(dead.sum()) >= 32 * E.TH * E.TW and bool((y.float().cpu()[dead] == 0).all())


def _run_resblock(tag, kind, shape, fmt, guard=False, ref=None):
    from hesic_amd import functional as Fn
    a = E.rb_operands(kind, shape, fmt)
    with _library(fmt):
        P = _Placer(fmt, guard)
        with _allocations(guard) as rec, torch.no_grad():
            y = Fn.resblock_c32(P.map16(a["x"], "x"), P.f32(a["w1"], "w1"), P.f32(a["b1"], "b1"), P.f32(a["w2"], "w2"), P.f32(a["b2"], "b2"),
                                act=a["act"], res2=P.map16(a["r2"], "r2"))
            torch.cuda.synchronize()
        assert rec
        P.check()
    if guard:
        assert bool(torch.isfinite(y.float()).all()), f"{tag}: poison in the output"
    R = E.rb_reference(kind, shape, fmt) if ref is None else ref
    assert y.dtype == E.FMT[fmt]["dtype"]
    c = E.resblock_check(R, y)
    print(f"enh_parity {tag} hard {c['ratio_hard']:.4f}")
    print(f"enh_parity {tag} tight_share {c['share_tight']:.3e}")
    assert c["ok_hard"], f"{tag} {c['msg']}"
    assert c["share_tight"] <= E.TIGHT_CAP, f"{tag}: {c['share_tight']:.3g} of the outputs outside the tight bar (cap {E.TIGHT_CAP:.3g})"


# ------------------------------------------------------------------------------------------------------------------------ small shapes, every variant
@pytest.mark.parametrize("tag", list(E.FWD_CASES))
def test_forward_variants(tag):
    _run_forward(tag, *E.FWD_CASES[tag])


@pytest.mark.parametrize("tag", list(E.RB_CASES))
def test_resblock_variants(tag):
    _run_resblock(tag, *E.RB_CASES[tag])


# ------------------------------------------------------------------------------------------------------------------------ the persistent loops
# (the upper decorator varies fastest: a tag's plain and guarded run are adjacent and share enh_ref.cached_multi_reference's two-entry cache)
@pytest.mark.parametrize("guard", [False, True], ids=["plain", "guarded"])
@pytest.mark.parametrize("tag", list(E.MULTI_FWD_CASES))
def test_multi_trip_forward(tag, guard):
    """More than 2 x 512 tiles: blocks make a second and a third trip over the halo prefetch; nine tiles per image, so images end in mid-loop."""
    kind, shape, fmt = E.MULTI_FWD_CASES[tag]
    assert E.tiles(shape) > 2 * E.FWD_BLOCKS
    _run_forward(tag + ("_guarded" if guard else ""), kind, shape, fmt, guard, ref=E.cached_multi_reference(tag))


@pytest.mark.parametrize("guard", [False, True], ids=["plain", "guarded"])
@pytest.mark.parametrize("tag", list(E.MULTI_RB_CASES))
def test_multi_trip_resblock(tag, guard):
    """More than 2 x 256 tiles of 14 x 30: the two-buffer producer / consumer pipeline runs stages 0 .. 3 in block 0."""
    kind, shape, fmt = E.MULTI_RB_CASES[tag]
    assert E.tiles(shape, E.RB_TH, E.RB_TW) > 2 * E.RB_BLOCKS
    _run_resblock(tag + ("_guarded" if guard else ""), kind, shape, fmt, guard, ref=E.cached_multi_reference(tag))


# ------------------------------------------------------------------------------------------------------------------------ weight gradient
def _direct_wgrad(a, fmt, cout, cin, with_db=True, prev=None, guard=True):
    """hesic_conv3x3_c32_wgrad on guarded operands, a NaN-filled guarded workspace and NaN-filled (or prefilled: accumulate = 1) guarded outputs;
    ``guard = False``: the same launch on plain allocations (the workspace and the outputs still start as NaN)."""
    from hesic_amd import _lib as L
    B, _, H, W = a["x"].shape
    with _library(fmt):
        P = _Placer(fmt, guard)
        x, g = P.map16(a["x"], "x"), P.map16(a["g"], "g")
        nws = int(L.lib().hesic_conv3x3_c32_wgrad_ws_bytes())
        ws = P._g(torch.full((nws // 4,), float("nan"), device=DEV), "ws")
        nan = lambda *s: torch.full(s, float("nan"), device=DEV)
        dw = P._g(nan(cout, cin, 3, 3) if prev is None else prev[0].to(DEV), "dw")
        db = P._g(nan(cout) if prev is None else prev[1].to(DEV), "db") if with_db else None
        L.call("hesic_conv3x3_c32_wgrad", L.ptr(x), L.ptr(g), L.ptr(dw), L.ptr(db), cout, cin, int(prev is not None), L.ptr(ws), nws, B, H, W, L.stream())
        torch.cuda.synchronize()
        P.check()
    return {"dw": dw, "db": db}


@pytest.mark.parametrize("fmt", E.FORMATS)
@pytest.mark.parametrize("shape", E.SMALL, ids=lambda s: "%dx%dx%d" % s)
def test_weight_gradient_small(shape, fmt):
    for i, (cout, cin) in enumerate(E.WG_WEIGHTS):
        a = E.wg_operands(shape, fmt, cout, cin)
        R = E.wgrad_reference(a["x"], a["g"], a["w"], a["b"])
        got = _direct_wgrad(a, fmt, cout, cin, with_db=(i != 1))
        _check_plain("wgrad_%dx%dx%d_%s_%dx%d" % (shape + (fmt, cout, cin)), R, got)


@pytest.mark.parametrize("cout,cin", E.WG_WEIGHTS)
def test_multi_trip_weight_gradient(cout, cin):
    """2145 strips for 1024 waves: every wave's second strip, and the third of waves 0 .. 96, go through the double-buffered LDS-DMA; the gradient is
    non-zero at one pixel in 64 (every trip, the first and the last pixel of a strip and the 2-pixel last strip of a row among them), so one
    strip that is dropped or read from the wrong buffer leaves the bar (tests/test_enh_ref_cpu.py)."""
    shape = E.MULTI_WG
    assert E.strips(shape) > 2 * E.WG_WAVES
    a = E.wg_operands(shape, "bf16", cout, cin, multi=True)
    R = E.cached_wg_reference(shape, "bf16", cout, cin, True)
    for guard in (False, True):          # once on plain allocations, once more inside guards
        for with_db in (True, False):
            got = _direct_wgrad(a, "bf16", cout, cin, with_db=with_db, guard=guard)
            _check_plain("multi_wgrad_%dx%d_%s%s" % (cout, cin, "db" if with_db else "nodb", "_guarded" if guard else ""), R, got)


@pytest.mark.parametrize("fmt", E.FORMATS)
@pytest.mark.parametrize("np_", list(E.FINISH_SHAPES))
def test_finish_kernel_partial_counts_and_accumulate(np_, fmt):
    """c32_wgrad_finish_kernel with nparts = 1 .. 5, 7 (its unroll-by-4 loop and tail) and 256, overwriting and adding to non-zero slots."""
    shape = E.FINISH_SHAPES[np_]
    assert E.nparts(shape) == np_
    a = E.wg_operands(shape, fmt)
    R = E.cached_wg_reference(shape, fmt, 32, 32, False)
    _check_plain("finish_nparts_%d_%s" % (np_, fmt), R, _direct_wgrad(a, fmt, 32, 32))
    prev = E.previous_slots(shape)
    Ra = E.wgrad_reference(a["x"], a["g"], a["w"], a["b"], prev=prev)
    _check_plain("finish_nparts_%d_%s_accumulate" % (np_, fmt), Ra, _direct_wgrad(a, fmt, 32, 32, prev=prev))


# ------------------------------------------------------------------------------------------------------------------------ autograd forms (bfloat16)
AUTOGRAD_SHAPES = [(2, 17, 33), E.MULTI_WG]


@pytest.mark.parametrize("cin", [32, 6])
@pytest.mark.parametrize("shape", AUTOGRAD_SHAPES, ids=lambda s: "%dx%dx%d" % s)
def test_conv3x3_c32_train_leaky(shape, cin):
    """y, dx, dw, db of ``conv3x3_c32_train`` with LeakyReLU against ``reference(..., act = LEAKY, y_saved = <device y>)``.  The 6-channel weight runs
    on a 32-channel map (its other channels meet zero weights) whose producer needs no gradient."""
    from hesic_amd import functional as Fn
    multi = shape == E.MULTI_WG
    a = E.wg_operands(shape, "bf16", 32, cin, multi)
    with _library("bf16"):
        P = _Placer("bf16", False)
        x, w, b, gy = P.map16(a["x"]), a["w"].to(DEV).requires_grad_(), a["b"].to(DEV).requires_grad_(), P.map16(a["g"])
        if cin == 32:
            x.requires_grad_()
        assert Fn.conv3x3_c32_train_ok(x, w)
        with _allocations(True) as rec:
            y = Fn.conv3x3_c32_train(x, w, b, act=G.ACT_LEAKY)
            y.backward(gy)
            torch.cuda.synchronize()
        assert rec
    R = G.reference(a["x"][:, :cin], a["w"], a["b"], a["g"], stride=1, pad=1, act=G.ACT_LEAKY, y_saved=y.detach().float().cpu())
    if multi:
        R["n"] = dict(R["n"], **E.nonzero_counts(a["x"][:, :cin], R["g"], tuple(a["w"].shape)))
    _check_plain("train_leaky_%dx%dx%d_cin%d" % (shape + (cin,)), R, {"y": y, "dx": x.grad, "dw": w.grad, "db": b.grad})


@pytest.mark.parametrize("shape", AUTOGRAD_SHAPES, ids=lambda s: "%dx%dx%d" % s)
def test_conv3x3_c32_out_train(shape):
    """The 32 -> 3 output conv plus the image it refines (fp32 planar out): y, the data gradient (16-bit map), dw and db."""
    from hesic_amd import functional as Fn
    multi = shape == E.MULTI_WG
    a = E.wg_operands(shape, "bf16", 3, 32, multi)
    img = E.Operands(shape, "bf16").img[:, :3].contiguous()
    gy = a["g"][:, :3].contiguous()
    with _library("bf16"):
        P = _Placer("bf16", False)
        t, w, b = P.map16(a["x"]).requires_grad_(), a["w"].to(DEV).requires_grad_(), a["b"].to(DEV).requires_grad_()
        with _allocations(True) as rec:
            y = Fn.conv3x3_c32_out_train(t, w, b, img.to(DEV))
            y.backward(gy.to(DEV))
            torch.cuda.synchronize()
        assert rec
    R = G.reference(a["x"], a["w"], a["b"], gy, stride=1, pad=1, y16=False, dx16=True)
    R["ref"]["y"], R["S"]["y"] = R["ref"]["y"] + img.double(), R["S"]["y"] + img.double().abs()
    if multi:
        R["n"] = dict(R["n"], **E.nonzero_counts(a["x"], gy, tuple(a["w"].shape)))
    assert y.dtype == torch.float32 and t.grad.dtype == torch.bfloat16
    _check_plain("out_train_%dx%dx%d" % shape, R, {"y": y, "dx": t.grad, "dw": w.grad, "db": b.grad})


def teardown_module():
    E.clear_cache()

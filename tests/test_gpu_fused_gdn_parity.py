"""Per-element fp64 parity of the fused conv + (I)GDN kernels on a real MI355X, in both 16-bit libraries: the image stage (csrc/sconv.hip:
``sconv_n2w_gdn_fast_kernel``, ``sconv_n2w_gdn_kernel<float | h16_t>``), the wide stages (csrc/conv_igemm.hip: the fused epilogue of
``igemm_glds_kernel`` at its 32 / 64 / 128 pixel tiles and of ``igemm_tr4_kernel<GDN, HALO>``) and the 6 -> 3 cat stage with its 3-channel
(I)GDN (``sconv_6to3_s1_kernel``).

Every case of tests/fused_gdn_ref.py's tables runs through the wrappers (``conv2d_gdn``, ``conv2d_cat``; under autograd for the stored conv
output ``y_pre``, bf16 only: the f16 library refuses training) or, where no wrapper reaches the form, through the C ABI
(``hesic_sconv2d_gdn_forward``: the fast image kernel without a prepacked weight image), and EVERY element of y and y_pre is compared with
the fp64 reference:  |err_e| <= 8 (unit_g + push)_e + extra_e for y, 8 sqrt(n) 2^-24 S_e + u |ref_e| for y_pre, exactly 0 where the
receptive field is all zero.  tests/test_fused_gdn_ref_cpu.py shows on the CPU that these bars fail an unwritten or late tile, a dropped
halo column or a first row read as in-image, a bias left out of the squares, a missing beta', swapped gamma' slabs, a neighbour's norm, the
wrong direction, a y_pre that is y, and for the cat stage swapped halves, the (I)GDN on the wrong half and a non-zero padding ring.

What runs here for the first time outside whole-model tests: the fast image kernel's tile loop (second and third trip with the row prefetch
in between, tile indices crossing an image in mid-loop), its in-kernel weight / gamma' gather, the ``<h16_t>`` image form, ``y_pre`` of every
variant and the fused epilogue at each pixel tile and in both ``igemm_tr4_kernel`` forms.  The multi-trip image cases, one wide case per tile
size, both tr4 forms and one cat case run once more inside guarded and poisoned allocations (tests/memguard.py).

Each case prints  "fused_gdn_parity <case> <output> <ratio>"  before anything is asserted: the largest (|err| - extra)+ / unit of an output.
The values measured when the tests were written are in profiles/fused_gdn_parity.json."""
import contextlib
import ctypes as C
import types

import pytest
import torch

import conv_grad_ref as G
import fused_gdn_ref as Fz
import memguard as MG

pytestmark = pytest.mark.gpu
DEV = "cuda"
CL = torch.channels_last
NAMES = {False: "gdn", True: "igdn"}


@contextlib.contextmanager
def _library(fmt):
    import hesic_amd
    hesic_amd.set_compute_dtype(Fz.FMT[fmt]["dtype"])
    try:
        yield
    finally:
        hesic_amd.set_compute_dtype(torch.bfloat16)
        hesic_amd.set_compute_dtype(torch.float32)


class _Placer:
    """Operands to the device -- inside NaN guards when ``guard`` is set."""

    def __init__(self, fmt, guard):
        self.dt, self.guard, self.kept = Fz.FMT[fmt]["dtype"], guard, []

    def put(self, t, name, dtype=None, nhwc=False):
        if t is None:
            return None
        t = t.to(DEV, dtype or t.dtype)
        t = t.contiguous(memory_format=CL) if nhwc else t.contiguous()
        if self.guard:
            t = MG.guarded(t, name=name)
            self.kept.append(t)
        return t

    def check(self):
        MG.check_all(self.kept)


def _allocations(guard):
    from hesic_amd import functional
    return MG.poisoned_allocations([functional]) if guard else contextlib.nullcontext([None])


def _report(case, res):
    """Print every figure, then assert: ``res`` = {output: (ok, ratio, message)}."""
    for q, (ok, ratio, msg) in res.items():
        print(f"fused_gdn_parity {case} {q} {ratio:.4f}")
    for q, (ok, ratio, msg) in res.items():
        assert ok, f"{case} {msg}"
        assert ratio <= Fz.C_BAR, f"{case} {q}: ratio {ratio:.3f}"


def _finite(case, guard, *ts):
    if guard:
        for t in ts:
            assert bool(torch.isfinite(t.float()).all()), f"{case}: poison in an output"


def _saved_conv_output(y):
    """The conv output the fused training forward stored for GDN's backward."""
    return y.grad_fn.saved_tensors[2]


# ------------------------------------------------------------------------------------------------------------------------ image stage
def _run_image(tag, fmt, inverse, guard=False, train=False):
    from hesic_amd import functional as Fn, _lib as L
    shape, form, opt = Fz.IMAGE[tag]
    o = Fz.operands(tag)
    case = f"{tag}_{fmt}_{NAMES[inverse]}" + ("_train" if train else "") + ("_guarded" if guard else "")
    dt = Fz.FMT[fmt]["dtype"]
    with _library(fmt):
        P = _Placer(fmt, guard)
        x = P.put(o["x"], "x", dt if form == "h16" else None, nhwc=bool(opt.get("nhwc")))
        w, b = P.put(o["w"], "w"), P.put(o["b"], "b")
        beta, gamma = P.put(o["beta"], "beta"), P.put(o["gamma"], "gamma")
        kw = dict(kernel_size=5, stride=2, padding=2, transposed=False, inverse=inverse, beta_min=1e-6, packer=None, gdn_packer=Fn.PackedGdn())
        v = None
        with _allocations(guard) as rec:
            if train:
                y = Fn.conv2d_gdn(x, w.requires_grad_(), b, beta, gamma, **kw)
                v = _saved_conv_output(y)
            elif form == "null_img":
                with torch.no_grad():
                    gp, bp = kw["gdn_packer"].get(beta, gamma, 1e-6)
                    Ho, Wo = G.out_hw(shape[1], shape[2], 5, 2, 2, False)
                    y = P.put(torch.full((shape[0], 128, Ho, Wo), float("nan"), dtype=dt), "y", nhwc=True)
                    d = Fn._sdesc(x, y, 3, 128, 5, 2, 2, False)
                    L.call("hesic_sconv2d_gdn_forward", C.byref(d), L.ptr(x), L.ptr(w), L.ptr(b), L.ptr(gp), L.ptr(bp), int(inverse), L.ptr(y), L.stream())
            else:
                with torch.no_grad():
                    y = Fn.conv2d_gdn(x, w, b, beta, gamma, **kw)
            torch.cuda.synchronize()
        assert rec, "no allocation of the package was guarded"
        P.check()
    assert y.dtype == dt and y.is_contiguous(memory_format=CL)
    _finite(case, guard, y, *(() if v is None else (v,)))
    R = Fz.reference_of(tag, fmt, inverse)
    assert tuple(y.shape) == R["shape"]
    res = {"y": Fz.check(R, y)}
    if v is not None:
        res["y_pre"] = Fz.check_pre(R, v)
    _report(case, res)
    if opt.get("zero_corner"):
        dead = R["dead"]
        assert int(dead.sum()) >= 128 * 2 * 19 * 19 and bool((Fz.to_pc(y.float().cpu())[dead] == 0).all())


IMAGE_RUNS = [(t, f, i) for t in Fz.IMAGE for f in Fz.FORMATS for i in Fz.inverses(t)]


@pytest.mark.parametrize("tag,fmt,inverse", IMAGE_RUNS, ids=[f"{t}-{f}-{NAMES[i]}" for t, f, i in IMAGE_RUNS])
def test_image_stage(tag, fmt, inverse):
    if tag in Fz.IMAGE_TRIPS:
        tiles, grid, per_trip = Fz.image_tiles(Fz.IMAGE[tag][0])
        assert tiles > per_trip * (Fz.IMAGE_TRIPS[tag] - 1)
    _run_image(tag, fmt, inverse)


@pytest.mark.parametrize("inverse", [False, True], ids=["gdn", "igdn"])
@pytest.mark.parametrize("tag", [t for t, c in Fz.IMAGE.items() if c[2].get("ypre")])
def test_image_stage_stores_the_conv_output(tag, inverse):
    """y and y_pre of the training forward (bf16): the second pass through the wave's LDS rows."""
    _run_image(tag, "bf16", inverse, train=True)


@pytest.mark.parametrize("fmt", Fz.FORMATS)
@pytest.mark.parametrize("tag", [t for t, c in Fz.IMAGE.items() if c[2].get("guard")])
def test_image_stage_multi_trip_guarded(tag, fmt):
    for inverse in (False, True):
        _run_image(tag, fmt, inverse, guard=True)
    if fmt == "bf16" and Fz.IMAGE[tag][2].get("ypre"):
        _run_image(tag, fmt, False, guard=True, train=True)


# ------------------------------------------------------------------------------------------------------------------------ wide stage
def _run_wide(tag, fmt, inverse, guard=False, train=False):
    from hesic_amd import functional as Fn
    Cin, k, s, tr, shape, plan, opt = Fz.WIDE[tag]
    o = Fz.operands(tag)
    case = f"{tag}_{fmt}_{NAMES[inverse]}" + ("_train" if train else "") + ("_guarded" if guard else "")
    dt = Fz.FMT[fmt]["dtype"]
    with _library(fmt):
        P = _Placer(fmt, guard)
        x = P.put(o["x"], "x", dt, nhwc=True)
        w, b = P.put(o["w"], "w"), P.put(o["b"], "b")
        beta, gamma = P.put(o["beta"], "beta"), P.put(o["gamma"], "gamma")
        kw = dict(kernel_size=k, stride=s, padding=k // 2, transposed=bool(tr), inverse=inverse, beta_min=1e-6, packer=Fn.PackedWeight(),
                  gdn_packer=Fn.PackedGdn())
        v = None
        prev = Fn.set_phase_fusion(opt.get("pf", 1))
        try:
            with _allocations(guard) as rec:
                if train:
                    y = Fn.conv2d_gdn(x, w.requires_grad_(), b, beta, gamma, **kw)
                    v = _saved_conv_output(y)
                else:
                    with torch.no_grad():
                        y = Fn.conv2d_gdn(x, w, b, beta, gamma, **kw)
                torch.cuda.synchronize()
        finally:
            Fn.set_phase_fusion(prev)
        assert rec, "no allocation of the package was guarded"
        P.check()
    assert y.dtype == dt and y.is_contiguous(memory_format=CL)
    _finite(case, guard, y, *(() if v is None else (v,)))
    R = Fz.reference_of(tag, fmt, inverse)
    assert tuple(y.shape) == R["shape"]
    res = {"y": Fz.check(R, y)}
    if v is not None:
        res["y_pre"] = Fz.check_pre(R, v)
    _report(case, res)


WIDE_RUNS = [(t, f, i) for t in Fz.WIDE for f in Fz.FORMATS for i in Fz.inverses(t)]


@pytest.mark.parametrize("tag,fmt,inverse", WIDE_RUNS, ids=[f"{t}-{f}-{NAMES[i]}" for t, f, i in WIDE_RUNS])
def test_wide_stage(tag, fmt, inverse):
    _run_wide(tag, fmt, inverse)


WIDE_TRAIN = [(t, i) for t in Fz.WIDE for i in Fz.inverses(t)]


@pytest.mark.parametrize("tag,inverse", WIDE_TRAIN, ids=[f"{t}-{NAMES[i]}" for t, i in WIDE_TRAIN])
def test_wide_stage_stores_the_conv_output(tag, inverse):
    """y and y_pre of ``hesic_conv2d_gdn_forward_train`` (bf16): v leaves through the place of the dead squared tile."""
    _run_wide(tag, "bf16", inverse, train=True)


@pytest.mark.parametrize("tag", [t for t, c in Fz.WIDE.items() if c[6].get("guard")])
def test_wide_stage_guarded(tag):
    inverse = bool(Fz.WIDE[tag][3])
    for fmt in Fz.FORMATS:
        _run_wide(tag, fmt, inverse, guard=True)
    _run_wide(tag, "bf16", inverse, guard=True, train=True)


# ------------------------------------------------------------------------------------------------------------------------ cat stage
def _run_cat(tag, guard=False):
    from hesic_amd import functional as Fn
    shape, lay, mode = Fz.CAT[tag]
    o = Fz.operands(tag)
    case = tag + ("_guarded" if guard else "")
    with _library("bf16"):
        P = _Placer("bf16", guard)
        xa = P.put(o["xa"], "xa", nhwc=(lay == "nb"))
        xb = P.put(o["xb"], "xb", torch.bfloat16 if lay == "nb" else None)
        w, b = P.put(o["w"], "w"), P.put(o["b"], "b")
        gdn = None
        if mode:
            gdn = types.SimpleNamespace(beta=P.put(o["beta"], "beta"), gamma=P.put(o["gamma"], "gamma"), inverse=(mode == 2), beta_min=1e-6)
        keep, Fn.FUSE_GDN3 = Fn.FUSE_GDN3, True
        try:
            with _allocations(guard) as rec, torch.no_grad():
                y = Fn.conv2d_cat(xa, xb, w, b, kernel_size=5, stride=1, padding=2, transposed=(mode == 2), gdn=gdn, gdn_on_input=(mode == 2))
                torch.cuda.synchronize()
        finally:
            Fn.FUSE_GDN3 = keep
        assert rec, "no allocation of the package was guarded"
        P.check()
    assert y.dtype == torch.float32
    _finite(case, guard, y)
    R = Fz.cat_reference(tag)
    assert tuple(y.shape) == R["shape"]
    _report(case, {"y": Fz.check(R, y)})


@pytest.mark.parametrize("tag", list(Fz.CAT))
def test_cat_stage(tag):
    _run_cat(tag)


def test_cat_stage_guarded():
    _run_cat(Fz.CAT_GUARD, guard=True)


def teardown_module():
    Fz.clear_cache()

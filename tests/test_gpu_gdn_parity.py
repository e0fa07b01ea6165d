"""Per-element fp64 parity of the GDN / IGDN kernels (hesic_amd/csrc/gdn.hip, the GDN backward of hesic_amd/csrc/wgrad.hip), forward and backward, on a real MI355X.

Every case of tests/gdn_ref.py's table runs the kernels through ``Fn.gdn`` under autograd -- or through the C ABI where a mode has no wrapper
route: the float16 backward, a single NHWC pixel of three channels, accumulation into a prefilled gradient, and ``hesic_gdn_backward_partial``
followed by ``hesic_gdn_param_finish_batched`` -- and checks y, dx, dgamma and dbeta element by element against the fp64 reference:
|got - ref| <= 8 x the element's unit bar (gdn_ref.py's error model), clamped parameters against the masked reference (exactly 0 where the
LowerBound rule stops the gradient).  tests/test_gdn_ref_cpu.py shows on the CPU that this bar fails a dropped pixel, tile or block partial,
a wrong or ignored mask, an untransposed gamma' and a wrong dn formula.  The parameters hold clamped (1e-7, negative), exactly-at-the-bound
and free entries; both signs of dtheta' occur among the clamped ones in every case.

Outputs and workspaces live in NaN-filled guards (tests/memguard.py): the buffer-addressed stores of the tail tile and of the prefetch one
grid stride ahead rely on the range check, and no guard byte may move.

Each case prints  "gdn_parity <case> <output> <max ratio to the unit bar>"  before anything is asserted; the values measured when the tests
were written are in profiles/gdn_parity.json.  A failure names the case, the output, the worst ratio and its pixel, channel and tile."""
import contextlib
import ctypes as C

import pytest
import torch

import gdn_ref as R
import memguard as MG

pytestmark = pytest.mark.gpu
DEV = "cuda"


@contextlib.contextmanager
def _library(fmt):
    """The library of a storage format: bfloat16 or float16 through ``set_compute_dtype`` (fp32 storage runs in either)."""
    import hesic_amd
    if fmt == "f32":
        yield
        return
    hesic_amd.set_compute_dtype(R.FMT[fmt]["dtype"])
    try:
        yield
    finally:
        hesic_amd.set_compute_dtype(torch.bfloat16)
        hesic_amd.set_compute_dtype(torch.float32)


def _assert_all(tag, ref, fmt, got, extra=None, want=None):
    """Every output of ``got`` against its bars; the ratios are printed before anything is asserted."""
    bars = R.bars(ref, fmt)
    want = want or ref["ref"]
    res = {q: R.check(want[q], bars[q], t, q, extra=None if extra is None else extra.get(q)) for q, t in got.items()}
    for q, (ok, ratio, msg) in res.items():
        print(f"gdn_parity {tag} {q} {ratio:.4f}")
    for q, (ok, ratio, msg) in res.items():
        assert ok, f"{tag} {msg}"


def _guarded_empty(shape, dtype, name):
    return MG.guarded(torch.empty(shape, dtype=dtype, device=DEV), name=name)


def _direct_forward(x, beta, gamma, inverse):
    from hesic_amd import _lib as L
    P, Cc = x.shape
    y = _guarded_empty(x.shape, x.dtype, "y")
    L.call("hesic_gdn_forward", L.ptr(x), L.ptr(beta), L.ptr(gamma), L.ptr(y), P, Cc, int(inverse), 1e-6, L.dt(x), L.stream())
    return y


def _direct_backward(x, gy, beta, gamma, inverse, into=None):
    """hesic_gdn_backward_acc on (P, C) NHWC operands; ``into`` = (dgamma, dbeta) prefilled: accumulate = 1."""
    from hesic_amd import _lib as L
    P, Cc = x.shape
    dx = _guarded_empty(x.shape, x.dtype, "dx")
    ws = _guarded_empty((max(64, int(L.lib().hesic_gdn_backward_ws_bytes(P, Cc))),), torch.uint8, "ws")
    if into is None:
        dgamma, dbeta = _guarded_empty((Cc, Cc), torch.float32, "dgamma"), _guarded_empty((Cc,), torch.float32, "dbeta")
    else:
        dgamma, dbeta = MG.guarded(into[0], name="dgamma"), MG.guarded(into[1], name="dbeta")
    L.call("hesic_gdn_backward_acc", L.ptr(x), L.ptr(gy), L.ptr(beta), L.ptr(gamma), L.ptr(dx), L.ptr(dbeta), L.ptr(dgamma), int(into is not None),
           L.ptr(ws), P, Cc, int(inverse), 1e-6, L.dt(x), L.stream())
    torch.cuda.synchronize()
    MG.check_all([dx, ws, dgamma, dbeta])
    return {"dx": dx, "dgamma": dgamma, "dbeta": dbeta}


def _device(o, fmt):
    dt = R.FMT[fmt]["dtype"]
    return (o["x"].to(DEV, dt), None if o["gy"] is None else o["gy"].to(DEV, dt), o["beta"].to(DEV), o["gamma"].to(DEV))


def _run(tag):
    """y (and dx, dgamma, dbeta) of a case as (P, C) / parameter-shaped tensors."""
    from hesic_amd import functional
    from hesic_amd import functional as Fn
    c = R.CASES[tag]
    o, ref = R.case(tag)
    P, Cc, B, fmt, inv = c["P"], c["C"], c["B"], c["fmt"], c["inverse"]
    x, gy, beta, gamma = _device(o, fmt)
    if (fmt == "f16" and c["bwd"]) or (Cc == 3 and P == 1):
        # no wrapper route: float16 is an inference format under autograd, and a (1, 3, 1, 1) tensor is planar to the wrapper
        y = _direct_forward(x, beta, gamma, inv)
        got = _direct_backward(x, gy, beta, gamma, inv)
        MG.check_all([y])
        return ref, dict(got, y=y)
    if c["layout"] == "planar":
        to4 = lambda t: t.view(B, P // B, Cc).permute(0, 2, 1).reshape(B, Cc, P // B, 1).contiguous()
    else:
        to4 = lambda t: t.view(1, P, 1, Cc).permute(0, 3, 1, 2)                      # (1, C, P, 1) in NHWC memory
    back = lambda t: t.detach().permute(0, 2, 3, 1).reshape(P, Cc)
    with MG.poisoned_allocations([functional]) as rec:
        if not c["bwd"]:
            with torch.no_grad():
                got = {"y": back(Fn.gdn(to4(x), beta, gamma, inverse=inv))}
        else:
            x4 = to4(x).detach().requires_grad_()
            beta.requires_grad_(), gamma.requires_grad_()
            y = Fn.gdn(x4, beta, gamma, inverse=inv)
            y.backward(to4(gy))
            got = {"y": back(y), "dx": back(x4.grad), "dgamma": gamma.grad, "dbeta": beta.grad}
        torch.cuda.synchronize()
    assert rec, "no allocation of the package was guarded"
    assert got["y"].dtype == R.FMT[fmt]["dtype"]
    return ref, got


@pytest.mark.parametrize("tag", list(R.CASES))
def test_gdn_parity(tag):
    fmt = R.CASES[tag]["fmt"]
    with _library(fmt):
        ref, got = _run(tag)
        if R.CASES[tag]["bwd"]:
            assert R._both_signs(ref), tag
        _assert_all(tag, ref, fmt, got)


def test_the_grid_stride_shapes_pass_their_launch_caps():
    """The launch caps the shapes are built around, blocks x pixels per block.  The caps are copied from the host code and a change there must
    be followed here AND in gdn_ref.py's table: hesic_gdn_forward in gdn.hip (512 blocks of 128 pixels for 16-bit, 256 of 64 for fp32,
    ``grid_for(P, 256, 2048)`` for three channels), hesic_gdn_backward in wgrad.hip (``tiles < 256 ? tiles : 256`` blocks of 128 pixels,
    ``grid_for(P, 256 * 2, 1024)`` for the fused three-channel pass)."""
    P = lambda g, Cc, fmt, bwd: max(c["P"] for c in R.CASES.values() if (c["group"], c["C"], c["fmt"], c["bwd"]) == (g, Cc, fmt, bwd))
    assert P("stride16", 128, "bf16", True) > 256 * 128 and P("stride16", 128, "f16", False) > 512 * 128
    assert P("wide32", 128, "f32", False) > 256 * 64
    assert P("small", 3, "f32", True) > max(1024 * 512, 2048 * 256)


ACCUMULATE = ["finish_c128_p2176_bf16_gdn", "wide16_c128_p129_bf16_igdn", "small_c3_p513_f32_igdn", "small_c3_p513_bf16_gdn", "generic_c5_p2049_f32_gdn",
              "wide32_c128_p65_f32_igdn"]


@pytest.mark.parametrize("tag", ACCUMULATE)
def test_backward_accumulates_into_a_prefilled_gradient(tag):
    """hesic_gdn_backward_acc with accumulate = 1: expected prefill + gradient, bar the gradient's plus 2^-24 |sum|."""
    from hesic_amd import synthetic
    c = R.CASES[tag]
    o, ref = R.case(tag)
    pre = {"dgamma": synthetic._uniform(tag + ".pre_g", (c["C"], c["C"]), -1, 1), "dbeta": synthetic._uniform(tag + ".pre_b", (c["C"],), -1, 1)}
    with _library(c["fmt"]):
        x, gy, beta, gamma = _device(o, c["fmt"])
        got = _direct_backward(x, gy, beta, gamma, c["inverse"], into=(pre["dgamma"].to(DEV), pre["dbeta"].to(DEV)))
    want = dict(ref["ref"], **{q: pre[q].double() + ref["ref"][q] for q in pre})
    extra = {q: R.U24 * want[q].abs() for q in pre}
    _assert_all(tag + "_accumulate", ref, c["fmt"], got, extra=extra, want=want)


BATCHES = {"nb_1_16_17": (0, "bf16", ["finish_c128_p128_bf16_gdn", "finish_c128_p2048_bf16_igdn", "finish_c128_p2176_bf16_gdn"]),
           "nb_33_17_16_accumulate": (1, "bf16", ["finish_c128_p4224_bf16_igdn", "finish_c128_p2176_bf16_igdn", "finish_c128_p2048_bf16_gdn"]),
           "f16_nb_17_33_17_accumulate": (1, "f16", ["finish_c128_p2176_f16_gdn", "finish_c128_p4224_f16_igdn", "finish_c128_p2176_f16_igdn"])}


@pytest.mark.parametrize("name", list(BATCHES))
def test_partial_backward_and_batched_finish(name):
    """Three ``hesic_gdn_backward_partial`` calls of different block counts, then ONE ``hesic_gdn_param_finish_batched``: dx of every job, and the
    gradients the finish writes (or adds to a prefill: what a training step does) against each job's own reference."""
    from hesic_amd import _lib as L
    from hesic_amd import synthetic
    accumulate, fmt, tags = BATCHES[name]
    with _library(fmt):
        jobs = []
        for tag in tags:
            c = R.CASES[tag]
            o, ref = R.case(tag)
            x, gy, beta, gamma = _device(o, fmt)
            assert L.lib().hesic_gdn_backward_partial_ok(c["P"], 128, L.dt(x))
            dx = _guarded_empty(x.shape, x.dtype, "dx")
            ws = _guarded_empty((int(L.lib().hesic_gdn_backward_ws_bytes(c["P"], 128)),), torch.uint8, "ws")
            pre = {"dgamma": synthetic._uniform(tag + ".pre_g", (128, 128), -1, 1), "dbeta": synthetic._uniform(tag + ".pre_b", (128,), -1, 1)}
            dgamma, dbeta = MG.guarded(pre["dgamma"].to(DEV), name="dgamma"), MG.guarded(pre["dbeta"].to(DEV), name="dbeta")
            L.call("hesic_gdn_backward_partial", L.ptr(x), L.ptr(gy), L.ptr(beta), L.ptr(gamma), L.ptr(dx), L.ptr(ws), c["P"], 128, int(c["inverse"]),
                   1e-6, L.dt(x), L.stream())
            jobs.append({"tag": tag, "ref": ref, "P": c["P"], "x": x, "gy": gy, "beta": beta, "gamma": gamma, "dx": dx, "ws": ws, "dgamma": dgamma,
                         "dbeta": dbeta, "pre": pre})
        n = len(jobs)
        vp, i64, f32 = C.c_void_p * n, C.c_int64 * n, C.c_float * n
        arr = lambda key: vp(*[j[key].data_ptr() for j in jobs])
        L.call("hesic_gdn_param_finish_batched", n, arr("ws"), i64(*[j["P"] for j in jobs]), arr("beta"), arr("gamma"), arr("dgamma"), arr("dbeta"),
               f32(*[1e-6] * n), accumulate, L.stream())
        torch.cuda.synchronize()
        for j in jobs:
            MG.check_all([j["dx"], j["ws"], j["dgamma"], j["dbeta"]])
    for j in jobs:
        ref, pre = j["ref"], j["pre"]
        want, extra = ref["ref"], None
        if accumulate:
            want = dict(ref["ref"], **{q: pre[q].double() + ref["ref"][q] for q in pre})
            extra = {q: R.U24 * want[q].abs() for q in pre}
        _assert_all(f"{j['tag']}_batched_{name}", ref, fmt, {q: j[q] for q in ("dx", "dgamma", "dbeta")}, extra=extra, want=want)


def teardown_module():
    R.clear_cache()

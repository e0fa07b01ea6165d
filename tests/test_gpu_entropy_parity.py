"""Per-element fp64 parity of the likelihood kernels of csrc/entropy.hip (EntropyBottleneck, GaussianConditional, the Gaussian mixture;
forward and backward) on a real MI355X.

Every case runs through ``hesic_amd.functional`` and, where a route needs it, the C ABI (the symbols output, a pixel stride wider than K M with
channel offsets, the fp32-in / fp32-out instantiations, a prepared table, accumulate = 1), and checks EVERY element against the fp64 reference
and bar of tests/entropy_ref.py; y_hat / z_hat, the symbols and the table plumbing are compared value for value.  The forward 16-bit cases also
run on the IEEE-half library.  tests/test_entropy_ref_cpu.py shows on the CPU that the bars are counted, not fitted, and which mutations they
reject.  Each case prints  "entropy_parity <case> <output> <ratio>"  (ratio = max_e (|err_e| - storage term) / unit_e; for the sums the unit is
the whole sum bar; 0 for an exact match, inf for a mismatch where exactness is required) before it asserts; the values measured when the tests
were written are in profiles/entropy_parity.json."""
import ctypes as C
import math

import pytest
import torch

import entropy_ref as E

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


def _bar(case, out, R, got):
    torch.cuda.synchronize()
    ok, ratio, msg = E.check(R, got, name=f"{case} {out}")
    print(f"entropy_parity {case} {out} {ratio:.4f}")
    return ok and ratio <= 1.0, msg


def _exact(case, out, got, want):
    torch.cuda.synchronize()
    got = got.detach().cpu().double().reshape(want.shape)
    same = bool((got == want.double()).all())
    print(f"entropy_parity {case} {out} {0.0 if same else math.inf:.4f}")
    return same, f"{case} {out}: {int((got != want.double()).sum())} of {want.numel()} values differ"


def _assert_all(results):
    for ok, msg in results:
        assert ok, msg


def _formats(c):
    """The 16-bit libraries a forward case runs on (None: an fp32 case, whatever library is loaded)."""
    return (BF, F16) if (c["st"] == "h16" or c["f32in"] == "h16") else (None,)


# =================================================================================================== Gaussian / Gaussian mixture
# Shapes, from the launch code (csrc/entropy.hip):
#   hesic_gmm_forward takes the pair kernel for a 16-bit dtype, K in {1, 5} and even M / stride / offsets; everything else (fp32, odd M = 65, K in
#   {2, 3, 8}) runs gmm_fwd_kernel, one thread per latent, grid capped at 2048 blocks x 256: the second trip needs > 524 288 latents
#   (k1_trip2_f32: 90 x 90 x 65 = 526 500).  The pair kernel has one thread per channel PAIR under the same cap: > 1 048 576 latents
#   (pair_k1_trip2: 100 x 164 x 64 = 1 049 600).  M = 16 is one partial block, M = 192 three pairs of weights rows per pixel; B = 2 everywhere else,
#   so that batch 1 reads weights row 1.  "wide": scales | means are the halves of one (B, HW, 2 K M) tensor (pixel stride 2 K M, m_c_off = K M),
#   HESIC+'s chunk(2, 1).  hesic_gmm_forward_f32in: K in {1, 5}, y_hat stored as 16-bit or fp32.
#   hesic_gmm_backward: block = 64 channels x 4 pixel lanes, M = 65 leaves 63 dead lanes in the second channel group.  pix_per_block =
#   clamp(ceil4(ceil(HW / ceil(1024 / (ceil(M / 64) B)))), 4, 64): HW = 6, 35, 272 give 4 (HW = 6 and 35: a ragged last block, 35 % 4 = 3);
#   bwd_k1_ppb8 (M = 192, B = 2: 171 blocks wanted, HW = 805 -> ceil 5 -> 8; 805 % 8 = 5, 805 % 4 = 1); bwd_k1_cap64 (M = 65, B = 2: 256 wanted,
#   HW = 16 400 -> 65 -> 68 -> capped to 64; 16 400 % 64 = 16).  K = 1 / 5 with a 16-bit dtype take gmm_bwd_kernel<h16_t, 1 / 5>, K = 2, 3, 8 and
#   fp32 the run-time-K form.
def _nchw(c, t, dtype):
    """(B, HW, X) in the kernel's order -> the (B, X, H, W) channels_last tensor functional takes."""
    return t.reshape(c["B"], c["H"], c["W"], -1).to(DEV, dtype).permute(0, 3, 1, 2).contiguous(memory_format=CL)


def _gmm_tensors(name, h16):
    c = E.GMM[name]
    o = E.gmm_operands(name, h16 or BF)
    sdt = F32 if c["st"] == "f32" else h16
    B, K, M = c["B"], c["K"], c["M"]
    t = dict(y=_nchw(c, o["y"], sdt), sc=_nchw(c, o["scales"].reshape(B, -1, K * M), sdt), mu=_nchw(c, o["means"].reshape(B, -1, K * M), sdt),
             w=None if o["weights"] is None else o["weights"].reshape(B, K * M, 1, 1).to(DEV, F32),
             noise=None if o["noise"] is None else _nchw(c, o["noise"], sdt), g=_nchw(c, o["g"], F32),
             gy=None if o["gy"] is None else _nchw(c, o["gy"], sdt))
    return c, o, sdt, t


def _lat(c, x):
    """(B, X, H, W) from the device -> (B, HW, X)."""
    return x.detach().permute(0, 2, 3, 1).reshape(c["B"], c["H"] * c["W"], -1)


def _gmm_functional(Fn, c, t, grad):
    ins = {k: (t[k].clone().requires_grad_() if grad and t[k] is not None else t[k]) for k in ("y", "sc", "mu", "w")}
    if c["K"] > 1:
        yh, lik = Fn.gaussian_mixture(ins["y"], ins["sc"], ins["mu"], ins["w"], c["K"], noise=t["noise"])
    elif c["umq"]:
        yh, lik = Fn.gaussian_conditional(ins["y"], ins["sc"], ins["mu"], noise=t["noise"])
    else:
        yh, lik = Fn.gaussian_conditional(ins["y"], ins["sc"], None, noise=t["noise"])
    return ins, yh, lik


def _gmm_abi_forward(L, c, t, sdt, out_dtype):
    """hesic_gmm_forward / _f32in on the C ABI with the symbols output; wide: one (B, H, W, 2 K M) buffer, scales at offset 0, means at K M."""
    B, K, M, HW = c["B"], c["K"], c["M"], c["H"] * c["W"]
    y = t["y"]
    if c["wide"]:
        both = torch.cat((t["sc"], t["mu"]), 1).contiguous(memory_format=CL)
        sp = mp = L.ptr(both)
        ps, so, mo = 2 * K * M, 0, K * M
    else:
        both = None
        sp, mp, ps, so, mo = L.ptr(t["sc"]), L.ptr(t["mu"]), K * M, 0, 0
    yh = torch.empty((B, M, c["H"], c["W"]), dtype=out_dtype, device=DEV).contiguous(memory_format=CL)
    lik = torch.full((B, M, c["H"], c["W"]), -1.0, dtype=F32, device=DEV).contiguous(memory_format=CL)
    sym = torch.full((B, M, c["H"], c["W"]), -999, dtype=torch.int32, device=DEV).contiguous(memory_format=CL)
    wts = None if t["w"] is None else t["w"].reshape(B, K * M).contiguous()
    d = L.GmmDesc(B, HW, M, K, L.dt(sdt), int(c["umq"]), ps, so, mo, 0.11, 1e-9)
    if c["f32in"]:
        L.call("hesic_gmm_forward_f32in", C.byref(d), L.ptr(y), sp, mp, L.ptr(wts), L.ptr(yh), L.dt(out_dtype), L.ptr(lik), L.ptr(sym), L.stream())
    else:
        L.call("hesic_gmm_forward", C.byref(d), L.ptr(y), sp, mp, L.ptr(wts), L.ptr(t["noise"]), L.ptr(yh), L.ptr(lik), L.ptr(sym), L.stream())
    torch.cuda.synchronize()
    del both
    return yh, lik, sym


@pytest.mark.parametrize("name", list(E.GMM))
def test_gmm_forward(name):
    Fn, L = _imp()
    c = E.GMM[name]
    res = []
    for h16 in _formats(c):
        if h16 is not None:
            _library(h16)
        lib16 = L.h16_dtype()
        c, o, sdt, t = _gmm_tensors(name, h16 or lib16)
        R = E.gmm_reference(name, h16 or lib16, "fwd")
        tag = name + (f"_{_name(h16)}" if h16 else "")
        out_dtype = {None: sdt, "h16": lib16, "f32": F32}[c["f32in"]]
        assert E.fast_path(c, "fwd") == (c["f32in"] is not None or (sdt != F32 and c["K"] in (1, 5) and c["M"] % 2 == 0))
        if not c["wide"] and not c["f32in"]:
            with torch.no_grad():
                _, yh, lik = _gmm_functional(Fn, c, t, False)
            assert yh.dtype == sdt and lik.dtype == F32
            res.append(_exact(tag, "y_hat", _lat(c, yh), R["y_hat"]))
            res.append(_bar(tag, "lik", R["lik"], _lat(c, lik)))
        yh, lik, sym = _gmm_abi_forward(L, c, t, sdt, out_dtype)
        res.append(_exact(tag, "abi_y_hat", _lat(c, yh), R["y_hat"]))
        res.append(_bar(tag, "abi_lik", R["lik"], _lat(c, lik)))
        if c["mode"] == "round":
            res.append(_exact(tag, "symbols", _lat(c, sym), R["symbols"]))
    _assert_all(res)


@pytest.mark.parametrize("name", [n for n, c in E.GMM.items() if c["bwd"]])
def test_gmm_backward(name):
    Fn, L = _imp()
    c, o, sdt, t = _gmm_tensors(name, BF)
    R = E.gmm_reference(name, BF, "bwd")
    B, K, M, HW = c["B"], c["K"], c["M"], c["H"] * c["W"]
    assert E.fast_path(c, "bwd") == (sdt != F32 and K in (1, 5))
    res = []
    comp = lambda x: _lat(c, x).reshape(B, HW, K, M)
    if not c["wide"]:
        ins, yh, lik = _gmm_functional(Fn, c, t, True)
        if t["gy"] is not None:
            torch.autograd.backward([lik, yh], [t["g"], t["gy"]])
        else:
            lik.backward(t["g"])
        assert ins["y"].grad.dtype == sdt and ins["sc"].grad.dtype == sdt
        res.append(_bar(name, "dy", R["dy"], _lat(c, ins["y"].grad)))
        res.append(_bar(name, "dscales", R["dscales"], comp(ins["sc"].grad)))
        if c["means"] or c["umq"]:
            res.append(_bar(name, "dmeans", R["dmeans"], comp(ins["mu"].grad)))
        if K > 1:
            assert ins["w"].grad.dtype == F32
            res.append(_bar(name, "dweights", R["dweights"], ins["w"].grad.reshape(B, K, M)))
    else:
        # the C ABI with the wide stride: gradients land in one (B, H, W, 2 K M) buffer at the operands' offsets
        both = torch.cat((t["sc"], t["mu"]), 1).contiguous(memory_format=CL)
        dboth = torch.full_like(both, float("nan"))
        dy = torch.full_like(t["y"], float("nan"))
        wts = t["w"].reshape(B, K * M).contiguous()
        dw = torch.zeros((B, K * M), dtype=F32, device=DEV)
        d = L.GmmDesc(B, HW, M, K, L.dt(sdt), int(c["umq"]), 2 * K * M, 0, K * M, 0.11, 1e-9)
        L.call("hesic_gmm_backward", C.byref(d), L.ptr(t["y"]), L.ptr(both), L.ptr(both), L.ptr(wts), L.ptr(t["noise"]), L.ptr(t["g"]),
               L.ptr(t["gy"]), L.ptr(dy), L.ptr(dboth), L.ptr(dboth), L.ptr(dw), L.stream())
        torch.cuda.synchronize()
        ds, dm = dboth.chunk(2, 1)
        res.append(_bar(name, "dy", R["dy"], _lat(c, dy)))
        res.append(_bar(name, "dscales", R["dscales"], comp(ds)))
        res.append(_bar(name, "dmeans", R["dmeans"], comp(dm)))
        res.append(_bar(name, "dweights", R["dweights"], dw.reshape(B, K, M)))
    _assert_all(res)


# ========================================================================================================= EntropyBottleneck
# Shapes, from the launch code: block = 16 channels x 16 pixel lanes, grid = (min(ceil(P / 16), cap), ceil(C / 16)).  C = 8: one ragged channel
# group (8 dead channel lanes in every shuffle of the backward); C = 16: one full group; C = 20: a second, ragged group; C = 128: eight groups.
# P = 1: one live pixel lane; P = 17: a second pixel slice with one pixel; forward cap 256 slices: the grid-stride second trip needs P > 4096
# (P = 4097 = 17 x 241); backward cap 32 slices: P > 512 (P = 513 = 19 x 27).  Round mode sends dv to the median column and stores dz = 0,
# noise mode stores dz.  "prepared": the table of hesic_eb_prepare_params (slot 59 set), read without softplus / tanh.
def _eb_tensors(name, h16):
    c = E.EB[name]
    o = E.eb_operands(name, h16 or BF)
    sdt = F32 if c["st"] == "f32" else h16
    cc = dict(c)
    nchw = lambda x, dt: None if x is None else _nchw(cc, x[None], dt)
    ms, bs, fs, q = o["params"]
    dev = lambda ts: [x.to(DEV, F32) for x in ts]
    return c, o, sdt, dict(z=nchw(o["z"], sdt), noise=nchw(o["noise"], sdt), g=nchw(o["g"], F32), gz=nchw(o["gz"], sdt),
                           ms=dev(ms), bs=dev(bs), fs=dev(fs), q=q.to(DEV, F32), table=o["table"].to(DEV, F32).contiguous())


def _pc(x):
    """(1, C, H, W) from the device -> (P, C)."""
    return x.detach().permute(0, 2, 3, 1).reshape(-1, x.shape[1])


@pytest.mark.parametrize("name", list(E.EB))
def test_eb_forward(name):
    Fn, L = _imp()
    c = E.EB[name]
    res = []
    for h16 in _formats(c):
        if h16 is not None:
            _library(h16)
        lib16 = L.h16_dtype()
        c, o, sdt, t = _eb_tensors(name, h16 or lib16)
        R = E.eb_reference(name, h16 or lib16, "fwd")
        tag = name + (f"_{_name(h16)}" if h16 else "")
        out_dtype = {None: sdt, "h16": lib16, "f32": F32}[c["f32in"]]
        P, Cc = o["z"].shape
        with torch.no_grad():
            zh, lik = Fn.entropy_bottleneck(t["z"], t["ms"], t["bs"], t["fs"], t["q"], noise=t["noise"],
                                            packer=Fn.PackedEb() if c["prepared"] else None, out_dtype=out_dtype if c["f32in"] else None)
        assert zh.dtype == out_dtype and lik.dtype == F32
        res.append(_exact(tag, "z_hat", _pc(zh), R["z_hat"]))
        res.append(_bar(tag, "lik", R["lik"], _pc(lik)))
        # the C ABI: the symbols output, and hesic_eb_forward_f32in's fp32-out form
        table = t["table"]
        if c["prepared"]:
            table = torch.empty_like(t["table"])
            L.call("hesic_eb_prepare_params", L.ptr(t["table"]), L.ptr(table), Cc, L.stream())
        zh2 = torch.empty_like(t["z"], dtype=out_dtype, memory_format=CL)
        lik2 = torch.full(t["z"].shape, -1.0, dtype=F32, device=DEV).contiguous(memory_format=CL)
        sym = torch.full(t["z"].shape, -999, dtype=torch.int32, device=DEV).contiguous(memory_format=CL)
        if c["f32in"]:
            L.call("hesic_eb_forward_f32in", L.ptr(t["z"]), L.ptr(table), L.ptr(zh2), L.dt(out_dtype), L.ptr(lik2), L.ptr(sym), P, Cc, L.stream())
        else:
            L.call("hesic_eb_forward", L.ptr(t["z"]), L.ptr(table), L.ptr(t["noise"]), L.ptr(zh2), L.ptr(lik2), L.ptr(sym), P, Cc, L.dt(sdt),
                   L.stream())
        res.append(_exact(tag, "abi_z_hat", _pc(zh2), R["z_hat"]))
        res.append(_bar(tag, "abi_lik", R["lik"], _pc(lik2)))
        if c["mode"] == "round":
            res.append(_exact(tag, "symbols", _pc(sym), R["symbols"]))
    _assert_all(res)


@pytest.mark.parametrize("name", [n for n, c in E.EB.items() if c["bwd"]])
def test_eb_backward(name):
    Fn, L = _imp()
    c, o, sdt, t = _eb_tensors(name, BF)
    R = E.eb_reference(name, BF, "bwd")
    Cc = c["C"]
    leaf = lambda ts: [x.clone().requires_grad_() for x in ts]
    ms, bs, fs = leaf(t["ms"]), leaf(t["bs"]), leaf(t["fs"])
    q = t["q"].clone().requires_grad_()
    z = t["z"].clone().requires_grad_()
    zh, lik = Fn.entropy_bottleneck(z, ms, bs, fs, q, noise=t["noise"])
    if t["gz"] is not None:
        torch.autograd.backward([lik, zh], [t["g"], t["gz"]])
    else:
        lik.backward(t["g"])
    assert z.grad.dtype == sdt
    got = torch.cat([p.grad.reshape(Cc, -1) for p in ms + bs + fs] + [q.grad[:, 0, 1:2]], 1)
    res = [_bar(name, "dz", R["dz"], _pc(z.grad)),
           _bar(name, "dparams", R["dparams"], got),
           _exact(name, "dquantiles_outer", q.grad[:, 0, (0, 2)], torch.zeros((Cc, 2), dtype=torch.float64))]
    _assert_all(res)


@pytest.mark.parametrize("accumulate", [0, 1])
@pytest.mark.parametrize("name", list(E.EB_AUX))
def test_eb_aux_loss(name, accumulate):
    """eb_aux_loss_kernel: one thread per (channel, quantile), 64 per block: C = 8 (24 threads, one partial block), C = 20 (60), C = 128 (384 = six
    full blocks); the scalar loss through one atomic per wave, dquantiles written or accumulated."""
    Fn, L = _imp()
    A = E.aux_reference(name, bool(accumulate))
    Cc = E.EB_AUX[name]
    table = A["table"].to(DEV, F32).contiguous()
    q = A["params"][3].to(DEV, F32).contiguous()
    loss = torch.zeros(1, dtype=F32, device=DEV)
    dq = A["old"].reshape(Cc, 1, 3).to(DEV, F32).contiguous() if accumulate else torch.full((Cc, 1, 3), float("nan"), dtype=F32, device=DEV)
    L.call("hesic_eb_aux_loss", L.ptr(table), L.ptr(q), 1e-9, L.ptr(loss), L.ptr(dq), Cc, accumulate, L.stream())
    tag = f"{name}_acc{accumulate}"
    res = [_bar(tag, "loss", A["loss"], loss), _bar(tag, "dquantiles", A["dq"], dq.reshape(Cc, 3))]
    if not accumulate:
        ms, bs, fs = ([x.to(DEV, F32) for x in ts] for ts in A["params"][:3])
        qq = q.clone().requires_grad_()
        lf = Fn.eb_aux_loss(ms, bs, fs, qq)
        lf.backward()
        res += [_bar(tag, "functional_loss", A["loss"], lf.reshape(1)), _bar(tag, "functional_dquantiles", A["dq"], qq.grad.reshape(Cc, 3))]
    _assert_all(res)


def test_eb_table_plumbing():
    """hesic_eb_pack_table / hesic_eb_scatter_grads (accumulate 0 and 1) against the layout restated in entropy_ref.eb_table, and
    hesic_eb_prepare_params per slot, at C = 20 (1280 table elements: five full blocks of 256)."""
    Fn, L = _imp()
    Cc = 20
    Pr = E.prepare_reference(Cc)
    ms, bs, fs, q = E.eb_params(Cc, 7000 + Cc)
    dev = lambda ts: [x.to(DEV, F32).contiguous() for x in ts]
    dms, dbs, dfs, dq = dev(ms), dev(bs), dev(fs), q.to(DEV, F32).contiguous()
    lay = Fn._eb_layout(dms, dbs, dfs, dq, 1e-9)
    table = torch.full((Cc, L.EB_PARAM_STRIDE), float("nan"), dtype=F32, device=DEV)
    L.call("hesic_eb_pack_table", C.byref(lay), L.ptr(table), Cc, L.stream())
    res = [_exact("table_c20", "pack", table, Pr["raw"])]
    ready = torch.full_like(table, float("nan"))
    L.call("hesic_eb_prepare_params", L.ptr(table), L.ptr(ready), Cc, L.stream())
    res.append(_bar("table_c20", "prepare", Pr, ready))
    # scatter: column j of a gradient table lands in its tensor's element; accumulate = 1 adds to what is there (whole numbers: exact)
    gen = torch.Generator().manual_seed(20)
    dtab = torch.randint(-8, 9, (Cc, L.EB_PARAM_STRIDE), generator=gen).to(F32)
    old = torch.randint(-8, 9, (Cc, L.EB_PARAM_STRIDE), generator=gen).to(F32)
    dtab_dev = dtab.to(DEV)
    for acc in (0, 1):
        host = old if acc else torch.full_like(old, float("nan"))
        tens, k = [], 0
        for p in ms + bs + fs:
            n = p[0].numel()
            tens.append(host[:, k:k + n].reshape(p.shape).to(DEV).contiguous())
            k += n
        gq = torch.full((Cc, 1, 3), 5.0, dtype=F32)
        gq[:, 0, 1] = host[:, 58]
        gq = gq.to(DEV)
        glay = Fn._eb_layout(tens[:5], tens[5:10], tens[10:], gq, 0.0)
        L.call("hesic_eb_scatter_grads", C.byref(glay), L.ptr(dtab_dev), Cc, acc, L.stream())
        torch.cuda.synchronize()
        got = torch.cat([x.reshape(Cc, -1) for x in tens] + [gq[:, 0, 1:2]], 1).cpu()
        want = (old[:, :59] + dtab[:, :59]) if acc else dtab[:, :59]
        res.append(_exact("table_c20", f"scatter_acc{acc}", got, want))
        res.append(_exact("table_c20", f"scatter_acc{acc}_outer_quantiles", gq[:, 0, (0, 2)], torch.full((Cc, 2), 5.0)))
    _assert_all(res)

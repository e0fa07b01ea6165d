"""CPU-only checks of tests/entropy_ref.py, the fp64 references and per-element bars that tests/test_gpu_entropy_parity.py holds
csrc/entropy.hip to.  They show that the bars are neither fitted nor toothless:
  * the chains with every slot at zero ARE the oracle (forward) and its fp64 autograd (the hand-written backward formulas), to 1e-10;
  * torch's own fp32 evaluation of every family stays at or below 1.0 unit (elementwise) / 1.0 of the sum bar: the roundings are counted;
  * an fp64 evaluation with exactly the kernels' by-design approximations (erfc_fast's polynomial, 16-bit stores) stays below the bar, and the
    erfc_fast constants are what the CPU derivation gives;
  * the operands satisfy the construction conditions (no likelihood within x2 of the bound, the shares below it, ties, the scale bound's
    neighbours);
  * each seeded mutation of a correct fp64 result leaves the bar on at least one element in every case that has the feature.
Not detectable, by construction of a sum bar: one dropped term of n once 8 n^1.5 2^-24 exceeds the term's share of S (n > 16 000 for equal
terms): the bottleneck sums here have n <= 1026 and dweights n <= 35 in the small cases, where a dropped pixel is seen; in the 16 400-pixel
dweights case of the GPU test it would not be (8 * 16400^1.5 * 2^-24 = 1.0)."""
import math

import pytest
import torch

import entropy_ref as E
from oracle import hesic_oracle as O

BF = torch.bfloat16
EB_BWD = [n for n, c in E.EB.items() if c["bwd"]]
EB_SMALL = [n for n, c in E.EB.items() if c["B"] * c["H"] * c["W"] <= 513]


def _close(a, b, what):
    a, b = a.double(), b.double()
    d = float(((a - b).abs() / (1.0 + b.abs())).max())
    assert d <= 1e-10, f"{what}: {d:.3g}"


# --------------------------------------------------------------------------------------------------------------- erfc_fast
def test_erfc_fast_constants_are_the_cpu_derivation():
    fit, whole, poly = E.derive_erfc_fast()
    print(f"entropy_ref erfc_fast fit {fit:.4f} whole {whole:.4f} poly {poly:.4f} (units of 2^-24)")
    assert math.ceil(poly) + 1 == E.K_POLY
    assert math.ceil(whole) + 3 == E.K_ERFC_FAST_WHOLE
    # the source comment's "1.8e-7 in fp32 Horner form" is 3.02 units: the fit alone is well inside it, the emulated fp32 Horner form with its
    # rounded argument reaches 3.19 units (1.9e-7)
    assert fit * E.U24 < 1.8e-7
    assert 1.8e-7 < poly * E.U24 < 2.0e-7


# ------------------------------------------------------------------------------------------------- the chains are the oracle
def _nchw(c, t):
    B, H, W = c["B"], c["H"], c["W"]
    return t.reshape(B, H, W, -1).permute(0, 3, 1, 2).contiguous()


def _oracle_gmm(name):
    c = E.GMM[name]
    o = E.gmm_operands(name, BF)
    B, K, M = c["B"], c["K"], c["M"]
    y = _nchw(c, o["y"]).requires_grad_()
    sc = _nchw(c, o["scales"].reshape(B, -1, K * M)).requires_grad_()
    mu = _nchw(c, o["means"].reshape(B, -1, K * M)).requires_grad_()
    nz = None if o["noise"] is None else _nchw(c, o["noise"])
    w = None
    if K > 1:
        w = o["weights"].reshape(B, K * M, 1, 1).clone().requires_grad_()
        yh, lik = O.gmm_forward(y, sc, mu, w, K, training=nz is not None, noise=nz)
    else:
        yh, lik = O.gc_forward(y, sc, mu if c["umq"] else None, training=nz is not None, noise=nz)
        if not c["umq"]:                  # GaussianConditional without means in the quantiser but with them in the likelihood: the K = 1 mixture
            yh, lik = O.gmm_forward(y, sc, mu, torch.ones((B, M, 1, 1), dtype=torch.float64), 1, training=nz is not None, noise=nz)
    return c, o, (y, sc, mu, w), yh, lik


@pytest.mark.parametrize("name", E.GMM_SMALL)
def test_gmm_chain_is_the_oracle(name):
    c, o, ins, yh, lik = _oracle_gmm(name)
    back = lambda t: t.permute(0, 2, 3, 1).reshape(c["B"], c["H"] * c["W"], -1)
    for fast in (False, True):
        ev = E.gmm_evaluate(name, BF, "fwd", fast=fast)
        _close(ev["y_hat"], back(yh.detach()), "y_hat")
        _close(ev["lik"], back(lik.detach()), "lik")
    if not c["bwd"]:
        return
    outs, gs = [lik], [_nchw(c, o["g"])]
    if o["gy"] is not None:
        outs.append(yh)
        gs.append(_nchw(c, o["gy"]))
    grads = torch.autograd.grad(outs, [t for t in ins if t is not None], gs, allow_unused=True)
    dy, dsc, dmu = grads[:3]
    B, K, M = c["B"], c["K"], c["M"]
    comp = lambda t: back(t).reshape(B, -1, K, M)
    for fast in (False, True):
        ev = E.gmm_evaluate(name, BF, "bwd", fast=fast)
        _close(ev["dy"], back(dy) if dy is not None else torch.zeros_like(ev["dy"]), "dy")
        _close(ev["dscales"], comp(dsc), "dscales")
        _close(ev["dmeans"], comp(dmu), "dmeans")
        if K > 1:
            _close(ev["dweights"], grads[3].reshape(B, K, M), "dweights")


def _oracle_eb(name):
    c = E.EB[name]
    o = E.eb_operands(name, BF)
    ms, bs, fs, q = o["params"]
    P = {"p_quantiles": q.clone().requires_grad_()}
    for i, m in enumerate(ms):
        P[f"p__matrices.{i}"] = m.clone().requires_grad_()
    for i, b in enumerate(bs):
        P[f"p__biases.{i}"] = b.clone().requires_grad_()
    for i, f in enumerate(fs):
        P[f"p__factors.{i}"] = f.clone().requires_grad_()
    C = c["C"]
    x = o["z"].t().reshape(1, C, c["H"], c["W"]).clone().requires_grad_()
    nz = None if o["noise"] is None else o["noise"].t().reshape(1, C, c["H"], c["W"])
    return c, o, P, x, nz


@pytest.mark.parametrize("name", EB_SMALL)
def test_eb_chain_is_the_oracle(name):
    c, o, P, x, nz = _oracle_eb(name)
    C = c["C"]
    xh, lik = O.eb_forward(P, "p_", x, training=nz is not None, noise=nz)
    back = lambda t: t.reshape(C, -1).t()
    ev = E.eb_evaluate(name, BF, "fwd")
    _close(ev["z_hat"], back(xh.detach()), "z_hat")
    _close(ev["lik"], back(lik.detach()), "lik")
    if not c["bwd"]:
        return
    outs, gs = [lik], [o["g"].t().reshape(lik.shape)]
    if o["gz"] is not None:
        outs.append(xh)
        gs.append(o["gz"].t().reshape(xh.shape))
    names = [f"p__matrices.{i}" for i in range(5)] + [f"p__biases.{i}" for i in range(5)] + [f"p__factors.{i}" for i in range(4)]
    grads = torch.autograd.grad(outs, [x] + [P[n] for n in names] + [P["p_quantiles"]], gs, allow_unused=True)
    ev = E.eb_evaluate(name, BF, "bwd")
    _close(ev["dz"], back(grads[0]) if nz is not None else torch.zeros_like(ev["dz"]), "dz")
    want = torch.zeros((C, 59), dtype=torch.float64)
    want[:, :58] = torch.cat([g.reshape(C, -1) for g in grads[1:15]], 1)
    if grads[15] is not None:
        want[:, 58] = grads[15][:, 0, 1]
    _close(ev["dparams"], want, "dparams")


@pytest.mark.parametrize("name", list(E.EB_AUX))
def test_aux_chain_is_the_oracle(name):
    A = E.aux_reference(name)
    ms, bs, fs, q = A["params"]
    P = {"p_quantiles": q.clone().requires_grad_()}
    for i in range(5):
        P[f"p__matrices.{i}"], P[f"p__biases.{i}"] = ms[i], bs[i]
    for i in range(4):
        P[f"p__factors.{i}"] = fs[i]
    loss = O.eb_aux_loss(P, "p_")
    _close(A["loss"]["ref"], loss.detach().reshape(1), "loss")
    _close(A["dq"]["ref"], torch.autograd.grad(loss, P["p_quantiles"])[0][:, 0, :], "dquantiles")
    assert abs(E.tail_target() - math.log(2 / 1e-9 - 1)) <= 2 * E.U24 * 22          # the host's fp32 target sits inside its 2-ulp slot


# --------------------------------------------------------------------------------------------------- torch's fp32 evaluation
def _ratios(R, ev, keys, tag):
    worst = 0.0
    for k in keys:
        if k not in R:
            continue
        ok, ratio, msg = E.check(R[k], ev[k], f"{tag} {k}")
        print(f"entropy_ref {tag} {k} {ratio:.4f}")
        assert ok and ratio <= 1.0, msg
        worst = max(worst, ratio)
    return worst


@pytest.mark.parametrize("name", E.GMM_SMALL)
def test_gmm_fp32_evaluation_stays_inside_one_unit(name):
    c = E.GMM[name]
    for what, keys in (("fwd", ("lik",)), ("bwd", ("dy", "dscales", "dmeans", "dweights"))):
        if what == "bwd" and not c["bwd"]:
            continue
        emulate = torch.float32 if E.fast_path(c, what) else None        # the pair form: its own fp32 erfc_fast, fma's included
        ev = E.gmm_evaluate(name, BF, what, dtype=torch.float32, emulate=emulate)
        _ratios(E.gmm_reference(name, BF, what), ev, keys, f"fp32 {name}")


@pytest.mark.parametrize("name", EB_SMALL)
def test_eb_fp32_evaluation_stays_inside_one_unit(name):
    c = E.EB[name]
    _ratios(E.eb_reference(name, BF, "fwd"), E.eb_evaluate(name, BF, "fwd", dtype=torch.float32), ("lik",), f"fp32 {name}")
    if c["bwd"]:
        _ratios(E.eb_reference(name, BF, "bwd"), E.eb_evaluate(name, BF, "bwd", dtype=torch.float32), ("dz", "dparams"), f"fp32 {name}")


@pytest.mark.parametrize("name", list(E.EB_AUX))
def test_aux_and_prepare_fp32_evaluation_stays_inside_one_unit(name):
    """The oracle's aux loss run in fp32 (torch's softplus / tanh / matmul) against the sum bar and the dquantiles unit; torch's fp32 softplus
    and tanh against the per-slot units of the prepared table."""
    A = E.aux_reference(name)
    ms, bs, fs, q = A["params"]
    P = {"p_quantiles": q.float().requires_grad_()}
    for i in range(5):
        P[f"p__matrices.{i}"], P[f"p__biases.{i}"] = ms[i].float(), bs[i].float()
    for i in range(4):
        P[f"p__factors.{i}"] = fs[i].float()
    loss = O.eb_aux_loss(P, "p_")
    dq = torch.autograd.grad(loss, P["p_quantiles"])[0][:, 0, :]
    _ratios(A, dict(loss=loss.detach().reshape(1), dq=dq), ("loss", "dq"), f"fp32 {name}")
    Pr = E.prepare_reference(E.EB_AUX[name])
    raw = Pr["raw"].float()
    got = raw.clone()
    got[:, :33] = torch.nn.functional.softplus(raw[:, :33])
    got[:, 46:58] = torch.tanh(raw[:, 46:58])
    got[:, E.EB_READY] = 1.0
    _ratios(dict(prepare=Pr), dict(prepare=got), ("prepare",), f"fp32 {name}")


# ------------------------------------------------------------------------------------------------------ fast-path emulation
@pytest.mark.parametrize("name", [n for n in E.GMM_SMALL if E.fast_path(n, "fwd") or (E.GMM[n]["bwd"] and E.fast_path(n, "bwd"))])
def test_fast_path_emulation_stays_below_the_bar(name):
    """fp64 with exactly the by-design approximations: erfc_fast's polynomial form (in fp64) and the 16-bit stores of the gradients."""
    c = E.GMM[name]
    worst = 0.0
    for what, keys in (("fwd", ("lik",)), ("bwd", ("dy", "dscales", "dmeans", "dweights"))):
        if not E.fast_path(c, what) or (what == "bwd" and not c["bwd"]):
            continue
        ev = E.gmm_evaluate(name, BF, what, emulate=torch.float64)
        if what == "bwd":
            for k in ("dy", "dscales", "dmeans"):
                ev[k] = ev[k].to(BF).double()
        worst = max(worst, _ratios(E.gmm_reference(name, BF, what), ev, keys, f"emulate {name}"))
    print(f"entropy_ref emulate {name} margin {1.0 - worst:.4f}")
    assert worst < 1.0


# ------------------------------------------------------------------------------------------------- construction conditions
@pytest.mark.parametrize("name", list(E.GMM))
def test_gmm_operands_meet_the_construction_conditions(name):
    c = E.GMM[name]
    for h16 in ((BF, torch.float16) if c["st"] == "h16" and not c["bwd"] else (BF,)):
        o = E.gmm_operands(name, h16)
        f = E._flat(c, o)
        L = E._gmm_lik_plain(c, dict(y=f["y"], mu=f["mu"].t(), sc=f["sc"].t(), noise=f["noise"], w=o["weights"]))
        assert not bool(((L > E.LIK_BOUND / 2) & (L < E.LIK_BOUND * 2)).any())
        below = L < E.LIK_BOUND
        assert float(below.double().mean()) >= 0.01 and float((below & (f["g"] < 0)).double().mean()) >= 0.01
        assert bool((f["g"] > 0).any()) and bool((f["g"] < 0).any())
        sdt = E._sdt(c, h16)
        for k in ("y", "means", "scales", "noise", "gy"):
            assert o[k] is None or torch.equal(o[k].to(sdt).double(), o[k]), k
        sc = o["scales"]
        nb = E._neighbours(sdt)
        assert int((nb < E.SCALE_BOUND).sum()) >= 2 and int((nb >= E.SCALE_BOUND).sum()) >= 2
        for v in nb:
            assert bool((sc == v).any())
        assert bool((sc < 0.03).any()) and bool((sc > 32).any())
        if c["mode"] == "round":
            d = f["y"] - (f["mu"][0] if c["umq"] else 0.0)
            for t in (0.5, -0.5, 1.5, -1.5, 2.5, -2.5):
                assert bool((d == t).any())
        if c["weights"]:
            w = o["weights"]
            assert torch.allclose(w.sum(1), torch.ones_like(w.sum(1)), atol=1e-6) and not torch.equal(w[0], w[1])


@pytest.mark.parametrize("name", list(E.EB))
def test_eb_operands_meet_the_construction_conditions(name):
    c = E.EB[name]
    o = E.eb_operands(name, BF)
    L = E.eb_reference(name, BF, "fwd")["L"]
    assert not bool(((L > E.LIK_BOUND / 2) & (L < E.LIK_BOUND * 2)).any())
    below = L < E.LIK_BOUND
    assert float(below.double().mean()) >= 0.01 and float((below & (o["g"] < 0)).double().mean()) >= 0.01
    assert bool((o["g"] > 0).any()) and bool((o["g"] < 0).any())
    t = o["table"]
    assert bool((t[:, 46:58].abs() > 2.8).any()) and bool((t[:, :33] > 20).any()) and bool((t[:, E.EB_BOUND] == E.LIK_BOUND).all())
    if c["mode"] == "round" and o["z"].numel() >= 64:
        d = o["z"] - t[:, E.EB_MED][None]
        for tie in (0.5, -0.5, 1.5, -1.5, 2.5, -2.5):
            assert bool((d == tie).any())


# ---------------------------------------------------------------------------------------------------------------- mutations
def _report(tag, name, out, R, mutant):
    share, n = E.changed_share(R, mutant)
    print(f"entropy_ref mutation {tag} {name} {out}: {share:.4f} of {n} changed elements leave the bar")
    return share > 0 if n else None          # None: the case has no element this mutation touches


def _swap_pairs(w):
    idx = torch.arange(w.shape[-1]) ^ 1
    return w[..., idx]


@pytest.mark.parametrize("name", E.GMM_SMALL)
def test_gmm_mutations_leave_the_bar(name):
    c = E.GMM[name]
    o = E.gmm_operands(name, BF)
    F = E.gmm_reference(name, BF, "fwd")
    seen = {}

    def fwd(tag, **kw):
        ev = E.gmm_evaluate(name, BF, "fwd", **kw)
        seen[tag] = _report(tag, name, "lik", F["lik"], ev["lik"])
        return ev

    if c["weights"]:
        w = o["weights"]
        fwd("weights of batch 0 for batch 1", ops=dict(o, weights=torch.stack((w[0], w[0]))))
        fwd("one component dropped", mut=("drop_component",))
        if c["M"] % 2 == 0:
            fwd("pair swapped in weights", ops=dict(o, weights=_swap_pairs(w)))
    fwd("scale clamp ignored", mut=("no_clamp",))
    if c["mode"] == "round":
        ev = E.gmm_evaluate(name, BF, "fwd", mut=("round_away",))
        seen["round half away"] = bool((ev["y_hat"] != F["y_hat"]).any())
        print(f"entropy_ref mutation round half away {name} y_hat: {int((ev['y_hat'] != F['y_hat']).sum())} elements differ (bit-exact output)")
    if c["bwd"]:
        Bk = E.gmm_reference(name, BF, "bwd")

        def bwd(tag, out, **kw):
            ev = E.gmm_evaluate(name, BF, "bwd", **kw)
            seen[tag] = _report(tag, name, out, Bk[out], ev[out])

        bwd("scale mask on the clamped scale", "dscales", mut=("mask_on_clamped",))
        bwd("scale mask without dsk < 0", "dscales", mut=("no_dsk_neg",))
        bwd("likelihood mask ignored", "dscales", mut=("no_lik_mask",))
        bwd("likelihood mask without g < 0", "dscales", mut=("no_lik_gneg",))
        if c["umq"] and c["mode"] == "round":
            bwd("dmu not cancelled", "dmeans", mut=("no_dmu_cancel",))
            if c["gy"]:
                bwd("g_yhat missing from dmeans", "dmeans", mut=("no_gy_in_dmeans",))
        if c["weights"]:
            t = Bk["dwt_terms"]                              # (B, HW, K, M)
            HW = t.shape[1]
            lane = torch.arange(HW) % 4 == 1                 # pix_per_block is a multiple of 4: pixel lane 1 of every block
            seen["pixel lane dropped"] = _report("pixel lane dropped", name, "dweights", Bk["dweights"], t[:, ~lane].sum(1))
            ppb = E.pix_per_block(c["B"], HW, c["M"])
            if HW % ppb:
                keep = HW - HW % ppb
                seen["HW tail dropped"] = _report("HW tail dropped", name, "dweights", Bk["dweights"], t[:, :keep].sum(1))
    missed = [k for k, v in seen.items() if not v]           # a mutation that touches nothing counts as missed here
    assert not missed, missed


@pytest.mark.parametrize("name", EB_BWD)
def test_eb_mutations_leave_the_bar(name):
    c = E.EB[name]
    Bk = E.eb_reference(name, BF, "bwd")
    ref = Bk["dparams"]["ref"]
    seen = {}
    P = c["B"] * c["H"] * c["W"]
    last = ref.clone()
    for k, t in Bk["terms"].items():
        last[:, k] -= t[:, P - 1].sum(0)
    seen["last pixel dropped"] = _report("last pixel dropped", name, "dparams", Bk["dparams"], last)
    for tag, mut in (("sigmoid omitted on layer 1", ("no_sigmoid_layer1",)),) + ((("median not accumulated", ("no_median",)),) if c["mode"] == "round" else ()):
        ev = E.eb_evaluate(name, BF, "bwd", mut=mut)
        seen[tag] = _report(tag, name, "dparams", Bk["dparams"], ev["dparams"])
    # The likelihood mask of the bottleneck is visible on dz only (noise mode without g_zhat: elementwise, a masked element is exactly 0).  In the 59
    # sums it is NOT detectable, and the shares are printed without an assertion: an element below the floor carries A (1 - A) <= ~1e-9 into
    # every column, against a bar of 8 sqrt(n) 2^-24 S >= 5e-7 S.
    for tag, mut in (("likelihood mask ignored", ("no_lik_mask",)), ("likelihood mask without g < 0", ("no_lik_gneg",))):
        ev = E.eb_evaluate(name, BF, "bwd", mut=mut)
        _report(tag, name, "dparams", Bk["dparams"], ev["dparams"])
        if c["mode"] == "noise":
            hit = _report(tag, name, "dz", Bk["dz"], ev["dz"])
            if not c["gz"]:           # next to a g_zhat of order 1 the ~1e-10 gradient of an element below the floor is inside 2^-24 |g_zhat|
                seen[tag] = hit
    if c["mode"] == "round" and P * c["C"] >= 64:
        F = E.eb_reference(name, BF, "fwd")
        ev = E.eb_evaluate(name, BF, "fwd", mut=("round_away",))
        seen["round half away"] = bool((ev["z_hat"].to(E._sdt(c, BF)).double() != F["z_hat"]).any())
    tiny = P * c["C"] < 64            # 8 or 20 elements: one or two of them below the floor, not every mask clause has an element
    missed = [k for k, v in seen.items() if v is False or (v is None and not tiny)]
    assert not missed, missed

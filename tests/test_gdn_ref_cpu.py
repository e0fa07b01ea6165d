"""The fp64 reference and error model of tests/gdn_ref.py, checked on the CPU for the cases of the GPU table (tests/test_gpu_gdn_parity.py;
of the wide grid-stride shapes one representative, the 32,769-pixel bf16 backward):

  (a) the closed form agrees with fp64 autograd of the oracle's gdn element by element to 1e-10 relative, LowerBound rule included.  An
      element that is a sum cancelling to nearly nothing gets, on top, the fp64 analogue of its own bar: C_BAR x the fp32 unit bar x 2^-29;
  (b) torch's own fp32 evaluation of forward and backward stays within 1.0 of the fp32 UNIT bar;
  (c) an fp64 evaluation with exactly the by-design 16-bit roundings (``gdn_ref.emulate``) stays below C_BAR / 2 = 4 unit bars: the
      kernels add only 1-ulp v_rsq_f32 / v_sqrt_f32 and fp32 ordering on top, so C_BAR = 8 holds with a factor of two to spare.
      Measured when written: y 1.01, dx 1.75, dgamma 1.83, dbeta 1.62 at most (profiles/gdn_parity.json);
  (d) each deliberate defect of that evaluation -- the last pixel, one 128-pixel tile or one block partial dropped from the parameter sums,
      the LowerBound mask inverted or ignored, gamma' untransposed in the dx sum, GDN's dn formula in an IGDN -- moves at least one element
      out of C_BAR x its bar, in every case that has the defect (``gdn_ref.mutations_of``: a dropped pixel is below the bar of ANY
      per-element test beyond P = 512 at bf16 noise).  The share of moved elements is printed; at bf16 it is 20 - 89 % of dgamma for the
      dropped pixel and 9 - 20 % for a wrong mask, which is why the condition is one element and not a share.

Every figure is printed as  "gdn_ref_cpu <case> <check> <output> <value>"  before it is asserted."""
import pytest
import torch

import gdn_ref as R

CHEAP = [t for t in R.CASES if t not in R.STRIDE] + ["stride16_c128_p32769_bf16_gdn"]
BWD = [t for t in CHEAP if R.CASES[t]["bwd"]]
WIDE16 = [t for t in CHEAP if R.CASES[t]["C"] == 128 and R.CASES[t]["fmt"] != "f32"]


@pytest.mark.parametrize("tag", [t for t in BWD if t not in R.STRIDE])
def test_closed_form_agrees_with_autograd(tag):
    o, ref = R.case(tag)
    auto = R.reference_autograd(o["x"], o["gy"], o["beta"], o["gamma"], ref["inverse"])
    bars = R.bars(ref, "f32")
    for q, a in auto.items():
        b = ref["ref"][q]
        over = ((a - b).abs() - R.C_BAR * 2.0 ** -29 * bars[q][0]).clamp_min(0)
        rel = float(torch.where(over > 0, over / b.abs(), over).max())
        print(f"gdn_ref_cpu {tag} autograd {q} {rel:.3g}")
        assert rel <= 1e-10, (tag, q, rel)
    # the oracle's mask and the closed form's agree entry by entry: the same zeros
    assert torch.equal(auto["dgamma"] == 0, ref["ref"]["dgamma"] == 0) and torch.equal(auto["dbeta"] == 0, ref["ref"]["dbeta"] == 0)


def test_the_parameters_hold_every_kind_of_entry():
    """Clamped (positive, negative), exactly at the bound, free -- and both signs of dtheta' among the clamped entries of every case."""
    for C in (3, 5, 8, 128):
        beta, gamma = R.params(C)
        below = gamma < R.GAMMA_BOUND
        assert bool((gamma[below] > 0).any()) and (C == 3 or bool((gamma[below] < 0).any())), C     # nine entries: index 0 is the only 11th
        assert bool((gamma == R.GAMMA_BOUND).any()) and bool((gamma > 0.01).any())
        assert float(beta[1]) < R.beta_bound() and float(beta[2]) == R.beta_bound()
    for tag in BWD:
        _, ref = R.case(tag)
        assert R._both_signs(ref), tag


@pytest.mark.parametrize("tag", CHEAP)
def test_fp32_evaluation_is_within_the_unit_bar(tag):
    from oracle import hesic_oracle as O
    o, ref = R.case(tag)
    C, P = ref["C"], ref["P"]
    x4 = o["x"].T.reshape(1, C, P, 1).clone().requires_grad_()
    b, g = o["beta"].clone().requires_grad_(), o["gamma"].clone().requires_grad_()
    y = O.gdn(x4, b, g, ref["inverse"])
    back = lambda t: t.detach().reshape(C, P).T
    got = {"y": back(y)}
    if o["gy"] is not None:
        y.backward(o["gy"].T.reshape(1, C, P, 1))
        got.update(dx=back(x4.grad), dgamma=g.grad, dbeta=b.grad)
    bars = R.bars(ref, "f32")
    res = {q: R.check(ref["ref"][q], bars[q], t, q, c=1.0) for q, t in got.items()}
    for q, (ok, ratio, msg) in res.items():
        print(f"gdn_ref_cpu {tag} fp32 {q} {ratio:.4f}")
    for q, (ok, ratio, msg) in res.items():
        assert ok, f"{tag} {msg}"


@pytest.mark.parametrize("tag", WIDE16)
def test_the_rounding_emulation_is_within_half_the_bar(tag):
    o, ref = R.case(tag)
    fmt = R.CASES[tag]["fmt"]
    if "dn" not in ref:                              # forward only
        ref = dict(ref, g=torch.zeros_like(ref["x"]))
    emu = R.emulate(ref, fmt)
    bars = R.bars(ref, fmt)
    res = {q: R.check(ref["ref"][q], bars[q], emu[q], q, c=R.C_BAR / 2) for q in bars}
    for q, (ok, ratio, msg) in res.items():
        print(f"gdn_ref_cpu {tag} emulation {q} {ratio:.4f}")
    for q, (ok, ratio, msg) in res.items():
        assert ok, f"{tag} {msg}"


@pytest.mark.parametrize("tag", BWD)
def test_every_mutation_moves_an_element_out_of_its_bar(tag):
    o, ref = R.case(tag)
    fmt = R.CASES[tag]["fmt"]
    bars = R.bars(ref, fmt)
    clean = R.emulate(ref, fmt)
    assert not any(bool(R.outside(ref["ref"][q], bars[q], clean[q]).any()) for q in bars), tag
    missed = []
    for mut in R.mutations_of(ref, fmt):
        emu = R.emulate(ref, fmt, mut)
        moved = {q: R.outside(ref["ref"][q], bars[q], emu[q]) for q in bars}
        for q, m in moved.items():
            if not torch.equal(emu[q], clean[q]):
                print(f"gdn_ref_cpu {tag} {mut} {q} {float(m.double().mean()):.4f}")
        if not any(bool(m.any()) for m in moved.values()):
            missed.append(mut)
    assert not missed, f"{tag}: no element leaves its bar under {missed}"


def test_a_clamped_entry_is_held_to_exactly_zero_or_its_own_bar():
    """Where theta < bound and the fp64 dtheta' >= 0 the expected value is 0 and the bar the entry's own: a value of the passed-through size
    fails, a sign flip within the bar passes."""
    tag = "wide16_c128_p129_bf16_gdn"
    _, ref = R.case(tag)
    unit, extra = R.bars(ref, "bf16")["dgamma"]
    want = ref["ref"]["dgamma"]
    zeroed = (ref["theta_g"] < R.GAMMA_BOUND) & (want == 0)
    assert bool(zeroed.any()) and bool((unit[zeroed] > 0).all())
    leak = torch.where(zeroed, ref["dg_raw"], want)
    assert bool(R.outside(want, (unit, extra), leak)[zeroed].any())
    flip = torch.where(zeroed, -0.5 * R.C_BAR * unit, want)
    ok, _, msg = R.check(want, (unit, extra), flip, "dgamma")
    assert ok, msg


def teardown_module():
    R.clear_cache()

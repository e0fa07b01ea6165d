"""The fp64 reference and error model of tests/conv_grad_ref.py, checked on the CPU for every case of the GPU table
(tests/test_gpu_conv_grad_parity.py):

  (a) torch's own fp32 evaluation of y / dx / dw / db on the same operands stays within the UNIT bound sqrt(n) 2^-24 S_e (ratio <= 1), so
      the bar c = 8 is more than eight times the error of an honest fp32 evaluation;
  (b) a subtly wrong gradient is caught: for each mutation of the reference (one output pixel's gy dropped, one input channel dropped, the
      last Q % 16 pixels dropped -- a ragged K tail --, one dead tap of a mask leaking) at least 90 % of the elements the mutation changes
      leave their bar.  Asserted for dw in every case, and for db wherever ONE term can be resolved at all: a term of a quarter of the mean
      magnitude m leaves the bar 8 sqrt(n) 2^-24 n m only while 8 n^1.5 2^-24 <= 0.25, i.e. up to n = 6500 output pixels.  The bias sums of
      deconv4_fused (n = 16384: the bar is one whole mean term) and deconv4_im2col (n = 6808) lie above that; their figures are printed
      (0 of 3 and 3 of 3 elements caught when this was written) -- a dropped pixel there shows in dw, which is asserted.  Where a mutation
      changes fewer than ten elements of an output, one of them may stay inside its bar (two dropped gy of opposite sign nearly cancel in
      one of the three bias sums of pre_17x130: 2 of 3 caught).
"""
import pytest
import torch
import torch.nn.functional as F

import conv_grad_ref as R


def _fp32_eval(tag):
    Cin, Cout, k, s, p, tr, _, opt = R.CASES[tag]
    o = R.operands(tag)
    ref = R.cached_reference(tag) if not opt.get("act") else R.reference_of(tag)
    x, w = o["x"].clone().requires_grad_(), o["w"].clone().requires_grad_()
    b = None if o["b"] is None else o["b"].clone().requires_grad_()
    xe = x.abs() if opt.get("in_abs") else x
    we = w if o["mask"] is None else w * o["mask"]
    pre = R._conv(xe, we, b, s, p, bool(tr), opt.get("out_pad", s - 1) if tr else None)
    g = ref["g"].float()                      # bf16-representable: exact in fp32
    grads = torch.autograd.grad(pre, [x, w] + ([b] if b is not None else []), g)
    act = opt.get("act", 0)
    y = torch.relu(pre) if act == R.ACT_RELU else F.leaky_relu(pre, 0.01) if act == R.ACT_LEAKY else pre
    return ref, {"y": y.detach(), "dx": grads[0], "dw": grads[1], "db": grads[2] if b is not None else None}


@pytest.mark.parametrize("tag", list(R.CASES))
def test_fp32_evaluation_is_within_the_unit_bound(tag):
    ref, got = _fp32_eval(tag)
    plain = dict(ref, y16=False, dx16=False)            # the fp32 evaluation stores nothing in bf16
    for q in ("y", "dx", "dw", "db"):
        if got[q] is None:
            continue
        ok, ratio, msg = R.check(plain, q, got[q], c=1.0)
        print(f"conv_grad_ref_cpu {tag} {q} fp32 ratio {ratio:.3f}")
        assert ok and ratio <= 1.0, msg


def _mutated(tag, what):
    """Operands of ``tag`` with one subtle error built in; returns (operands, mask override)."""
    Cin, Cout, k, s, p, tr, (B, H, W), opt = R.CASES[tag]
    o = {n: (None if t is None else t.clone()) for n, t in R.operands(tag).items()}
    if what == "gy_last_pixel":
        o["gy"][-1, :, -1, -1] = 0
    elif what == "x_last_channel":
        o["x"][:, -1] = 0
    elif what == "ragged_tail":              # the last Q % 16 pixels of the K (pixel) dimension of the weight-gradient GEMM
        t = o["x"] if tr else o["gy"]
        r = (t.shape[0] * t.shape[2] * t.shape[3]) % 16
        flat = t[-1].reshape(t.shape[1], -1)
        flat[:, flat.shape[1] - r:] = 0
        t[-1] = flat.reshape(t[-1].shape)
    elif what == "dead_tap_leak":
        o["mask"][:, :, -1, -1] = 1
    return o


def _mutations(tag):
    Cin, Cout, k, s, p, tr, (B, H, W), opt = R.CASES[tag]
    Ho, Wo = R.out_hw(H, W, k, s, p, tr, opt.get("out_pad"))
    Q = B * (H * W if tr else Ho * Wo)
    out = [("gy_last_pixel", ("dw", "db")), ("x_last_channel", ("dw",))]
    if Q % 16:
        out.append(("ragged_tail", ("dw",) if tr else ("dw", "db")))
    if "mask" in opt:
        out.append(("dead_tap_leak", ("dw",)))
    return out


MUTATIONS = [(tag, what, qs) for tag in R.CASES for what, qs in _mutations(tag)]


@pytest.mark.parametrize("tag,what,qs", MUTATIONS, ids=[f"{t}-{w}" for t, w, _ in MUTATIONS])
def test_mutation_of_the_reference_is_caught(tag, what, qs):
    Cin, Cout, k, s, p, tr, _, opt = R.CASES[tag]
    ref = R.cached_reference(tag) if not opt.get("act") else R.reference_of(tag)
    o = _mutated(tag, what)
    y16, dx16 = R.storage(tag)
    # the mutation is in the gradient's terms only: act'(y) stays the true reference's
    mut = R.reference(o["x"], o["w"], o["b"], o["gy"], stride=s, pad=p, transposed=bool(tr), out_pad=opt.get("out_pad"), mask=o["mask"],
                      in_abs=opt.get("in_abs", False), act=opt.get("act", 0), y_saved=ref["ref"]["y"], y16=y16, dx16=dx16)
    for q in qs:
        if ref["ref"][q] is None:
            continue
        diff = (mut["ref"][q] - ref["ref"][q]).abs()
        changed = diff > 0
        assert bool(changed.any()), f"{what} changes no element of {q}"
        caught = diff[changed] > R.bars(ref, q)[changed]
        frac = float(caught.double().mean())
        print(f"conv_grad_ref_cpu {tag} {what} {q}: {int(caught.sum())} of {int(changed.sum())} changed elements caught")
        if q == "db" and 8.0 * ref["n"]["db"] ** 1.5 * R.U24 > 0.25:
            continue                     # one term of n is below what fp32 summation resolves (module docstring)
        # 90 % of fewer than ten elements (the three bias sums of an image-side conv) would mean all of them: one miss is allowed there
        missed = int(changed.sum()) - int(caught.sum())
        assert missed <= max(1.0, 0.1 * int(changed.sum())), f"{what}: only {frac:.3f} of the changed {q} elements leave their bar"


def test_dead_elements_have_a_zero_bar():
    """Dead taps of a mask, and taps that never meet a 2x2 map, have S_e == 0: the bar is exactly 0 there and nowhere else."""
    ref = R.cached_reference("mask_A_taps")
    m = R.operands("mask_A_taps")["mask"]
    assert bool((R.bars(ref, "dw")[m == 0] == 0).all()) and bool((ref["ref"]["dw"][m == 0] == 0).all())
    assert float((R.bars(ref, "dw")[m == 1] > 0).double().mean()) > 0.99
    tiny = R.cached_reference("c5s2_tiny")
    dead = tiny["S"]["dw"] == 0
    assert bool(dead.any()) and bool((tiny["ref"]["dw"][dead] == 0).all())
    ok, _, msg = R.check(tiny, "dw", tiny["ref"]["dw"] + dead * 1e-30)
    assert not ok and "dead elements hit" in msg

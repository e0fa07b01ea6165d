"""The fp64 references and error models of tests/glue_ref.py, checked on the CPU (no GPU needed) for the cases of
tests/test_gpu_glue_parity.py:

  (a) torch's own fp32 evaluation of every family stays within 1.0 of the UNIT bound, so a bar is never tighter than honest fp32 arithmetic;
  (b) seeded mutations of a correct result are rejected: for the warp a dropped tap at the right border, a half-pixel offset and a second
      x-block shifted by one pixel; ``align_corners=False`` for upsample4; one dropped n of the tail for the pooled linear layer; the remainder
      pixels dropped from sum_sq_diff; a tie resolved to the higher index and -inf for the signed-zero channel for spatial_max;
  (c) the bars are tight enough to matter: FINE mutations whose size is a constant written in this file, never a multiple of the bar under
      test, are caught at the bar and would NOT be caught at ten times the bar, so loosening a constant by 10x fails these tests.  Pinned this
      way: the warp forward unit (a 2^-12 pixel offset), the upsample4 forward unit (2^-14 of a pixel), the C_BAR sqrt(n) 2^-24 S sums through
      pooled_linear's dp at N = 960 (one product off by a sixteenth), softmax_k's weights and dlogits (2^-18 relative), the sum term of the
      warp's backward on the 4:1 map (2^-17 S_e, the coordinate term set aside), U_LOG (every log2 off by 2^-21 relative) and sum_sq_diff's unit
      (one pixel with 4 <= d2 <= 8 of 600000 dropped, against a bar of 1.7).  NOT pinned: the coordinate terms of the two backward bars
      (warp, upsample4), the 16-bit storage terms (u is the format's own half-ulp) and expf's 2^-23 term.
"""
import math

import pytest
import torch
import torch.nn.functional as F

import glue_ref as G


def _caught(R, mutated, c):
    """Fraction of the elements a mutation changes that leave their bar  c * unit + store."""
    diff = (mutated.double().reshape(R["ref"].shape) - R["ref"]).abs()
    changed = diff > 0
    assert bool(changed.any()), "the mutation changes nothing"
    bar = c * R["unit"] + R.get("store", 0.0)
    return float((diff > bar)[changed].double().mean()), int(changed.sum())


# ------------------------------------------------------------------------------------------------------------------------ warp
@pytest.mark.parametrize("tag", G.WARP_FWD)
def test_warp_forward_fp32_is_within_the_unit_bound(tag):
    B, Cc, hw, dsize, ac, inv, *_ = G.WARP[tag]
    o = G.warp_operands(tag)
    R = G.warp_reference(tag)
    ok, ratio, msg = G.check(R, G.warp_forward_fp32(o["src"], o["M"], dsize, ac, inv), name=tag)
    print(f"glue_ref_cpu warp {tag} fp32 ratio {ratio:.3f} dead {float(R['dead'].double().mean()):.3f}")
    assert ok and ratio <= 1.0, msg
    assert bool((R["ref"][R["dead"]] == 0).all()) and bool((R["unit"][R["dead"]] == 0).all())


@pytest.mark.parametrize("tag", G.WARP_BWD)
def test_warp_backward_fp32_is_within_the_unit_bound(tag):
    B, Cc, (H, W), dsize, ac, inv, *_ = G.WARP[tag]
    o = G.warp_operands(tag)
    R = G.warp_backward_reference(tag)
    ok, ratio, msg = G.check(R, G.warp_backward_fp32((B, Cc, H, W), o["g"], o["M"], ac, inv), c=1.0, name=tag)
    print(f"glue_ref_cpu warp_bwd {tag} fp32 ratio {ratio:.3f} n max {int(R['n'].max())}")
    assert ok and ratio <= 1.0, msg


def test_warp_cases_reach_their_edges():
    """What the case comments promise, read off the reference: the off-frame case is dead everywhere, the shift case loses taps with weight
    1/2 exactly on the border, the horizon case has both signs of Z, |Z| >= 2^-7 and large finite coordinates, down4 lands 16 destination pixels in each cell."""
    assert bool(G.warp_reference("off_frame")["dead"].all())
    R = G.warp_reference("shift")
    assert bool(((R["sx"] - torch.floor(R["sx"])) == 0.5).all()) and 0.2 < float(R["dead"].double().mean()) < 0.8
    o = G.warp_operands("horizon")
    Z = o["M"][:, 2, 0].double().reshape(-1, 1) * torch.arange(40.0, dtype=torch.float64) + o["M"][:, 2, 2].double().reshape(-1, 1)
    assert bool((Z[:, 20] < 0).all()) and bool((Z[:, 21] > 0).all()) and float(Z.abs().min()) >= 2.0 ** -7
    R = G.warp_reference("horizon")
    assert 100 < float(R["sx"].abs().max()) < 1e6 and 0.2 < float(R["dead"].double().mean()) < 0.8
    n = G.warp_backward_reference("down4")["n"]
    assert 48 <= float(n[:, :, 2:-2, 2:-2].mean()) <= 80          # 16 destination pixels per cell, each reaching four cells
    B, Cc, (H, W), (Ho, Wo), *_ = G.WARP["grid_stride"]
    assert Ho * Wo > 2048 * 256
    B, Cc, (H, W), (Ho, Wo), *_ = G.WARP["fast_wide"]
    assert Wo > 256 and Wo % 256 and Ho % 4 == 2
    B, Cc, (H, W), (Ho, Wo), *_ = G.WARP["c1_45_blocks"]
    nb = -(-Ho * Wo // 256)
    assert B == 1 and Cc == 1 and nb == 45 and nb % 8 and 8 < nb <= 2048             # the generic kernel, one launch row, a ragged remap


WARP_MUTATIONS = {
    "dropped_right_tap": {"taps": lambda xi, yi, k: ~((xi == 299) & (k % 2 == 1))},               # the x1 tap on the last source column
    "half_pixel": {"coords": lambda sx, sy: (sx + 0.5, sy)},
    "second_block_shifted": {"coords": lambda sx, sy: (torch.cat((sx[..., :256], sx[..., 257:], sx[..., -1:] + 1), -1), sy)},
}


@pytest.mark.parametrize("what", list(WARP_MUTATIONS))
@pytest.mark.parametrize("tag", ["fast_wide", "fast_wide_ac"])
def test_warp_mutation_is_caught(tag, what):
    B, Cc, hw, dsize, ac, inv, *_ = G.WARP[tag]
    o = G.warp_operands(tag)
    R = G.warp_reference(tag)
    mut = G.warp_forward_ref(o["src"], o["M"], dsize, ac, inv, **WARP_MUTATIONS[what])["ref"]
    frac, n = _caught(R, mut, 1.0)
    print(f"glue_ref_cpu warp {tag} {what}: {frac:.4f} of {n} changed elements caught")
    assert frac >= 0.99 and not G.check(R, mut)[0]
    if what == "second_block_shifted":
        assert bool((mut[..., :256] == R["ref"][..., :256]).all())


def test_warp_bar_resolves_a_four_thousandth_of_a_pixel():
    """A 2^-12 pixel offset of the sample points (|sx| up to 300): caught at the bar for nine elements in ten, lost at ten times the bar."""
    tag = "fast_wide"
    B, Cc, hw, dsize, ac, inv, *_ = G.WARP[tag]
    o = G.warp_operands(tag)
    R = G.warp_reference(tag)
    mut = G.warp_forward_ref(o["src"], o["M"], dsize, ac, inv, coords=lambda sx, sy: (sx + 2.0 ** -12, sy + 2.0 ** -12))["ref"]
    f1, n = _caught(R, mut, 1.0)
    f10, _ = _caught(R, mut, 10.0)
    print(f"glue_ref_cpu warp fine offset: caught {f1:.3f} at the bar, {f10:.3f} at 10x, of {n}")
    assert f1 >= 0.9 and f10 < 0.5


def test_warp_backward_sum_term_resolves_2_to_the_minus_17():
    """The sum term C_BAR sqrt(n_e) 2^-24 S_e alone (the coordinate term set aside) on the 4:1 map, cells with n_e >= 16: an error of
    2^-17 S_e is outside it (8 sqrt(64) 2^-24 = 2^-18 at n = 64) and would be inside ten times it (n_e <= 156 keeps 2^-17 <= 80 sqrt(n) 2^-24 from n = 3 on)."""
    R = G.warp_backward_reference("down4")
    cells = (R["n"] >= 16) & (R["S"] > 0)
    assert int(cells.sum()) > 1000 and float(R["n"].max()) <= 156
    err = 2.0 ** -17 * R["S"]
    bar = G.C_BAR * R["unit"]
    print(f"glue_ref_cpu warp_bwd sum term: {float((err > bar)[cells].double().mean()):.3f} of {int(cells.sum())} cells caught, "
          f"{float((err > 10 * bar)[cells].double().mean()):.3f} at 10x")
    assert bool((err > bar)[cells].all()) and not bool((err > 10 * bar)[cells].any())
    assert not G.check({"ref": R["ref"], "unit": R["unit"]}, R["ref"] + err * cells, c=G.C_BAR)[0]


# ------------------------------------------------------------------------------------------------------------------- upsample4
@pytest.mark.parametrize("tag", list(G.UPSAMPLE) + list(G.UPSAMPLE_LOOPS) + list(G.CAT))
def test_upsample4_fp32_is_within_the_unit_bound(tag):
    R = G.upsample_reference(tag)
    z = R["z"].clone().requires_grad_()
    up = F.interpolate(z, scale_factor=4, mode="bilinear", align_corners=True)
    up.backward(R["g"])
    ok, ratio, msg = G.check(R["fwd"], up, name=tag)
    ok2, ratio2, msg2 = G.check(dict(R["bwd"], store=R["bwd"]["coord"]), z.grad, c=1.0, name=tag)        # one unit + the coordinate term
    print(f"glue_ref_cpu upsample4 {tag} fp32 bwd against the sum term alone: {G.check(dict(R['bwd'], store=None), z.grad)[1]:.3f} (the device's bar: {G.C_BAR})")
    print(f"glue_ref_cpu upsample4 {tag} fp32 ratio fwd {ratio:.3f} bwd {ratio2:.3f}")
    assert ok and ratio <= 1.0, msg
    assert ok2 and ratio2 <= 1.0, msg2


@pytest.mark.parametrize("tag", ["v8", "scalar", "1x7", "stride"])
def test_upsample4_mutations_are_caught(tag):
    R = G.upsample_reference(tag)
    wrong = F.interpolate(R["z"].double(), scale_factor=4, mode="bilinear", align_corners=False)
    frac, n = _caught(R["fwd"], wrong, 1.0)
    print(f"glue_ref_cpu upsample4 {tag} align_corners=False: {frac:.4f} of {n} caught")
    assert frac >= 0.99
    zz = R["z"].double().requires_grad_()
    F.interpolate(zz, scale_factor=4, mode="bilinear", align_corners=False).backward(R["g"].double())
    frac, n = _caught(R["bwd"], zz.grad, G.C_BAR)
    assert frac >= 0.99


def test_upsample4_bar_resolves_2_to_the_minus_14_of_a_pixel():
    R = G.upsample_reference("stride")
    B, Cc, H, W = G.UPSAMPLE["stride"]
    oy, ox = torch.meshgrid(torch.arange(4.0 * H, dtype=torch.float64), torch.arange(4.0 * W, dtype=torch.float64), indexing="ij")
    sy, sx = (oy * ((H - 1) / (4 * H - 1))).expand(B, -1, -1), (ox * ((W - 1) / (4 * W - 1))).expand(B, -1, -1)
    off = 2.0 ** -14                               # coordinates up to 23: the bar is that much finer than the warp's
    mut = G.sample(R["z"], (sx + off).clamp(max=W - 1), (sy + off).clamp(max=H - 1), pad="edge", k_c=G.K_C_UP)["ref"]
    f1, n = _caught(R["fwd"], mut, 1.0)
    f10, _ = _caught(R["fwd"], mut, 10.0)
    print(f"glue_ref_cpu upsample4 fine offset: caught {f1:.3f} at the bar, {f10:.3f} at 10x, of {n}")
    assert f1 >= 0.9 and f10 < 0.5


# ----------------------------------------------------------------------------------------------------------------- spatial max
@pytest.mark.parametrize("leaky", [False, True])
@pytest.mark.parametrize("tag", list(G.SPATIAL))
def test_spatial_max_reference_and_its_mutations(tag, leaky):
    B, Cc, HW, grad = G.SPATIAL[tag]
    x, g = G.spatial_operands(tag)
    val, arg = G.spatial_max_ref(x, leaky)
    want = x.amax(2)
    want = F.leaky_relu(want, 0.01) if leaky else want
    assert torch.equal(val, want) and bool((torch.gather(x, 2, arg.unsqueeze(2)).squeeze(2) == x.amax(2)).all())
    # the special channels: all negative; a maximum of +0.0 (tied: lowest index); -0.0 everywhere; only the last pixel non-negative
    assert bool((val[:, 0] < 0).all()) and bool((val[:, 1] == 0).all()) and bool((val[:, 2] == 0).all()) and bool((val[:, 3] == 0.5).all())
    assert bool((arg[:, 1] == (HW // 2 if HW > 1 else 0)).all()) and bool((arg[:, 2] == 0).all()) and bool((arg[:, 3] == HW - 1).all())
    # mutations: -inf for the signed-zero channel; a tie resolved to the HIGHER index
    broken = val.clone()
    broken[:, 2] = -math.inf
    assert not torch.equal(broken, val)
    if HW > 1:
        hi = torch.where(x == x.amax(2, keepdim=True), torch.arange(HW), -1).amax(2)
        assert bool((hi[:, 1] == HW - 1).all()) and not torch.equal(hi, arg)
        assert not torch.equal(G.spatial_max_backward_ref(g, val, hi, HW, leaky, torch.float32),
                               G.spatial_max_backward_ref(g, val, arg, HW, leaky, torch.float32))


# ------------------------------------------------------------------------------------------------ pooled linear, softmax over K
@pytest.mark.parametrize("tag", list(G.POOLED))
def test_pooled_linear_fp32_is_within_the_unit_bound(tag):
    R = G.pooled_reference(tag)
    p, g, w, b = R["p"], R["g"], R["w"], R["b"]
    got = {"y": p @ w.T + b, "dp": g @ w, "dw": g.T @ p, "db": g.sum(0)}
    for q, t in got.items():
        ok, ratio, msg = G.check(R[q], t, c=1.0, name=f"{tag} {q}")
        print(f"glue_ref_cpu pooled_linear {tag} {q} fp32 ratio {ratio:.3f}")
        assert ok and ratio <= 1.0, msg


@pytest.mark.parametrize("tag", list(G.POOLED))
def test_pooled_linear_one_dropped_n_of_the_tail_is_caught(tag):
    """The last n of the last n-slice (the ``n + u < n1`` tail) dropped from dpooled, the last j from the logits.  At N = 960 the bar also
    resolves that one product being off by a sixteenth of itself; ten times the bar would not."""
    B, N = G.POOLED[tag]
    R = G.pooled_reference(tag)
    g64, w64, p64 = R["g"].double(), R["w"].double(), R["p"].double()
    gm = g64.clone()
    gm[:, N - 1] = 0
    f1, n = _caught(R["dp"], gm @ w64, G.C_BAR)
    gm[:, N - 1] = g64[:, N - 1] * (1 - 1 / 16)                       # the fine form: that product off by a sixteenth
    f16, _ = _caught(R["dp"], gm @ w64, G.C_BAR)
    f10, _ = _caught(R["dp"], gm @ w64, 10 * G.C_BAR)
    pm = p64.clone()
    pm[:, N - 1] = 0
    fy, _ = _caught(R["y"], pm @ w64.T + R["b"].double(), G.C_BAR)
    print(f"glue_ref_cpu pooled_linear {tag} dropped n: dp caught {f1:.3f} of {n}; y caught {fy:.3f}; a sixteenth: {f16:.3f} (10x: {f10:.3f})")
    assert f1 >= 0.99 and fy >= 0.99
    if tag == "3x960":
        assert f16 >= 0.7 and f10 < 0.3


@pytest.mark.parametrize("tag", list(G.SOFTMAX))
def test_softmax_k_fp32_is_within_the_unit_bound(tag):
    K, M = G.SOFTMAX[tag]
    l = G.softmax_logits(tag)
    B = l.shape[0]
    R = G.softmax_ref(l, K, M)
    w = torch.softmax(l.reshape(B, K, M), 1).reshape(B, K * M)
    ok, ratio, msg = G.check(R, w, c=1.0, name=tag)
    print(f"glue_ref_cpu softmax_k {tag} fp32 ratio {ratio:.3f}")
    assert ok and ratio <= 1.0, msg
    ref = R["ref"].reshape(B, K, M)
    assert bool((ref[:, :, 0] == 1.0 / K).all()) and float(ref[:, 0, 1].max()) < 1e-34 and float(ref[:, -1, 1].min()) > 0.99
    g = G.grid16(f"sm.{tag}.g", (B, K * M))
    Rb = G.softmax_backward_ref(w, g, K, M)
    w3, g3 = w.reshape(B, K, M), g.reshape(B, K, M)
    ok, ratio, msg = G.check(Rb, w3 * (g3 - (g3 * w3).sum(1, keepdim=True)), c=1.0, name=tag)
    assert ok and ratio <= 1.0, msg
    # every weight / gradient off by 2^-18 relative (3.8e-6) against C_BAR sqrt(K) 2^-24 (+ 2^-23) = 1.2e-6 / 0.9e-6 relative: outside the bar
    # as it stands, inside a ten times looser one (for dlogits: 80 sqrt(K + 1) >= 64 and |ref| <= w (|g| + sum |g w|))
    fine = 1 + 2.0 ** -18
    assert not G.check(R, R["ref"] * fine, c=G.C_BAR)[0] and G.check(dict(R, unit=10 * R["unit"]), R["ref"] * fine, c=G.C_BAR)[0]
    assert not G.check(Rb, Rb["ref"] * fine, c=G.C_BAR)[0] and G.check(dict(Rb, unit=10 * Rb["unit"]), Rb["ref"] * fine, c=G.C_BAR)[0]
    # a weight computed without the max subtraction overflows at a spread of 80: the reference has no NaN, the naive form does
    naive = torch.exp(l.reshape(B, K, M) * 3) / torch.exp(l.reshape(B, K, M) * 3).sum(1, keepdim=True)
    assert bool(torch.isnan(naive).any()) and bool(torch.isfinite(R["ref"]).all())


# ------------------------------------------------------------------------------------------------------------------ reductions
@pytest.mark.parametrize("tag", list(G.SUM_LOG2))
def test_sum_log2_fp32_is_within_the_unit_bound(tag):
    n, off = G.SUM_LOG2[tag]
    lik = G.likelihoods(tag)[off:]
    R = G.sum_log2_ref(lik)
    ok, ratio, msg = G.check(R, torch.log2(lik).double().sum().reshape(1), c=1.0, name=tag)
    print(f"glue_ref_cpu sum_log2 {tag} fp32 ratio {ratio:.3f}")
    assert ok and ratio <= 1.0, msg
    # every log2 off by 2^-21 relative (four ulp of a value near 1, all one way): 4.8e-7 against U_LOG = 2.3e-7, inside ten times U_LOG
    fine = R["ref"] * (1 + 2.0 ** -21)
    assert not G.check(R, fine, c=1.0)[0] and G.check(dict(R, unit=10 * R["unit"]), fine, c=1.0)[0]
    if n > 1:                    # the scalar tail (n % 4 elements, or everything when unaligned) dropped
        tail = n % 4 or n
        assert not G.check(R, torch.log2(lik[:n - tail].double()).sum().reshape(1), c=1.0)[0] or tail == n


@pytest.mark.parametrize("tag", list(G.SQ_DIFF))
def test_sum_sq_diff_fp32_and_dropped_pixels(tag):
    a, b = G.sq_diff_operands(tag)
    B, Cc, H, W = a.shape
    R = G.sum_sq_diff_ref(a, b)
    part = ((a - b) ** 2).sum(1)                                    # fp32 per pixel, as the kernel forms it
    ok, ratio, msg = G.check(R, part.double().sum().reshape(1), c=1.0, name=tag)
    print(f"glue_ref_cpu sum_sq_diff {tag} fp32 ratio {ratio:.3f}")
    assert ok and ratio <= 1.0, msg
    npix = B * H * W
    rem = G.remainder_pixels(npix)                                  # what the unrolled loop leaves to the remainder loop
    assert len(rem) == {"50x100": 360, "2x2": 4, "big": 75712}.get(tag, npix) and len(torch.unique(rem)) == len(rem)
    if Cc == 3:
        dropped = G.sum_sq_diff_ref(a, b, drop=rem)["ref"]
        assert not G.check(R, dropped, c=1.0)[0]
    if tag == "big":
        # one pixel of 600000, picked by an ABSOLUTE window (4 <= d2 <= 8; the bar is 2^-23 * 3 * sum = 1.7): visible at the bar, and a ten
        # times looser constant in sum_sq_diff_ref (17) lets it through, which fails the first assertion
        d2 = ((a.double() - b.double()) ** 2).sum(1).reshape(-1)
        assert 1.5 < float(R["unit"]) < 2.0
        cand = torch.nonzero((d2 >= 4.0) & (d2 <= 8.0)).reshape(-1)
        assert len(cand) > 0
        one = G.sum_sq_diff_ref(a, b, drop=cand[:1])["ref"]
        print(f"glue_ref_cpu sum_sq_diff big: dropped pixel d2 {float(d2[cand[0]]):.4f} against a bar of {float(R['unit']):.4f}")
        assert not G.check(R, one, c=1.0)[0]
        assert G.check(dict(R, unit=10 * R["unit"]), one, c=1.0)[0]


def test_operands_are_exact_in_every_storage_format():
    x = G.grid16("exact", (4096,))
    for dt in (torch.bfloat16, torch.float16):
        assert torch.equal(x.to(dt).float(), x)
    assert bool((x == 0).any()) and bool((x > 0).any()) and bool((x < 0).any())
    l = G.softmax_logits("5x192")
    assert torch.equal((l * 16).round() / 16, l)                     # differences of logits are exact in fp32

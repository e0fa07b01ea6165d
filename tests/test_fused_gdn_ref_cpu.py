"""tests/fused_gdn_ref.py checked on the CPU: the reference against the oracle in fp64, the by-design roundings against the bars (below
C_BAR / 2 for every case of the tables), deliberate defects against the bars (each must leave its bar at every position it is applied to),
and the case tables' claims about the launch plans (hesic_conv2d_variant: host logic, no GPU)."""
import ctypes as C
import os

import pytest
import torch

import conv_grad_ref as G
import fused_gdn_ref as Fz
import gdn_ref as GR

MUT_TILES = "img_50x70"          # odd Ho, partial 16-column tiles, two images
MUT_HALO = "img_odd"             # odd W: ix0 + 4 == W - 1 exists


def teardown_module():
    Fz.clear_cache()
    GR.clear_cache()


# ------------------------------------------------------------------------------------------------------------------------ the reference
@pytest.mark.parametrize("tag", ["img_50x70", "img_unrounded", "w_c32_t64", "w_d192_t32"])
@pytest.mark.parametrize("fmt", Fz.FORMATS)
def test_reference_equals_the_oracle_in_fp64(tag, fmt):
    from oracle import hesic_oracle as O
    o = Fz.operands(tag)
    s, p, tr = Fz.geometry(tag)
    x, w = Fz.rnd(o["x"], fmt).double(), Fz.rnd(o["w"], fmt).double()
    b = None if o["b"] is None else o["b"].double()
    for inverse in (False, True):
        R = Fz.reference_of(tag, fmt, inverse)
        v = (O.deconv if tr else O.conv)(x, w, b, s)
        y = O.gdn(v, o["beta"].double(), o["gamma"].double(), inverse)
        assert tuple(y.shape) == R["shape"]
        assert float((Fz.to_pc(y) - R["ref"]).abs().max()) <= 1e-12 * float(y.abs().max())
        assert float((v - R["conv"]["ref"]["y"]).abs().max()) <= 1e-12 * float(v.abs().max())


@pytest.mark.parametrize("tag", ["cat_17x130_pp_m0", "cat_17x130_nb_m1", "cat_17x131_pp_m2"])
def test_cat_reference_equals_the_oracle_in_fp64(tag):
    from oracle import hesic_oracle as O
    o = Fz.operands(tag)
    mode = Fz.CAT[tag][2]
    xa, xb, w, b = (o[k].double() for k in ("xa", "xb", "w", "b"))
    beta, gamma = o["beta"].double(), o["gamma"].double()
    if mode == 2:
        y = O.deconv(torch.cat((O.gdn(xa, beta, gamma, True), xb), 1), w, b, 1)
    else:
        y = O.conv(torch.cat((xa, xb), 1), w, b, 1)
        if mode == 1:
            y = O.gdn(y, beta, gamma, False)
    R = Fz.cat_reference(tag)
    assert float((Fz.to_pc(y) - R["ref"]).abs().max()) <= 1e-12 * float(y.abs().max())


def test_unrounded_operands_are_not_representable():
    """The case that pins RNE multiplies operands neither format holds; every other case multiplies operands both formats hold."""
    o = Fz.operands("img_unrounded")
    for fmt in Fz.FORMATS:
        assert not torch.equal(Fz.rnd(o["x"], fmt), o["x"]) and not torch.equal(Fz.rnd(o["w"], fmt), o["w"])
    for tag in ("img_50x70", "w_c32_t64", "img_v300"):
        o = Fz.operands(tag)
        for fmt in Fz.FORMATS:
            assert torch.equal(Fz.rnd(o["x"], fmt), o["x"]) and torch.equal(Fz.rnd(o["w"], fmt), o["w"])
    v = Fz.case_conv("img_v300", "f16")["v"].abs()
    assert 200 < float(v.mean()) < 400 and float(v.max()) < 2047          # squares 2^-6 stay inside binary16


def test_zero_corner_is_dead():
    R = Fz.reference_of("img_zero", "bf16", False)
    dead = R["dead"]
    assert int(dead.all(1).sum()) == 2 * 19 * 19 and bool((R["bar"][0][dead] == 0).all()) and bool((R["ref"][dead] == 0).all())
    got = R["ref"].clone()
    got[torch.nonzero(dead.all(1))[0, 0], 5] = 2.0 ** -30                  # anything but 0 in a dead element is a miss
    assert bool(Fz.outside(R, got).any())


# ------------------------------------------------------------------------------------------------------------------------ the roundings
@pytest.mark.parametrize("tag", list(Fz.IMAGE) + list(Fz.WIDE))
def test_emulation_stays_below_half_the_bar(tag):
    for fmt in Fz.FORMATS:
        Rc = Fz.case_conv(tag, fmt)
        for inverse in Fz.inverses(tag):
            R = Fz.reference_of(tag, fmt, inverse)
            y, pre = Fz.emulate(Rc, R, fmt)
            ok, ratio, msg = GR.check(R["ref"], R["bar"], y, "y", Fz.C_BAR)
            okp, ratio_p, msgp = Fz.check_pre(R, Fz.from_pc(pre, R["shape"]))
            print(f"fused_gdn_emulate {tag} {fmt} {'igdn' if inverse else 'gdn'} y {ratio:.4f} y_pre {ratio_p:.4f}")
            assert ok and ratio < Fz.C_BAR / 2, f"{tag} {fmt} {msg}"
            assert okp and ratio_p < Fz.C_BAR / 2, f"{tag} {fmt} {msgp}"
            del R


@pytest.mark.parametrize("tag", list(Fz.CAT))
def test_cat_stage_in_fp32_stays_below_its_unit(tag):
    """A plain fp32 torch evaluation of the cat stage against the fp64 reference: below 1.0 of the unit."""
    o = Fz.operands(tag)
    mode = Fz.CAT[tag][2]
    xa, xb, w, b = o["xa"], o["xb"], o["w"], o["b"]

    def gdn32(x, inverse):
        bp = o["beta"].clamp_min(GR.beta_bound()) ** 2 - GR.PED
        gp = o["gamma"].clamp_min(GR.GAMMA_BOUND) ** 2 - GR.PED
        n = torch.nn.functional.conv2d(x * x, gp.reshape(3, 3, 1, 1), bp)
        return x * (n.sqrt() if inverse else n.rsqrt())
    if mode == 2:
        y = torch.nn.functional.conv_transpose2d(torch.cat((gdn32(xa, True), xb), 1), w, b, padding=2)
    else:
        y = torch.nn.functional.conv2d(torch.cat((xa, xb), 1), w, b, padding=2)
        if mode == 1:
            y = gdn32(y, False)
    R = Fz.cat_reference(tag)
    ok, ratio, msg = Fz.check(R, y)
    print(f"fused_gdn_emulate {tag} fp32 y {ratio:.4f}")
    assert ok and ratio < 1.0, msg


# ------------------------------------------------------------------------------------------------------------------------ the defects
def _positions(tag):
    """Wave tiles a defect is applied to: a full interior tile, a partial tile at the right edge, one in the last (odd) row of an image, the
    first tile of the second image and the very last tile."""
    B, _, Ho, Wo = Fz.reference_of(tag, "bf16", False)["shape"]
    tx_n, ty_n = (Wo + 15) // 16, (Ho + 1) // 2
    assert Ho % 2 == 1 and Wo % 16 and B == 2
    return {"interior": Fz.TILE_LATE_STRIDE + tx_n, "right_edge": Fz.TILE_LATE_STRIDE + 2 * tx_n - 1, "last_row": tx_n * ty_n - tx_n,
            "second_image": tx_n * ty_n, "last": B * tx_n * ty_n - 1}


@pytest.mark.parametrize("fmt", Fz.FORMATS)
@pytest.mark.parametrize("inverse", [False, True], ids=["gdn", "igdn"])
def test_every_defect_leaves_its_bar(fmt, inverse):
    for tag, muts in ((MUT_TILES, Fz.TILE_MUTATIONS), (MUT_HALO, ("drop_halo_col", "first_row_in_image"))):
        Rc, R = Fz.case_conv(tag, fmt), Fz.reference_of(tag, fmt, inverse)
        y0, pre0 = Fz.emulate(Rc, R, fmt)
        assert not bool(Fz.outside(R, y0).any())
        pre_out = lambda pre: ~((pre - Fz.to_pc(R["conv"]["ref"]["y"])).abs() <= Fz.to_pc(G.bars(R["conv"], "y")))
        assert not bool(pre_out(pre0).any())
        places = _positions(tag) if tag == MUT_TILES else {"line": None}
        for mut in muts:
            for where, t in places.items():
                y, pre, touched = Fz.mutate(Rc, R, fmt, mut, t)
                bad_y, bad_p = Fz.outside(R, y), pre_out(pre)
                hit = bad_p if mut.startswith("ypre") else bad_y
                assert bool(touched.any()) and bool(hit[touched].any()), f"{mut} at {where} ({fmt}) stays inside every bar"
                assert not bool(bad_y[~touched].any()) and not bool(bad_p[~touched].any())
                if mut in ("drop_halo_col", "first_row_in_image"):     # a halo defect shows in v too
                    assert bool(bad_p[touched].any()), f"{mut}: y_pre stays inside its bar"


@pytest.mark.parametrize("tag", ["cat_17x130_pp_m0", "cat_17x130_nb_m1", "cat_17x130_nb_m2", "cat_17x131_pp_m2"])
def test_every_cat_defect_leaves_its_bar(tag):
    R = Fz.cat_reference(tag)
    B, _, H, W = R["shape"]
    for mut in Fz.CAT_MUTATIONS[Fz.CAT[tag][2]]:
        bad = Fz.outside(R, Fz.cat_reference(tag, mut)["ref"]).any(1).reshape(B, H, W)
        assert bool(bad.any()), f"{tag} {mut}"
        if mut == "pad_not_zero":          # every border line of every image shows it, and nothing beyond the halo does
            assert bool(bad[:, 0].any(1).all()) and bool(bad[:, -1].any(1).all()) and bool(bad[:, :, 0].any(1).all()) and bool(bad[:, :, -1].any(1).all())
            assert not bool(bad[:, 4:-4, 4:-4].any())
        else:                              # every row of every image
            assert bool(bad.any(2).all())


# ------------------------------------------------------------------------------------------------------------------------ the tables' claims
def _lib():
    from hesic_amd import _lib as L
    if not os.path.exists(L.LIB_PATH):
        import __graft_entry__ as ge
        ge.build()
    return L


@pytest.mark.parametrize("tag", list(Fz.WIDE))
def test_wide_cases_take_the_planned_tile(tag):
    L = _lib()
    l = L.lib()
    B, H, W, Cin, Ho, Wo, Cout, k, s, p, tr = Fz.wide_desc(tag)
    d = L.ConvDesc(B, H, W, Cin, Ho, Wo, Cout, k, k, s, p, tr, L.H16, 0, 0, Cin, 0, Cout, 0, 0)
    prev = l.hesic_conv2d_set_phase_fusion(Fz.WIDE[tag][6].get("pf", 1))
    try:
        v = (C.c_int32 * 4)(-1, -1, -1, -1)
        assert l.hesic_conv2d_variant(C.byref(d), v) == 0, l.hesic_last_error()
    finally:
        l.hesic_conv2d_set_phase_fusion(prev if prev in (0, 1, 2) else 1)
    assert tuple(v) == Fz.WIDE[tag][5]


def test_wide_table_covers_every_tile_and_option():
    plans = {c[5] for c in Fz.WIDE.values()}
    assert {p[0] for p in plans if p[3] == 1} == {32, 64, 128} and any(p[3] == 2 for p in plans)
    for bm in (32, 64, 128):
        rows = [c for c in Fz.WIDE.values() if c[5][0] == bm and c[5][3] == 1]
        assert any(not c[6].get("bias", True) for c in rows) and any(c[6].get("guard") for c in rows)
    for fam in (1, 2):
        assert any(c[6].get("cross") for c in Fz.WIDE.values() if c[5][3] == fam)
    # both ring depths of the 32-pixel tile (igemm_plan's rule, copied into the module) and of the larger ones
    assert Fz.wide_ring_is_deep("w_c192_t32") and Fz.wide_ring_is_deep("w_d192_t32") and not Fz.wide_ring_is_deep("w_c128_t32")
    assert Fz.wide_ring_is_deep("w_c32_t64") and not Fz.wide_ring_is_deep("w_c64_t64")
    tr4 = [t for t, c in Fz.WIDE.items() if c[5][3] == 2]
    assert all(Fz.WIDE[t][6].get("guard") or t == "w_d128_tr4h_r" for t in tr4)


def test_image_multi_trip_claims():
    for tag, trips in Fz.IMAGE_TRIPS.items():
        tiles, grid, per_trip = Fz.image_tiles(Fz.IMAGE[tag][0])
        assert grid == 256 and per_trip == 8 * 256
        assert 8 * 256 * (trips - 1) < tiles <= 8 * 256 * trips
    assert Fz.image_tiles(Fz.IMAGE["img_trips3"][0])[0] == 4200 and Fz.image_tiles(Fz.IMAGE["img_trips2"][0])[0] == 2208
    B, H, W = Fz.IMAGE["img_trips3"][0]
    assert 4200 % B == 0 and (4200 // B) % (8 * 256) != 0              # an image ends inside a trip, not at its boundary
    for tag, (shape, form, opt) in Fz.IMAGE.items():                     # the forms' layout rules
        assert (shape[2] % 2 == 0) == (form != "f32" or bool(opt.get("nhwc")))

"""tests/hilo_ref.py on the CPU (no GPU): for every case and format the fp64 evaluation with exactly the by-design roundings (``emulate``)
stays below C_BAR / 2 and passes the pair checks, and every applicable deliberate defect (``mutations_of``: an unwritten or late tile, a
dropped halo column, a lost lo product class, a dropped gamma'_lo or sq_lo term, swapped halves, a neighbour's or a zero lo half, the scale
applied behind the bias, |.| taken behind the split, a lost K slice) fails a check inside the pixels it touches, at every tile position it
is applied to.  Also: the case tables' claims about the launch plans (``hesic_conv2d_hilo_variant``: host logic) and the host splits."""
import ctypes as C

import pytest
import torch

import conv_grad_ref as G
import hilo_ref as Hz


def teardown_module():
    Hz.clear_cache()


def _emulation_and_mutations(case, R, flags=(), plan=None):
    out = Hz.emulate(R)
    res = Hz.check(R, out)
    for q, (ok, ratio, msg) in res.items():
        print(f"hilo_emulate {case} {q} {ratio:.4f}")
    for q, (ok, ratio, msg) in res.items():
        assert ok, f"{case} {msg}"
        if q in ("sum", "y32"):
            assert ratio < Hz.C_BAR / 2, f"{case} {q}: the emulation sits at {ratio:.3f} of the unit"
    n = len(Hz.tiles(R, R.get("plan")))
    for mut in Hz.mutations_of(R, flags):
        if mut == "tile_late" and n * (R["plan"][1] if R.get("plan") else 128) <= R["shape"][1]:
            continue                                      # one pixel tile
        for where in ([0] if mut == "drop_halo_col" else Hz.positions(n)):
            got, touched = Hz.mutate(R, out, mut, where)
            assert bool(touched.any()), f"{case} {mut} at {where}: nothing touched"
            if not bool(R["ref"][touched].any()):
                continue                                  # a tile of exact zeros (the zero corner): nothing to lose
            assert bool(Hz.outside(R, got, touched).any()), f"{case} {mut} at tile {where} of {n}: inside every bar"


IMAGE_CASES = [(t, f) for t in Hz.IMAGE for f in Hz.FORMATS]


@pytest.mark.parametrize("tag,fmt", IMAGE_CASES, ids=[f"{t}-{f}" for t, f in IMAGE_CASES])
def test_image_stage(tag, fmt):
    shape, o = Hz.IMAGE[tag]
    flags = tuple(k for k in ("loheavy", "dominant") if o.get(k) is not None)
    for form in o.get("forms", Hz.IMAGE_FORMS):
        for inverse in o.get("inverse", (False, True)):
            _emulation_and_mutations(f"{tag}_{fmt}_{form}_{Hz.NAMES[inverse]}", Hz.image_reference(tag, fmt, form, inverse), flags)


def test_image_trip_counts():
    import fused_gdn_ref as Fz
    for tag, trips in Hz.IMAGE_TRIPS.items():
        tiles, grid, per_trip = Fz.image_tiles(Hz.IMAGE[tag][0])
        assert per_trip * (trips - 1) < tiles <= per_trip * trips


WIDE_CASES = [(t, f) for t in Hz.WIDE for f in Hz.FORMATS]


@pytest.mark.parametrize("tag,fmt", WIDE_CASES, ids=[f"{t}-{f}" for t, f in WIDE_CASES])
def test_wide_stage(tag, fmt):
    o = Hz.WIDE[tag][5]
    flags = tuple(k for k in ("loheavy", "dominant") if o.get(k) is not None)
    for t, products, inverse in Hz.wide_runs():
        if t == tag:
            _emulation_and_mutations(f"{tag}_{fmt}_x{products}_{Hz.NAMES[inverse]}", Hz.wide_reference(tag, fmt, products, inverse), flags)


OUT_CASES = [(t, f) for t in Hz.HILO_OUT for f in Hz.FORMATS]


@pytest.mark.parametrize("tag,fmt", OUT_CASES, ids=[f"{t}-{f}" for t, f in OUT_CASES])
def test_hilo_out(tag, fmt):
    for inverse in (False, True):
        _emulation_and_mutations(f"{tag}_{fmt}_{Hz.NAMES[inverse]}", Hz.hilo_out_reference(tag, fmt, inverse))


@pytest.mark.parametrize("fmt", Hz.FORMATS)
@pytest.mark.parametrize("tag", list(Hz.IM2COL))
def test_im2col_route(tag, fmt):
    o = Hz.im2col_operands(tag, fmt)
    assert bool((o["ch"][:, 75:] == 0).all()) and bool((o["cl"][:, 75:] == 0).all())
    assert bool((o["ch"][:, 0, 0, 0] == 0).all())                        # tap (0, 0) of the first output pixel lies outside the image
    for inverse in (False, True):
        _emulation_and_mutations(f"{tag}_{fmt}_{Hz.NAMES[inverse]}", Hz.im2col_reference(tag, fmt, inverse))


PLAIN_CASES = Hz.plain_runs()


@pytest.mark.parametrize("tag,products,fmt", PLAIN_CASES, ids=[f"{t}-x{p}-{f}" for t, p, f in PLAIN_CASES])
def test_plain(tag, products, fmt):
    _emulation_and_mutations(f"{tag}_{fmt}_x{products}", Hz.plain_reference(tag, fmt, products))


@pytest.mark.parametrize("fmt", Hz.FORMATS)
@pytest.mark.parametrize("products", [3, 2])
def test_class_isolation(fmt, products):
    """Each product class at full magnitude: the lost-class defects leave the bar on the launch that isolates the class; the launches whose
    class the form does not have are exactly act(bias)."""
    for cls in Hz.ISO_CLASSES:
        R, _ = Hz.isolation_reference(fmt, products, cls)
        has = cls == "hh" or cls == "lh" or (cls == "hl" and products == 3)
        b = Hz.isolation_operands(fmt, products)["b"].double()
        if not has:
            assert bool((R["ref"] == b.view(1, -1)).all())
            continue
        out = Hz.emulate(R)
        for q, (ok, ratio, msg) in Hz.check(R, out).items():
            assert ok and (q not in ("sum", "y32") or ratio < Hz.C_BAR / 2), f"iso_{cls} {msg} {ratio}"
        mut = {"lh": "drop_xlo_whi", "hl": "drop_xhi_wlo"}.get(cls)
        if mut:
            assert mut in Hz.mutations_of(R, ("isolation",))
            n = len(Hz.tiles(R, R["plan"]))
            for where in Hz.positions(n):
                got, touched = Hz.mutate(R, out, mut, where)
                assert bool(Hz.outside(R, got, touched).any()), f"iso_{cls} {mut} at tile {where}: inside every bar"


# ------------------------------------------------------------------------------------------------------------------------ the plans
def _planned(l, L, cin, cout, k, s, shape, products, gdn):
    B, H, W = shape
    Ho, Wo = G.out_hw(H, W, k, s, k // 2, False)
    d = L.ConvDesc(B, H, W, cin, Ho, Wo, cout, k, k, s, k // 2, 0, L.H16, 0, 0, (1 if products == 1 else 2) * cin, 0, 2 * cout, 0, 0)
    v = (C.c_int * 4)()
    assert l.hesic_conv2d_hilo_variant(C.byref(d), products, gdn, v) == 0, l.hesic_last_error()
    return tuple(v)


@pytest.mark.parametrize("fmt", Hz.FORMATS)
def test_planned_tiles(fmt):
    """The tiles the case tables name are what igemm_plan answers for the pair options, in both libraries (host arithmetic, no GPU)."""
    from hesic_amd import _lib as L
    l = L.lib(Hz.FMT[fmt]["dtype"])
    for tag, products, inverse in Hz.wide_runs():
        cin, k, s, shape, _, _ = Hz.WIDE[tag]
        assert _planned(l, L, cin, 128, k, s, shape, products, 4 if inverse else 3)[:3] == Hz.wide_plan(tag, products, inverse), (tag, products, inverse)
    for tag, inverse in Hz.hilo_out_runs():
        cin, k, s, shape, plan, _ = Hz.HILO_OUT[tag]
        assert _planned(l, L, cin, 128, k, s, shape, 1, 4 if inverse else 3)[:3] == plan, (tag, inverse)
    for tag, products, f in Hz.plain_runs():
        cin, cout, k, s, shape, plan, _ = Hz.PLAIN[tag]
        assert _planned(l, L, cin, cout, k, s, shape, products, 0) == plan, (tag, products)
    for tag, ((B, H, W), _) in Hz.IM2COL.items():
        Ho, Wo = G.out_hw(H, W, 5, 2, 2, False)
        assert _planned(l, L, Hz.KP, 128, 1, 1, (B, Ho, Wo), 3, 3)[:3] == Hz.IM2COL_PLAN, tag
    cin, cout, k, s, shape = Hz.ISOLATION
    assert _planned(l, L, cin, cout, k, s, shape, 3, 0)[:3] == (128, 128, 64)
    assert {Hz.wide_plan(*r)[0] for r in Hz.wide_runs()} == {32, 64, 128, 256}
    assert 64 in {row[5][1] for row in Hz.PLAIN.values()} and any(row[5][3] > 1 for row in Hz.PLAIN.values())


def test_plan_query_refuses_bad_arguments():
    from hesic_amd import _lib as L
    l = L.lib()
    d = L.ConvDesc(1, 8, 8, 32, 4, 4, 128, 3, 3, 2, 1, 0, L.H16, 0, 0, 64, 0, 256, 0, 0)
    v = (C.c_int * 4)()
    for products, gdn in ((0, 3), (4, 0), (3, 1), (3, 2), (1, 0)):
        assert l.hesic_conv2d_hilo_variant(C.byref(d), products, gdn, v) != 0
    assert l.hesic_conv2d_hilo_variant(None, 3, 3, v) != 0 and l.hesic_conv2d_hilo_variant(C.byref(d), 3, 3, None) != 0


# ------------------------------------------------------------------------------------------------------------------------ the host splits
@pytest.mark.parametrize("fmt", Hz.FORMATS)
def test_split_and_walk(fmt):
    t = G.synthetic._uniform("hlp.split", (4096,), -3, 3)
    hi, lo = Hz.split(t, fmt)
    u = Hz.FMT[fmt]["u"]
    assert bool((lo.double().abs() <= 0.5 * Hz.ulp16(hi, fmt)).all())
    assert bool(((hi.double() + lo.double() - t.double()).abs() <= u * u * t.double().abs() + Hz.FMT[fmt]["h"]).all())
    if fmt == "f16":
        hi, lo = Hz.split(torch.tensor([1e6, -1e6]), fmt)
        assert hi.tolist() == [65504.0, -65504.0] and lo.tolist() == [0.0, 0.0]
    w = G.synthetic._uniform("hlp.walk", (8, 3, 5, 5), -0.2, 0.2)
    q = Hz.shaped_walk(w, fmt)
    assert bool((q == Hz.rnd16(q, fmt)).all()) and not bool((q == Hz.rnd16(w, fmt)).all())
    # error feedback: the sum over the taps is kept to the last tap's rounding, plain rounding only to sqrt(25) of them
    assert float((q.double().sum((2, 3)) - w.double().sum((2, 3))).abs().max()) <= u * float(w.abs().max()) * 1.01
    w16 = Hz.rnd16(w, fmt)
    assert bool((Hz.shaped_walk(w16, fmt) == w16).all())

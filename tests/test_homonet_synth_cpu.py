"""Synthetic-warp pairs for HomographyNet, the parts that need no GPU: the descriptor layout and the C ABI of
include/hesic_homonet_synth.h, the host checks of ``functional.check_homonet_synth_items``, ``homography.draw_deltas``, the restatement
tests/homonet_synth_ref.py against ``homography_train_ref.warp_torch``, the conditions the GPU test's cases are chosen for, and the new
options of ``python -m hesic_amd.homography_train`` / ``homography_eval``."""
import ctypes as C
import random
import re
import subprocess

import numpy as np
import pytest
import torch

import homography_train_ref as HT
import homonet_synth_ref as SR
from hesic_amd import _lib as L
from hesic_amd import functional as Fn
from hesic_amd import homography, homography_eval, homography_train
from hesic_amd.compressai.datasets import MEAN, STD

FIELDS = ("view", "pitch_px", "rows", "x0", "y0", "cw", "ch", "wx", "wy", "delta")


# ------------------------------------------------------------------------------------------------------------------------ ABI
def test_item_dtype_is_the_headers_struct():
    dt = np.dtype(Fn.HOMONET_SYNTH_ITEM_DTYPE)
    assert dt.itemsize == 72 and dt.names == FIELDS
    assert [dt.fields[n][1] for n in FIELDS] == [0] + [8 + 4 * i for i in range(9)]
    assert dt.fields["view"][0] == np.dtype("<u8") and dt.fields["delta"][0] == np.dtype(("<i4", (8,)))
    assert C.sizeof(L.HomonetSynthItem) == 72 and [(n, getattr(L.HomonetSynthItem, n).offset) for n, _ in L.HomonetSynthItem._fields_] == \
        [(n, dt.fields[n][1]) for n in FIELDS]
    text = re.sub(r"/\*.*?\*/", "", open(L.header_path("hesic_homonet_synth.h")).read(), flags=re.S)
    body = re.search(r"typedef struct \{(.*?)\} hesic_homonet_synth_item;", text, flags=re.S).group(1)
    assert tuple(re.findall(r"\b([a-z_0-9]+)(?:\[8\])?\s*[,;]", body)) == FIELDS
    assert body.count("const uint8_t*") == 1 and "int32_t delta[8]" in body
    items = Fn.homonet_synth_items(3)
    assert items.shape == (3,) and items.dtype == dt and not items.view(np.uint8).any()


@pytest.mark.parametrize("fmt", ["bf16", "f16"])
def test_abi_header_bindings_exports(fmt):
    declared = L.declared_symbols("hesic_homonet_synth.h")
    assert declared == ["hesic_homonet_synth_items"] and set(declared) == set(L._HOMONET_SYNTH_SIGS)
    assert "hesic_homonet_synth" not in open(L.header_path("hesic_hip.h")).read()                  # hesic_hip.h does not include it
    exported = subprocess.check_output(["nm", "-D", "--defined-only", L.LIB_PATH_F16 if fmt == "f16" else L.LIB_PATH], text=True)
    assert " T hesic_homonet_synth_items\n" in exported


OUTS = ("grey_a", "patch_a", "corners", "delta", "h", "grey_b", "patch_b")


@pytest.mark.parametrize("bad, word", [
    (dict(items=None), "null"), (dict(h=None), "null"), (dict(patch_b=None), "null"), (dict(B=0), "shape"), (dict(B=65536), "shape"),
    (dict(S=0), "P <= S"), (dict(P=0), "P <= S"), (dict(P=9), "P <= S"), (dict(S=16385), "P <= S"),
    (dict(std=0.0), "std"), (dict(std=float("nan")), "std"), (dict(mean=float("nan")), "std"), (dict(items=4), "misaligned"),
    (dict(h=4), "misaligned"), (dict(grey_b=2), "misaligned"),
], ids=lambda v: "-".join(f"{k}" for k in v) if isinstance(v, dict) else None)
def test_bad_arguments_return_einval_with_a_message(bad, word):
    """Host dummies for pointers: every case is refused before anything is launched or dereferenced.  An integer moves that pointer by so
    many bytes off its 8-byte alignment."""
    lib = L.lib()
    buf = (C.c_double * 16)()
    a = dict(items=0, B=1, S=8, P=4, mean=0.5, std=0.25, **{k: 0 for k in OUTS})
    a.update(bad)
    ptr = {k: None if a[k] is None else C.c_void_p(C.addressof(buf) + a[k]) for k in ("items",) + OUTS}
    assert lib.hesic_homonet_synth_items(ptr["items"], a["B"], a["S"], a["P"], a["mean"], a["std"], 1, *[ptr[k] for k in OUTS], None) == -1
    msg = lib.hesic_last_error().decode()
    assert msg.startswith("homonet_synth_items:") and word in msg, msg


# ---------------------------------------------------------------------------------------------------------------- host checks
def _good_items():
    """Three items that satisfy the contract for S = 16, P = 8 (the pointers are never followed on the host)."""
    items = Fn.homonet_synth_items(3)
    rows = [(17, 13, 0, 0, 17, 13, 0, 0, [0] * 8), (20, 32, 3, 5, 17, 27, 8, 8, [-3, 2, 3, -3, 1, 2, -2, 3]),
            (40, 9, 39, 8, 1, 1, 4, 0, [3, 3, -4, 3, -4, -4, 3, -4])]
    for b, (pitch, nrows, x0, y0, cw, ch, wx, wy, delta) in enumerate(rows):
        items[b] = (4096, pitch, nrows, x0, y0, cw, ch, wx, wy, delta)
    return items


def test_check_homonet_synth_items_accepts_the_contracts_edges():
    Fn.check_homonet_synth_items(_good_items(), 16, 8)


@pytest.mark.parametrize("b, change, word", [
    (1, dict(x0=4), "columns"), (1, dict(y0=6), "rows"), (2, dict(cw=0), "crop"), (0, dict(ch=0), "crop"), (1, dict(wx=9), "window"),
    (2, dict(wy=9), "window"), (0, dict(wx=-1), "window"), (2, dict(x0=-1), "columns"), (1, dict(view=0), "null"),
    (2, dict(delta=[0, 0, -5, 4, -3, -5, 0, 0]), "convex"),         # corner 1 pushed inside the triangle of the others: a reflex vertex
    (0, dict(delta=[0, 0, -4, 4, 0, 0, 0, 0]), "convex"),           # corner 1 onto the diagonal 0 - 2 ... (4, 4): a collinear triple
    (1, dict(delta=[9, 0, -9, 0, 0, 0, 0, 0]), "convex"),           # the top edge reversed: a self-intersecting quadrilateral
])
def test_check_homonet_synth_items_names_the_item(b, change, word):
    items = _good_items()
    for k, v in change.items():
        items[b][k] = v
    with pytest.raises(ValueError, match=rf"item {b} .*{word}|item {b} {word}"):
        Fn.check_homonet_synth_items(items, 16, 8)
    launches = []
    with L.call_hook(lambda name, args: launches.append(name)):
        with pytest.raises(ValueError, match=f"item {b} "):
            Fn.homonet_synth(items, 16, 8, 0.5, 0.25, True)          # refused on the host, before the device is asked for
    assert launches == []


def test_convexity_is_exact_integer_arithmetic():
    assert Fn.perturbed_quad_is_convex(0, 0, 8, [0] * 8)
    assert not Fn.perturbed_quad_is_convex(0, 0, 8, [0, 0, -4, 4, 0, 0, 0, 0])        # (0,0), (4,4), (8,8): cross product exactly 0
    big = 2 ** 40                                                                      # no float would keep these cross products apart
    assert Fn.perturbed_quad_is_convex(big, big, 8, [0, 0, 0, 0, 0, 0, 0, 0])
    assert not Fn.perturbed_quad_is_convex(big, big, 8, [0, 0, -4, 4, 0, 0, 0, 0])
    assert Fn.perturbed_quad_is_convex(big, big, 8, [0, 0, -4, 3, 0, 0, 0, 0])


def test_homonet_synth_argument_errors():
    with pytest.raises(ValueError, match="HOMONET_SYNTH_ITEM_DTYPE"):
        Fn.homonet_synth(Fn.homonet_items(2), 16, 8, 0.5, 0.25, True)
    with pytest.raises(ValueError, match=r"\(B, 72\)"):
        Fn.homonet_synth(torch.zeros(2, 48, dtype=torch.uint8), 16, 8, 0.5, 0.25, True)
    with pytest.raises(ValueError, match="P <= S"):
        Fn.homonet_synth(_good_items(), 8, 16, 0.5, 0.25, True)
    with pytest.raises(ValueError, match="B <= 65535"):
        Fn.homonet_synth(Fn.homonet_synth_items(0), 16, 8, 0.5, 0.25, True)


# ----------------------------------------------------------------------------------------------------------------- draw_deltas
class _Script:
    """A scripted ``rng``: ``randrange`` hands out the listed numbers in order and records its calls; any other method is an error."""

    def __init__(self, values):
        self.values, self.calls = list(values), []

    def randrange(self, a, b):
        self.calls.append((a, b))
        return self.values.pop(0)


def test_draw_deltas_order_and_count():
    script = _Script(range(1, 17))
    got = homography.draw_deltas(2, [(20, 20), (30, 40)], 64, 24, script)
    assert got == [list(range(1, 9)), list(range(9, 17))]              # corner 0 x, corner 0 y, ... corner 3 y; eight per item
    assert script.calls == [(-24, 24)] * 16 and script.values == []
    # the (B,4,2) corners are accepted as well; the first corner is the origin
    corners = torch.tensor([[[20, 20], [84, 20], [84, 84], [20, 84]], [[30, 40], [94, 40], [94, 104], [30, 104]]], dtype=torch.float32)
    assert homography.draw_deltas(2, corners, 64, 24, _Script(range(1, 17))) == got
    # a real stream: the values are randrange's, in that order, and every value is in [-rho, rho)
    a, b = random.Random(5), random.Random(5)
    got = homography.draw_deltas(3, [(45, 45)] * 3, 128, 45, a)
    assert got == [[b.randrange(-45, 45) for _ in range(8)] for _ in range(3)] and a.getstate() == b.getstate()
    assert all(-45 <= v < 45 for d in got for v in d)


def test_draw_deltas_redraws_a_non_convex_draw():
    bad = [0, 0, -5, 4, -3, -5, 0, 0]                    # not convex for an 8 x 8 window (the host check's case)
    good = [1, -1, 2, 0, -2, 1, 0, 3]
    script = _Script(bad + good + good)
    assert not Fn.perturbed_quad_is_convex(4, 0, 8, bad) and Fn.perturbed_quad_is_convex(4, 0, 8, good)
    assert homography.draw_deltas(2, [(4, 0), (4, 0)], 8, 6, script) == [good, good]
    assert len(script.calls) == 24 and script.values == []              # all eight are drawn again, and only for the item that needed it


def test_draw_deltas_rho_zero_touches_nothing():
    assert homography.draw_deltas(3, [(0, 0)] * 3, 8, 0, None) == [[0] * 8] * 3
    with pytest.raises(ValueError, match="rho"):
        homography.draw_deltas(1, [(0, 0)], 8, -1, random.Random(0))
    with pytest.raises(ValueError, match="windows"):
        homography.draw_deltas(2, [(0, 0)], 8, 2, random.Random(0))


# ------------------------------------------------------------------------------------------------------------- the restatement
@pytest.mark.parametrize("align", [True, False], ids=["align1", "align0"])
@pytest.mark.parametrize("rho", SR.RHOS)
def test_restated_warp_against_grid_sample(rho, align):
    """The header's fp64 sum against ``homography_train_ref.warp_torch`` (grid_sample) in fp64, before the rounding to fp32: 1e-12."""
    geometry, deltas = SR.case(rho)
    grey_a, _, corners, delta, h, grey_b, _ = SR.synth_items(SR.stored_views(), geometry, deltas, SR.S, SR.P, float(MEAN), float(STD), align)
    want = HT.warp_torch(torch.from_numpy(grey_a).double(), torch.from_numpy(h).view(-1, 3, 3), (SR.S, SR.S), align).numpy()
    exact = SR.warp(grey_a, h, align, dtype=np.float64)
    worst = float(np.abs(exact - want).max())
    print(f"homonet_synth restatement rho{rho} align{int(align)}: max |fp64 sum - fp64 grid_sample| {worst:.3e}")
    assert worst <= 1e-12
    assert grey_b.dtype == np.float32 and np.array_equal(exact.astype(np.float32), grey_b)            # the one rounding


def test_the_cases_are_what_they_are_for():
    """rho = 2 keeps the windows in [2, 6]; rho = 5 puts them at (0, 0) and at least one ``patch_b`` element of some item comes from a
    sample with a tap outside the frame; the deltas are not all zero, and the photometric loss with ``delta = 0`` -- here the mean
    |patch_a - patch_b| of the restatement -- is at least 1000 x 2^-21 for both conventions."""
    for rho in SR.RHOS:
        geometry, deltas = SR.case(rho)
        windows = [g[4:] for g in geometry]
        assert all(-rho <= v < rho for d in deltas for v in d) and any(v for d in deltas for v in d)
        assert all(Fn.perturbed_quad_is_convex(wx, wy, SR.P, d) for (wx, wy), d in zip(windows, deltas))
        if rho == 2:
            assert all(2 <= w <= 6 for xy in windows for w in xy)
        else:
            assert windows == [(0, 0)] * 4 and any(v < 0 for d in deltas for v in d)
        for align in (True, False):
            grey_a, patch_a, _, _, h, _, patch_b = SR.synth_items(SR.stored_views(), geometry, deltas, SR.S, SR.P, float(MEAN), float(STD), align)
            _, outside = SR.warp(grey_a, h, align, with_outside=True)
            in_patch = [bool(outside[b, 0, wy:wy + SR.P, wx:wx + SR.P].any()) for b, (wx, wy) in enumerate(windows)]
            zero_loss = float(np.abs(patch_a.astype(np.float64) - patch_b).mean())
            print(f"homonet_synth case rho{rho} align{int(align)}: items with an outside tap in patch_b {in_patch}, loss at delta = 0 {zero_loss:.4f}")
            assert zero_loss >= 1000 * 2.0 ** -21
            if rho == 5:
                assert any(in_patch)
    # the residual of dlt_torch's own solution, the yardstick of the GPU test's bar on h
    res = max(float(SR.corner_residual(SR.dlt(*_corners_delta(rho)), *_corners_delta(rho)).max()) for rho in SR.RHOS)
    print(f"homonet_synth dlt_torch corner residual over the cases {res:.3e} px")
    assert res < 1e-9


def _corners_delta(rho):
    geometry, deltas = SR.case(rho)
    corners = np.array([[[x, y], [x + SR.P, y], [x + SR.P, y + SR.P], [x, y + SR.P]] for _, _, _, _, x, y in geometry], dtype=np.float64)
    return corners, np.asarray(deltas, dtype=np.float64).reshape(-1, 4, 2)


# ------------------------------------------------------------------------------------------------------------------ the command
def test_synthetic_epoch_has_the_photometric_runs_plan():
    """``draw_batch`` on the epoch's stream and ``draw_deltas`` on the deltas' own stream: the batches, crops and windows are those of a
    photometric run, whose stream ends in the same state."""
    pairs = [(f"l{i}", f"r{i}", (40 + i % 3, 30 + i % 2)) for i in range(10)]
    runs = []
    for synthetic in (False, True):
        rng, srng = random.Random("3/1"), random.Random("3/1/synth")
        plan = []
        for items in homography_train.batches(pairs, 4, (20, 24), rng, True, True):
            origins, sizes, windows = homography_train.draw_batch(items, (20, 24), rng, 64, 32, 8)
            if synthetic:
                deltas = homography.draw_deltas(len(items), windows, 32, 8, srng)
                assert len(deltas) == len(items)
            plan.append((items, origins, sizes, windows))
        runs.append((plan, rng.getstate()))
    assert runs[0] == runs[1]


def test_parser_supervision(tmp_path, capsys):
    assert homography_train.parser().parse_args(["root"]).supervision == "photometric"
    assert homography_train.parser().parse_args(["root", "--supervision", "synthetic", "--cache", "device"]).supervision == "synthetic"
    for argv in (["--supervision", "synthetic"], ["--supervision", "synthetic", "--cache", "host"], ["--supervision", "labels"]):
        with pytest.raises(SystemExit) as e:
            homography_train.main([str(tmp_path)] + argv)
        assert e.value.code == 2
    assert "--supervision synthetic needs --cache device" in capsys.readouterr().err


def test_eval_without_a_device_returns_2(tmp_path, capsys, monkeypatch):
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    assert homography_eval.main([str(tmp_path), "--checkpoint", "synthetic"]) == 2
    assert "needs a ROCm device" in capsys.readouterr().err
    with pytest.raises(SystemExit):
        homography_eval.main([str(tmp_path)])                        # --checkpoint is required

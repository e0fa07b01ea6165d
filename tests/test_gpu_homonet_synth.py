"""Synthetic-warp pairs for HomographyNet on the GPU (include/hesic_homonet_synth.h, functional.homonet_synth,
pair_cache.DevicePairCache.homonet_synth_batch).  ``grey_a``, ``patch_a`` and ``corners`` are held to the bits of
``functional.homonet_prepare_items``, ``h`` to the corner residual of ``dlt_torch``'s own fp64 solution, and ``grey_b`` / ``patch_b`` to the
BITS of tests/homonet_synth_ref.py fed with the kernel's own ``h``.  The batch is that of tests/test_gpu_homonet_items.py (shapes, stored
sizes, crops) with windows and deltas drawn for rho = 2 and rho = 5 (homonet_synth_ref.case)."""
import functools
import random

import numpy as np
import pytest
import torch

import homonet_synth_ref as SR
import memguard
from hesic_amd import functional as Fn
from hesic_amd import codec, geometry, homography, pair_cache, synthetic
from hesic_amd.compressai.datasets import MEAN, STD

pytestmark = pytest.mark.gpu
DEV = "cuda"
S, P = SR.S, SR.P
NAMES = SR.NAMES
ALIGNS = [True, False]


@functools.lru_cache(maxsize=None)
def _views():
    return SR.stored_views()


def _outside(geo, value, img):
    """``img`` with every byte outside the crop rectangle set to ``value``."""
    x0, y0, cw, ch = geo[:4]
    out = np.full(img.shape, value, dtype=np.uint8)
    out[y0:y0 + ch, x0:x0 + cw] = img[y0:y0 + ch, x0:x0 + cw]
    return out


def _shapes(B):
    return [(B, 1, S, S), (B, 1, P, P), (B, 4, 2), (B, 4, 2), (B, 9), (B, 1, S, S), (B, 1, P, P)]


def _items(stored, geometry_, deltas, order, fill=memguard.NAN_FILL):
    """Guarded device copies of the stored views of ``order``'s items and their descriptors."""
    views, items = [], Fn.homonet_synth_items(len(order))
    for b, i in enumerate(order):
        t = memguard.guarded(torch.from_numpy(stored[i]).to(DEV), fill=fill, name=f"view{i}")
        assert t.is_contiguous()
        views.append(t)
        x0, y0, cw, ch, wx, wy = geometry_[i]
        items[b] = (t.data_ptr(), stored[i].shape[1], stored[i].shape[0], x0, y0, cw, ch, wx, wy, deltas[i])
    return views, items


def _run(rho, align, outside=None, fill=memguard.NAN_FILL, order=None):
    """functional.homonet_synth on guarded stored views (bytes outside the crops optionally overwritten) into guarded, NaN-filled ``out=``
    tensors; every guard is checked, and the tensors returned are the ones passed.  Returns numpy copies of the seven outputs."""
    geometry_, deltas = SR.case(rho)
    order = list(range(len(geometry_))) if order is None else list(order)
    stored = _views() if outside is None else [_outside(g, outside, v) for g, v in zip(geometry_, _views())]
    views, items = _items(stored, geometry_, deltas, order, fill)
    outs = [memguard.guarded(torch.full(s, float("nan"), dtype=torch.float64 if n == "h" else torch.float32, device=DEV), name=n)
            for n, s in zip(NAMES, _shapes(len(order)))]
    got = Fn.homonet_synth(items, S, P, float(MEAN), float(STD), align, out=outs)
    torch.cuda.synchronize()
    memguard.check_all(views + outs)
    assert all(g is o for g, o in zip(got, outs))
    return [t.cpu().numpy() for t in got]


@functools.lru_cache(maxsize=None)
def _base(rho, align):
    """The plain run of a case, computed once and shared; nothing mutates it."""
    return _run(rho, align)


def _same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.view(np.int64 if a.dtype == np.float64 else np.int32),
                                                                        b.view(np.int64 if b.dtype == np.float64 else np.int32))


def _assert_bits(tag, got, want):
    for name, g, w in zip(NAMES, got, want):
        assert _same_bits(g, w), (tag, name, int((g != w).sum()))


@pytest.mark.parametrize("rho", SR.RHOS)
def test_first_view_is_the_item_entrys(rho):
    """grey_a, patch_a, corners: ``torch.equal`` to homonet_prepare_items' grey1, patch1, corners for the same items; delta: the integers."""
    geometry_, deltas = SR.case(rho)
    got = _base(rho, True)
    items = Fn.homonet_items(len(geometry_))
    views = [torch.from_numpy(v).to(DEV) for v in _views()]
    for b, (v, (x0, y0, cw, ch, wx, wy)) in enumerate(zip(views, geometry_)):
        items[b] = (v.data_ptr(), v.data_ptr(), v.shape[1], v.shape[0], x0, y0, cw, ch, wx, wy)
    grey1, _, patch1, _, corners = Fn.homonet_prepare_items(items, S, P, float(MEAN), float(STD))
    for name, g, w in (("grey_a", got[0], grey1), ("patch_a", got[1], patch1), ("corners", got[2], corners)):
        assert torch.equal(torch.from_numpy(g), w.cpu()), name
    assert got[3].dtype == np.float32 and np.array_equal(got[3], np.asarray(deltas, dtype=np.float32).reshape(-1, 4, 2))
    _assert_bits("align0_first_view", _base(rho, False)[:5], got[:5])                  # the convention touches grey_b and patch_b only


def test_h_maps_the_corners_onto_the_perturbed_corners():
    """``h`` applied in fp64 numpy to the four corners gives corners + delta within 2^10 x the largest such residual of ``dlt_torch``'s own
    fp64 solution over these cases (the elimination orders differ; the conditioning at coordinates <= 16 is mild), floor 1e-12 px.
    Measured: dlt_torch 1.2e-14 px (1.1e-14 with another LAPACK), so the bar is 1.3e-11 px; the kernel's h: 2.0e-15 px."""
    ref = max(float(SR.corner_residual(SR.dlt(c, d), c, d).max()) for c, d in (_base(rho, True)[2:4] for rho in SR.RHOS))
    bar = max(1e-12, 2.0 ** 10 * ref)
    for rho in SR.RHOS:
        _, _, corners, delta, h, _, _ = _base(rho, True)
        assert h.dtype == np.float64 and np.isfinite(h).all() and (h[:, 8] == 1.0).all()
        res = SR.corner_residual(h, corners, delta)
        print(f"homonet_synth h rho{rho}: corner residual {res.max():.3e} px, dlt_torch {ref:.3e} px, bar {bar:.3e} px")
        assert (res <= bar).all(), (rho, res, bar)


@pytest.mark.parametrize("align", ALIGNS, ids=["align1", "align0"])
@pytest.mark.parametrize("rho", SR.RHOS)
def test_warp_has_the_bits_of_the_restatement(rho, align):
    """grey_b and patch_b: the restatement fed with the kernel's OWN h bits, bit for bit; in the rho = 5 set at least one patch_b element
    comes from a sample with a tap outside the frame (asserted on the restatement)."""
    geometry_, deltas = SR.case(rho)
    got = _base(rho, align)
    want = SR.synth_items(_views(), geometry_, deltas, S, P, float(MEAN), float(STD), align, h=got[4])
    for k in (5, 6):
        nbad = int((got[k].view(np.int32) != want[k].view(np.int32)).sum())
        print(f"homonet_synth rho{rho} align{int(align)} {NAMES[k]} elements that differ in bits: {nbad} of {got[k].size}, "
              f"max |difference| {np.abs(got[k].astype(np.float64) - want[k]).max():.3e}")
        assert nbad == 0, NAMES[k]
    _, outside = SR.warp(got[0], got[4], align, with_outside=True)
    in_patch = [bool(outside[b, 0, wy:wy + P, wx:wx + P].any()) for b, (_, _, _, _, wx, wy) in enumerate(geometry_)]
    if rho == 5:
        assert any(in_patch)
        assert (got[5] == 0).any()                      # and whole samples outside the frame: the zero padding


@pytest.mark.parametrize("rho", SR.RHOS)
def test_consistent_with_the_photometric_loss(rho):
    """The loss the net is trained on afterwards: at the true delta it is at most 2^-21 (twice the two fp32 roundings involved), at
    delta = 0 at least 1000 times that -- the sampling convention and the direction of h."""
    outs = [torch.from_numpy(t).to(DEV) for t in _base(rho, geometry.DEFAULT_ALIGN_CORNERS)]
    grey_a, _, corners, delta, _, _, patch_b = outs
    true = float(homography.photometric_loss(delta, grey_a, patch_b, corners))
    zero = float(homography.photometric_loss(torch.zeros_like(delta), grey_a, patch_b, corners))
    print(f"homonet_synth photometric rho{rho}: loss at the true delta {true:.3e} (bar {2.0 ** -21:.3e}), at delta = 0 {zero:.4f}")
    assert true <= 2.0 ** -21
    assert zero >= 1000 * 2.0 ** -21


@pytest.mark.parametrize("rho", SR.RHOS)
def test_nothing_outside_the_crop_is_read(rho):
    """Every byte outside the crop rectangles -- the rest of the stored images and the guards around them; item 2's crop ends at the last
    byte of its image -- takes two different values: the same bits as the plain run, and intact guards (checked in ``_run``)."""
    x0, y0, cw, ch = SR.CROPS[2]
    assert (y0 + ch, x0 + cw) == SR.STORED[2]
    want = _base(rho, True)
    _assert_bits("outside_00", _run(rho, True, outside=0x00, fill=0xFF), want)
    _assert_bits("outside_ff", _run(rho, True, outside=0xFF, fill=0x00), want)


def test_every_output_element_is_written_and_out_is_returned():
    for rho in SR.RHOS:
        for align in ALIGNS:
            for name, g in zip(NAMES, _base(rho, align)):                # NaN-filled out= tensors, returned as passed (asserted in _run)
                assert np.isfinite(g).all(), (rho, align, name)
    with pytest.raises(ValueError, match="out must be"):
        Fn.homonet_synth(_items(_views(), *SR.case(2), [0])[1], S, P, float(MEAN), float(STD), True,
                         out=[torch.empty(s, device=DEV) for s in _shapes(1)])                      # h must be fp64


@pytest.mark.parametrize("rho", SR.RHOS)
def test_items_are_independent_of_batch_and_position(rho):
    want = _base(rho, False)
    for i in range(len(SR.CROPS)):
        _assert_bits(f"alone{i}", _run(rho, False, order=[i]), [w[i:i + 1] for w in want])
    order = [3, 1, 1, 0, 2, 3, 0]
    _assert_bits("reordered", _run(rho, False, order=order), [w[order] for w in want])


def test_runs_and_graph_replays_repeat_their_bits():
    want = _base(5, True)
    _assert_bits("second_run", _run(5, True), want)
    geometry_, deltas = SR.case(5)
    views, items = _items(_views(), geometry_, deltas, range(len(geometry_)))
    items_dev = torch.from_numpy(items.view(np.uint8).reshape(len(items), 72)).to(DEV)
    outs = [torch.full(s, float("nan"), dtype=torch.float64 if n == "h" else torch.float32, device=DEV) for n, s in zip(NAMES, _shapes(len(items)))]
    from hesic_amd import _lib as L

    def launch():
        L.call("hesic_homonet_synth_items", L.ptr(items_dev), len(items), S, P, float(MEAN), float(STD), 1, *[L.ptr(t) for t in outs], L.stream())
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        launch()                                        # warm: the code object is loaded outside the capture
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        launch()
    for t in outs:
        t.fill_(float("nan"))
    graph.replay()
    torch.cuda.synchronize()
    _assert_bits("graph_replay", [t.cpu().numpy() for t in outs], want)


# ----------------------------------------------------------------------------------------------------------------- the cache
@pytest.mark.parametrize("view", ["left", "right"])
def test_cache_synth_batch_device_equals_stream_and_the_restatement(tmp_path, view):
    from PIL import Image
    x1, x2, _ = synthetic.stereo_batch(10, 3, 24, 40)
    stored = {}
    for side, x in (("left", x1), ("right", x2)):
        d = tmp_path / "train" / side
        d.mkdir(parents=True)
        stored[side] = list(codec.quantise(x))
        for i, img in enumerate(stored[side]):
            Image.fromarray(img).save(d / f"pair{i:02d}.png")
    indices, windows = [2, 0, 1, 2], [(0, 0), (8, 8), (1, 7), (4, 4)]
    origins, sizes = [(9, 5), (0, 0), (3, 17), (0, 2)], [(14, 16), (24, 40), (16, 23), (5, 19)]
    deltas = homography.draw_deltas(4, windows, P, 3, random.Random(4))
    got = {}
    for mode in ("device", "stream"):
        cache = pair_cache.DevicePairCache(tmp_path, "train", mode=mode, workers=2)
        got[mode] = [t.cpu().numpy() for t in cache.homonet_synth_batch(indices, origins, sizes, windows, deltas, S, P, view=view)]
        if mode == "stream":
            assert cache._slab.numel() == sum(ch * cw * 3 for ch, cw in sizes)          # only the one view's crops are uploaded
    _assert_bits("device_vs_stream", got["device"], got["stream"])
    geo = [(x0, y0, cw, ch) + w for (y0, x0), (ch, cw), w in zip(origins, sizes, windows)]
    want = SR.synth_items([stored[view][i] for i in indices], geo, deltas, S, P, float(MEAN), float(STD), geometry.DEFAULT_ALIGN_CORNERS,
                          h=got["device"][4])
    _assert_bits("cache_vs_restatement", got["device"], want)
    with pytest.raises(ValueError, match="view"):
        cache.homonet_synth_batch(indices, origins, sizes, windows, deltas, S, P, view="both")
    with pytest.raises(ValueError, match="deltas"):
        cache.homonet_synth_batch(indices, origins, sizes, windows, deltas[:3], S, P)

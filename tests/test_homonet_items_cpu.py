"""HomographyNet's inputs from stored uint8 images, the parts that need no GPU: the descriptor layout and the C ABI of
include/hesic_homonet_items.h, the host checks of ``functional.check_homonet_items``, ``homography_train.draw_batch`` against the draws of
the host route (``load_batch`` + ``homography.window_origins``), and the new options of ``python -m hesic_amd.homography_train``."""
import ctypes as C
import random
import re
import subprocess

import numpy as np
import pytest
import torch

from hesic_amd import _lib as L
from hesic_amd import functional as Fn
from hesic_amd import homography, homography_train

FIELDS = ("left", "right", "pitch_px", "rows", "x0", "y0", "cw", "ch", "wx", "wy")


# ------------------------------------------------------------------------------------------------------------------------ ABI
def test_item_dtype_is_the_headers_struct():
    dt = np.dtype(Fn.HOMONET_ITEM_DTYPE)
    assert dt.itemsize == 48 and dt.names == FIELDS
    assert [dt.fields[n][1] for n in FIELDS] == [0, 8] + [16 + 4 * i for i in range(8)]
    assert [dt.fields[n][0] for n in FIELDS] == [np.dtype("<u8")] * 2 + [np.dtype("<i4")] * 8
    assert C.sizeof(L.HomonetItem) == 48 and [(n, getattr(L.HomonetItem, n).offset) for n, _ in L.HomonetItem._fields_] == \
        [(n, dt.fields[n][1]) for n in FIELDS]
    # the struct as the header spells it: two pointers, then the eight int32 in this order
    text = re.sub(r"/\*.*?\*/", "", open(L.header_path("hesic_homonet_items.h")).read(), flags=re.S)
    body = re.search(r"typedef struct \{(.*?)\} hesic_homonet_item;", text, flags=re.S).group(1)
    assert tuple(re.findall(r"\b([a-z_0-9]+)\s*[,;]", body)) == FIELDS
    assert body.count("const uint8_t*") == 2 and body.count("int32_t") == 4
    items = Fn.homonet_items(3)
    assert items.shape == (3,) and items.dtype == dt and not items.view(np.uint8).any()


@pytest.mark.parametrize("fmt", ["bf16", "f16"])
def test_abi_header_bindings_exports(fmt):
    declared = L.declared_symbols("hesic_homonet_items.h")
    assert declared == ["hesic_homonet_prepare_items"] and set(declared) == set(L._HOMONET_ITEMS_SIGS)
    assert '#include "hesic_homonet_items.h"' in open(L.header_path("hesic_homography_prep.h")).read()       # one include serves both forms
    exported = subprocess.check_output(["nm", "-D", "--defined-only", L.LIB_PATH_F16 if fmt == "f16" else L.LIB_PATH], text=True)
    assert " T hesic_homonet_prepare_items\n" in exported


@pytest.mark.parametrize("bad, word", [
    (dict(items=None), "null"), (dict(corners=None), "null"), (dict(B=0), "shape"), (dict(B=65536), "shape"),
    (dict(S=0), "P <= S"), (dict(P=0), "P <= S"), (dict(P=9), "P <= S"), (dict(S=16385), "P <= S"),
    (dict(std=0.0), "std"), (dict(std=float("nan")), "std"), (dict(mean=float("nan")), "std"), (dict(items=4), "misaligned"),
    (dict(grey2=2), "misaligned"),
], ids=lambda v: "-".join(f"{k}" for k in v) if isinstance(v, dict) else None)
def test_bad_arguments_return_einval_with_a_message(bad, word):
    """Host dummies for pointers: every case is refused before anything is launched or dereferenced.  An integer moves that pointer by so
    many bytes off its 8-byte alignment."""
    lib = L.lib()
    buf = (C.c_double * 16)()
    a = dict(items=0, B=1, S=8, P=4, mean=0.5, std=0.25, grey1=0, grey2=0, patch1=0, patch2=0, corners=0)
    a.update(bad)
    ptr = {k: None if a[k] is None else C.c_void_p(C.addressof(buf) + a[k]) for k in ("items", "grey1", "grey2", "patch1", "patch2", "corners")}
    assert lib.hesic_homonet_prepare_items(ptr["items"], a["B"], a["S"], a["P"], a["mean"], a["std"], ptr["grey1"], ptr["grey2"], ptr["patch1"],
                                           ptr["patch2"], ptr["corners"], None) == -1
    msg = lib.hesic_last_error().decode()
    assert msg.startswith("homonet_prepare_items:") and word in msg, msg


# ---------------------------------------------------------------------------------------------------------------- host checks
def _good_items():
    """Three items that satisfy the contract for S = 16, P = 8 (the pointers are never followed on the host)."""
    items = Fn.homonet_items(3)
    for b, (pitch, rows, x0, y0, cw, ch, wx, wy) in enumerate([(17, 13, 0, 0, 17, 13, 0, 0), (20, 32, 3, 5, 17, 27, 8, 8), (40, 9, 39, 8, 1, 1, 4, 0)]):
        items[b] = (4096, 8192, pitch, rows, x0, y0, cw, ch, wx, wy)
    return items


def test_check_homonet_items_accepts_the_contracts_edges():
    Fn.check_homonet_items(_good_items(), 16, 8)


@pytest.mark.parametrize("b, change, word", [
    (1, dict(x0=4), "columns"),               # one pixel past the right edge
    (1, dict(y0=6), "rows"),                  # one pixel past the bottom edge
    (2, dict(cw=0), "crop"),
    (0, dict(ch=0), "crop"),
    (1, dict(wx=9), "window"),                # S - P + 1
    (2, dict(wy=9), "window"),
    (0, dict(wx=-1), "window"),
    (2, dict(x0=-1), "columns"),
    (1, dict(left=0), "null"),
    (2, dict(right=0), "null"),
])
def test_check_homonet_items_names_the_item(b, change, word):
    items = _good_items()
    for k, v in change.items():
        items[b][k] = v
    with pytest.raises(ValueError, match=rf"item {b} .*{word}|item {b} {word}"):
        Fn.check_homonet_items(items, 16, 8)
    launches = []
    with L.call_hook(lambda name, args: launches.append(name)):
        with pytest.raises(ValueError, match=f"item {b} "):
            Fn.homonet_prepare_items(items, 16, 8, 0.5, 0.25)          # refused on the host, before the device is asked for
    assert launches == []


def test_homonet_prepare_items_argument_errors():
    with pytest.raises(ValueError, match="HOMONET_ITEM_DTYPE"):
        Fn.homonet_prepare_items(Fn.pair_items(2), 16, 8, 0.5, 0.25)
    with pytest.raises(ValueError, match=r"\(B, 48\)"):
        Fn.homonet_prepare_items(torch.zeros(2, 40, dtype=torch.uint8), 16, 8, 0.5, 0.25)
    with pytest.raises(ValueError, match="P <= S"):
        Fn.homonet_prepare_items(_good_items(), 8, 16, 0.5, 0.25)
    with pytest.raises(ValueError, match="B <= 65535"):
        Fn.homonet_prepare_items(Fn.homonet_items(0), 16, 8, 0.5, 0.25)


# ------------------------------------------------------------------------------------------------------------------ draw_batch
def _write_folder(root, split, sizes, seed=0):
    """PNG pairs of the given (height, width) list under root/split/{left,right}; returns the decoded arrays per pair."""
    from PIL import Image
    g = np.random.Generator(np.random.PCG64(seed))
    out = []
    for side in ("left", "right"):
        (root / split / side).mkdir(parents=True)
    for i, (h, w) in enumerate(sizes):
        a, b = (g.integers(0, 256, size=(h, w, 3), dtype=np.uint8) for _ in range(2))
        Image.fromarray(a).save(root / split / "left" / f"pair{i:02d}.png")
        Image.fromarray(b).save(root / split / "right" / f"pair{i:02d}.png")
        out.append((a, b))
    return out


@pytest.mark.parametrize("crop", [None, (7, 9)], ids=["whole", "crop7x9"])
@pytest.mark.parametrize("S, P, rho", [(32, 16, 4), (64, 32, 20)], ids=["windows_drawn", "no_window_draw"])
def test_draw_batch_consumes_the_stream_as_the_host_route(tmp_path, crop, S, P, rho):
    """``load_batch`` then ``window_origins`` on one stream, ``draw_batch`` on an equally seeded one: the same windows, the crops are the
    full images sliced at the drawn origins, and the two streams end in the same state.  (64, 32, 20): S - rho - P < rho, no window draw."""
    sizes = [(12, 15)] * 3
    stored = _write_folder(tmp_path, "train", sizes)
    items = homography_train.list_pairs(tmp_path, "train")
    assert [it[2] for it in items] == [(15, 12)] * 3
    rng_a, rng_b = random.Random("7/3"), random.Random("7/3")
    x1, x2 = homography_train.load_batch(items, crop, rng_a, "cpu")
    want_windows = homography.window_origins(len(items), None, S, P, rho, rng_a)
    origins, got_sizes, windows = homography_train.draw_batch(items, crop, rng_b, S, P, rho)
    assert windows == want_windows
    assert rng_a.getstate() == rng_b.getstate()
    assert len(origins) == 3 and (got_sizes is None if crop is None else got_sizes == [crop] * 3)
    if S - rho - P < rho:
        assert windows == [(0, 0)] * 3
    for b, ((left, right), (y0, x0)) in enumerate(zip(stored, origins)):
        ch, cw = crop if crop is not None else sizes[b]
        assert (crop is not None or (y0, x0) == (0, 0)) and 0 <= y0 <= sizes[b][0] - ch and 0 <= x0 <= sizes[b][1] - cw
        assert np.array_equal(x1[b].permute(1, 2, 0).numpy(), left[y0:y0 + ch, x0:x0 + cw])
        assert np.array_equal(x2[b].permute(1, 2, 0).numpy(), right[y0:y0 + ch, x0:x0 + cw])
    if crop is not None:
        assert len(set(origins)) > 1                                # the draws differ between pairs: the order of the draws is checked


def test_batches_mix_sizes_forms_one_pool():
    pairs = [(f"l{i}", f"r{i}", (16, 12) if i % 2 else (20, 10)) for i in range(12)]
    grouped = homography_train.batches(pairs, 4, None, random.Random(1), True)
    mixed = homography_train.batches(pairs, 4, None, random.Random(1), True, mix_sizes=True)
    assert sorted(len(b) for b in grouped) == [2, 2, 4, 4] and [len(b) for b in mixed] == [4, 4, 4]
    assert all(len({p[2] for p in b}) == 1 for b in grouped) and any(len({p[2] for p in b}) == 2 for b in mixed)
    assert sorted(p for b in mixed for p in b) == sorted(pairs)
    assert homography_train.batches(pairs, 4, None, None, False) == homography_train.batches(pairs, 4, None, None, False, mix_sizes=False)


# ---------------------------------------------------------------------------------------------------------------------- parser
def test_parser_cache_options(tmp_path, capsys):
    a = homography_train.parser().parse_args(["root"])
    assert a.cache == "host" and a.mix_sizes is False and a.cache_gb is None and a.num_workers == 3
    a = homography_train.parser().parse_args(["root", "--cache", "stream", "--mix-sizes", "-n", "2", "--cache-gb", "0.5"])
    assert (a.cache, a.mix_sizes, a.num_workers, a.cache_gb) == ("stream", True, 2, 0.5)
    for argv in (["--mix-sizes"], ["--mix-sizes", "--cache", "host"], ["--cache", "disk"], ["--cache", "device", "-n", "0"],
                 ["--cache", "device", "--cache-gb", "0"]):
        with pytest.raises(SystemExit) as e:
            homography_train.main([str(tmp_path)] + argv)
        assert e.value.code == 2
    assert "--mix-sizes needs --cache device" in capsys.readouterr().err


@pytest.mark.parametrize("cache", ["host", "device", "stream"])
def test_main_without_a_device_returns_2(tmp_path, cache, capsys, monkeypatch):
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    assert homography_train.main([str(tmp_path), "--cache", cache]) == 2
    assert "needs a ROCm device" in capsys.readouterr().err

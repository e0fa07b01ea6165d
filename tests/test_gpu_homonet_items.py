"""HomographyNet's inputs straight from stored uint8 images (include/hesic_homonet_items.h, functional.homonet_prepare_items,
pair_cache.DevicePairCache.homonet_batch, ``python -m hesic_amd.homography_train --cache device|stream [--mix-sizes]``).  The kernel is held
to the BITS of tests/homonet_items_ref.py -- ``homography_prep_ref.prepare`` on each item's crop -- and of ``functional.homonet_prepare`` on
that crop; the folder trainer to the bits of its host route."""
import functools

import numpy as np
import pytest
import torch

import homonet_items_ref as IR
import memguard
from hesic_amd import codec, homography, homography_train, pair_cache, synthetic, train
from hesic_amd import functional as Fn
from hesic_amd.compressai.datasets import MEAN, STD

pytestmark = pytest.mark.gpu
DEV = "cuda"
NAMES = ("grey1", "grey2", "patch1", "patch2", "corners")
S, P = 16, 8
STORED = [(13, 17), (32, 20), (9, 40), (16, 16)]                                    # (rows, pitch_px) of the four stored pairs
# (x0, y0, cw, ch, wx, wy): a whole image (rows up, columns down), an interior crop at an odd origin (columns up, rows down), a crop flush
# against the bottom-right corner of its image (columns down by more than 2, rows up), and an S x S crop that is copied
GEOMETRY = [(0, 0, 17, 13, 0, 0), (3, 5, 11, 23, S - P, S - P), (7, 4, 33, 5, 3, 5), (0, 0, 16, 16, S - P, 0)]


@functools.lru_cache(maxsize=None)
def _case():
    """(lefts, rights, restatement) of the mixed batch, computed once; nothing mutates them."""
    g = np.random.Generator(np.random.PCG64(2024))
    lefts, rights = ([g.integers(0, 256, size=(r, p, 3), dtype=np.uint8) for r, p in STORED] for _ in range(2))
    for v in lefts + rights:
        v[: max(v.shape[0] // 2, 1), : max(v.shape[1] // 2, 1)] &= 0xFE          # even levels: averages land on k + 0.5 there
        v[0, 0], v[-1, -1] = 255, 0
    return lefts, rights, IR.prepare_items(lefts, rights, GEOMETRY, S, P, float(MEAN), float(STD))


def _outside(shape, geo, value, img):
    """``img`` with every byte outside the crop rectangle set to ``value``."""
    x0, y0, cw, ch = geo[:4]
    out = np.full(shape, value, dtype=np.uint8)
    out[y0:y0 + ch, x0:x0 + cw] = img[y0:y0 + ch, x0:x0 + cw]
    return out


def _run(lefts, rights, geometry, outside=None, fill=memguard.NAN_FILL, order=None):
    """functional.homonet_prepare_items on guarded stored images (bytes outside the crops optionally overwritten) into guarded, NaN-filled
    ``out=`` tensors; every guard is checked, and the tensors returned are the ones passed.  ``order``: the items of the batch."""
    order = list(range(len(geometry))) if order is None else list(order)
    B = len(order)
    views, items = [], Fn.homonet_items(B)
    for b, i in enumerate(order):
        x0, y0, cw, ch, wx, wy = geometry[i]
        pair = []
        for name, img in (("left", lefts[i]), ("right", rights[i])):
            if outside is not None:
                img = _outside(img.shape, geometry[i], outside, img)
            t = memguard.guarded(torch.from_numpy(img).to(DEV), fill=fill, name=f"{name}{i}")
            assert t.is_contiguous()
            pair.append(t)
        views += pair
        items[b] = (pair[0].data_ptr(), pair[1].data_ptr(), lefts[i].shape[1], lefts[i].shape[0], x0, y0, cw, ch, wx, wy)
    outs = [memguard.guarded(torch.full(s, float("nan"), device=DEV), name=n)
            for n, s in zip(NAMES, [(B, 1, S, S), (B, 1, S, S), (B, 1, P, P), (B, 1, P, P), (B, 4, 2)])]
    got = Fn.homonet_prepare_items(items, S, P, float(MEAN), float(STD), out=outs)
    torch.cuda.synchronize()
    memguard.check_all(views + outs)
    assert all(g is o for g, o in zip(got, outs))
    return [t.cpu().numpy() for t in got]


def _assert_bits(tag, got, want):
    for name, g, w in zip(NAMES, got, want):
        assert g.dtype == np.float32 and g.shape == w.shape, (tag, name)
        nbad = int((g.view(np.int32) != w.view(np.int32)).sum())
        print(f"homonet_items {tag} {name} elements that differ in bits: {nbad} of {g.size}")
        assert nbad == 0 and np.array_equal(g, w), (tag, name)


def test_bits_of_the_restatement_mixed_sizes_in_one_launch():
    lefts, rights, want = _case()
    got = _run(lefts, rights, GEOMETRY)
    _assert_bits("restatement", got, want)
    # ... and of the strided entry on the uint8 crop view of every item alone
    for b, (x0, y0, cw, ch, wx, wy) in enumerate(GEOMETRY):
        a, c = (torch.from_numpy(v).to(DEV)[y0:y0 + ch, x0:x0 + cw].permute(2, 0, 1)[None] for v in (lefts[b], rights[b]))
        assert a.shape == (1, 3, ch, cw)
        alone = Fn.homonet_prepare(a, c, torch.tensor([[wx, wy]], dtype=torch.int32, device=DEV), S, P, float(MEAN), float(STD))
        for name, g, w in zip(NAMES, got, alone):
            assert torch.equal(torch.from_numpy(g[b:b + 1]), w.cpu()), (b, name)


def test_nothing_outside_the_crop_is_read():
    """Every byte outside the crop rectangles -- the rest of the stored images and the guards around them; item 2's crop ends at the last
    byte of its image, flush against the trailing guard -- takes two different values: the same bits, equal to the restatement's, and
    intact guards.  A tap clamped to the stored image instead of the crop reads those bytes."""
    lefts, rights, want = _case()
    x0, y0, cw, ch = GEOMETRY[2][:4]
    assert (y0 + ch, x0 + cw) == STORED[2]
    a = _run(lefts, rights, GEOMETRY, outside=0x00, fill=0xFF)
    b = _run(lefts, rights, GEOMETRY, outside=0xFF, fill=0x00)
    _assert_bits("outside_00", a, want)
    _assert_bits("outside_ff", b, want)


def test_every_output_element_is_written_and_out_is_returned():
    lefts, rights, _ = _case()
    got = _run(lefts, rights, GEOMETRY)                  # NaN-filled out= tensors, returned as passed (asserted in _run)
    for name, g in zip(NAMES, got):
        assert np.isfinite(g).all(), name
    # a crop one pixel wide and one pixel high: the narrow path writes everything too, one level everywhere
    geo = [(16, 12, 1, 1, 0, 0), (0, 0, 1, 32, S - P, 3)]
    one = _run(lefts[:2], rights[:2], geo)
    _assert_bits("one_pixel", one, IR.prepare_items(lefts[:2], rights[:2], geo, S, P, float(MEAN), float(STD)))
    assert all(np.isfinite(g).all() for g in one) and len(np.unique(one[0][0])) == 1


def test_items_are_independent_of_batch_and_position():
    lefts, rights, want = _case()
    for i in range(len(GEOMETRY)):
        _assert_bits(f"alone{i}", _run(lefts, rights, GEOMETRY, order=[i]), [w[i:i + 1] for w in want])
    order = [3, 1, 1, 0, 2, 3, 0]
    _assert_bits("reordered", _run(lefts, rights, GEOMETRY, order=order), [w[order] for w in want])


# ----------------------------------------------------------------------------------------------------------------- the cache
def _write_pairs(root, split, first_seed, n, h, w, start=0):
    from PIL import Image
    x1, x2, _ = synthetic.stereo_batch(first_seed, n, h, w)
    for side, x in (("left", x1), ("right", x2)):
        d = root / split / side
        d.mkdir(parents=True, exist_ok=True)
        for i, img in enumerate(codec.quantise(x)):
            Image.fromarray(img).save(d / f"pair{start + i:02d}.png")
    return codec.quantise(x1), codec.quantise(x2)


@pytest.mark.parametrize("crops", [False, True], ids=["whole", "crops"])
def test_cache_homonet_batch_device_equals_stream(tmp_path, crops):
    la, ra = _write_pairs(tmp_path, "train", 10, 2, 24, 40)
    lb, rb = _write_pairs(tmp_path, "train", 20, 2, 33, 21, start=2)
    lefts, rights = list(la) + list(lb), list(ra) + list(rb)
    indices, windows = [3, 0, 2, 1, 3], [(0, 0), (8, 8), (1, 7), (8, 0), (4, 4)]
    origins = [(9, 5), (0, 0), (20, 0), (3, 17), (0, 2)] if crops else None
    sizes = [(24, 16), (24, 40), (13, 21), (16, 23), (5, 19)] if crops else None
    got = {}
    for mode in ("device", "stream"):
        cache = pair_cache.DevicePairCache(tmp_path, "train", mode=mode, workers=2)
        assert cache.sizes == [(24, 40)] * 2 + [(33, 21)] * 2
        got[mode] = [t.cpu().numpy() for t in cache.homonet_batch(indices, origins, sizes, windows, S, P)]
        again = [t.cpu().numpy() for t in cache.homonet_batch(indices[:2], None if not crops else origins[:2], None if not crops else sizes[:2],
                                                             windows[:2], S, P)]                 # the slab is reused for a smaller batch
        _assert_bits(f"{mode}_again", again, [g[:2] for g in got[mode]])
    _assert_bits("device_vs_stream", got["device"], got["stream"])
    geo = [((0, 0) if not crops else (origins[b][1], origins[b][0])) +
           ((lefts[i].shape[1], lefts[i].shape[0]) if not crops else (sizes[b][1], sizes[b][0])) + windows[b] for b, i in enumerate(indices)]
    want = IR.prepare_items([lefts[i] for i in indices], [rights[i] for i in indices], geo, S, P, float(MEAN), float(STD))
    _assert_bits("cache_vs_restatement", got["device"], want)
    with pytest.raises(ValueError, match="outside pair 0"):
        cache.homonet_batch([0], [(0, 25)], [(24, 16)], [(0, 0)], S, P)
    with pytest.raises(ValueError, match="window"):
        cache.homonet_batch([0], None, None, [(S - P + 1, 0)], S, P)


# ----------------------------------------------------------------------------------------------------------- folder training
def _train(root, out, *extra, epochs=2):
    logs = []
    hist = homography_train.main([str(root), "--picsize", "64", "--patchsize", "32", "--rho", "8", "--batch_size", "4", "--seed", "1", "--epochs",
                                  str(epochs), "--out", str(out), *extra], log=logs.append)
    assert len(logs) == len(hist)
    return hist, torch.load(out / "checkpoint.pth.tar", map_location="cpu")


def _assert_same_run(tag, a, b):
    (ha, ca), (hb, cb) = a, b
    assert [(r["epoch"], r["train_loss"], r["valid_loss"], r["steps"], r["best"]) for r in ha] == \
        [(r["epoch"], r["train_loss"], r["valid_loss"], r["steps"], r["best"]) for r in hb], tag
    _assert_same_checkpoint(tag, ca, cb)


def _assert_same_checkpoint(tag, ca, cb):
    assert set(ca) == set(cb) == {"state_dict", "loss", "optimizer", "dropout", "epoch", "seed"}, tag
    assert ca["dropout"] == cb["dropout"] and ca["loss"] == cb["loss"] and ca["epoch"] == cb["epoch"], tag
    assert set(ca["state_dict"]) == set(cb["state_dict"])
    for k, v in ca["state_dict"].items():
        assert torch.equal(v, cb["state_dict"][k]), (tag, k)
    sa, sb = ca["optimizer"]["state"], cb["optimizer"]["state"]
    assert set(sa) == set(sb) and len(sa) > 0
    for i in sa:
        for k in ("step", "exp_avg", "exp_avg_sq"):
            assert torch.equal(sa[i][k], sb[i][k]), (tag, i, k)


@pytest.mark.parametrize("crop", [(), ("--crop", "64", "96")], ids=["whole", "crop64x96"])
def test_folder_training_is_the_same_in_every_cache_mode(tmp_path, crop):
    root = tmp_path / "data"
    _write_pairs(root, "train", 100, 8, 96, 128)
    _write_pairs(root, "test", 200, 4, 96, 128)
    runs = {mode: _train(root, tmp_path / mode, "--cache", mode, *crop) for mode in ("host", "device", "stream")}
    hist = runs["host"][0]
    assert [r["epoch"] for r in hist] == [0, 1] and all(r["steps"] == 2 and np.isfinite(r["train_loss"]) and np.isfinite(r["valid_loss"]) for r in hist)
    assert all("cache" not in r and "decode_seconds" not in r for r in hist)                        # the host route's records are unchanged
    for mode in ("device", "stream"):
        _assert_same_run(mode, runs["host"], runs[mode])
        h = runs[mode][0]
        assert all(r["cache"] == mode for r in h) and h[0]["decode_seconds"] >= 0 and "decode_seconds" not in h[1]
    assert runs["device"][0][0]["decode_seconds"] > 0 and runs["stream"][0][0]["decode_seconds"] == 0
    if not crop:
        # one epoch under ``device``, the second resumed under ``host``: the two-epoch run's parameters
        _train(root, tmp_path / "r", "--cache", "device", epochs=1)
        more, resumed = _train(root, tmp_path / "r", "--cache", "host", "--resume", str(tmp_path / "r" / "checkpoint.pth.tar"))
        assert [r["epoch"] for r in more] == [1] and more[0]["valid_loss"] == hist[1]["valid_loss"]
        _assert_same_checkpoint("resumed", runs["host"][1], resumed)


def test_mix_sizes_fills_the_batches(tmp_path):
    root = tmp_path / "data"
    for split, n in (("train", 6), ("test", 2)):
        _write_pairs(root, split, 100 if split == "train" else 200, n, 96, 128)
        _write_pairs(root, split, 300 if split == "train" else 400, n, 80, 112, start=n)
    grouped = _train(root, tmp_path / "g", "--cache", "device", epochs=1)
    mixed = [_train(root, tmp_path / f"m{k}", "--cache", "device", "--mix-sizes", epochs=1) for k in range(2)]
    assert grouped[0][0]["steps"] == 4 and all(m[0][0]["steps"] == 3 for m in mixed)
    assert all(np.isfinite(m[0][0]["train_loss"]) and np.isfinite(m[0][0]["valid_loss"]) for m in mixed)
    _assert_same_run("mixed_twice", mixed[0], mixed[1])
    # one mixed batch: its loss is that of inputs prepared per size group by the strided entry and concatenated
    cache = pair_cache.DevicePairCache(root, "train", mode="device")
    indices, windows = [0, 5, 6, 11], [(8, 8), (24, 9), (10, 24), (17, 17)]
    assert [cache.sizes[i] for i in indices] == [(96, 128)] * 2 + [(80, 112)] * 2
    got = cache.homonet_batch(indices, None, None, windows, 64, 32)
    parts = []
    for lo in (0, 2):
        views = [torch.stack([torch.from_numpy(cache._read(i)[v]) for i in indices[lo:lo + 2]]).to(DEV).permute(0, 3, 1, 2) for v in (0, 1)]
        parts.append(Fn.homonet_prepare(views[0], views[1], torch.tensor(windows[lo:lo + 2], dtype=torch.int32, device=DEV), 64, 32,
                                        float(MEAN), float(STD)))
    want = [torch.cat([p[k] for p in parts]) for k in range(5)]
    for name, g, w in zip(NAMES, got, want):
        assert torch.equal(g, w), name
    torch.manual_seed(1)
    net = homography.Net(patch_size=32)
    synthetic.fill_homography_state_dict_(net.state_dict())
    trainer = train.HomographyTrainer(net.to(DEV), lr=1e-4, seed=1)
    loss_a = trainer.evaluate(got[0], got[2], got[3], got[4])
    loss_b = trainer.evaluate(want[0], want[2], want[3], want[4])
    print(f"homonet_items mixed batch loss {float(loss_a):.9f} / per size group {float(loss_b):.9f}")
    assert bool(torch.isfinite(loss_a)) and torch.equal(loss_a, loss_b)

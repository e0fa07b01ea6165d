"""Device-resident pair batches, the parts that need no GPU: the numpy restatement the GPU test holds the kernel to (tests/pair_batch_ref.py)
against the loader's host path, ``pair_cache.crop_origin`` / ``epoch_plan`` / ``bytes_needed``, the C ABI of include/hesic_pair_batch.h and the
refusals of ``python -m hesic_amd.train_folder``'s parser."""
import ctypes as C
import random
import subprocess

import numpy as np
import pytest
import torch

import pair_batch_ref as R
from hesic_amd import _lib as L
from hesic_amd import functional as Fn
from hesic_amd import pair_cache, train_folder
from hesic_amd.compressai.datasets import ImageFolder, to_tensor


def _write_pair(root, split, stem, left, right, H=None):
    from PIL import Image
    for side, img in (("left", left), ("right", right)):
        d = root / split / side
        d.mkdir(parents=True, exist_ok=True)
        Image.fromarray(img).save(d / f"{stem}.png")
    if H is not None:
        (root / split / "H").mkdir(exist_ok=True)
        np.save(root / split / "H" / f"{stem}.npy", H)


def _random_image(g, h, w):
    return g.integers(0, 256, size=(h, w, 3), dtype=np.uint8)


# ------------------------------------------------------------------------------------------- the restatement against the loader
@pytest.mark.parametrize("shape, crop, origin", [((37, 53), (32, 30), (5, 23)), ((64, 80), (32, 30), (0, 1)), ((33, 32), (32, 30), (1, 2)),
                                                 ((41, 45), (41, 1), (0, 44))])
def test_restatement_pixels_equal_to_tensor(shape, crop, origin):
    g = np.random.Generator(np.random.PCG64([3, *shape]))
    img = _random_image(g, *shape)
    img[0, 0], img[-1, -1] = 255, 0
    (ph, pw), (y0, x0) = crop, origin
    got = R.pixels(img, x0, y0, ph, pw)
    assert got.dtype == np.float32 and np.array_equal(got, to_tensor(img[y0:y0 + ph, x0:x0 + pw]).numpy())


def test_all_256_levels_equal_to_tensor():
    img = np.arange(256, dtype=np.uint8).reshape(1, 256, 1).repeat(3, axis=2)
    assert np.array_equal(R.pixels(img, 0, 0, 1, 256), to_tensor(img).numpy())


def _realistic_matrix(g):
    """A full-image homography as SURF + RANSAC returns them: near a translation of tens of pixels, small perspective terms, [2,2] = 1 -- with
    fp64 entries that are not fp32-representable."""
    H = np.eye(3) + g.normal(0, 0.02, size=(3, 3))
    H[0, 2], H[1, 2] = g.uniform(-60, 60), g.uniform(-20, 20)
    H[2, 0], H[2, 1] = g.normal(0, 2e-5), g.normal(0, 2e-5)
    return H / H[2, 2]


def test_restatement_matrices_within_one_ulp_of_the_loader(tmp_path):
    """One fp32 ulp: the loader's matrix products may contract into fused multiply-adds where the restatement (and the kernel) may not; both
    are fp64 results a few fp64 ulps apart, so after the cast to fp32 they differ by at most one rounding flip."""
    g = np.random.Generator(np.random.PCG64(11))
    _write_pair(tmp_path, "train", "a", _random_image(g, 8, 8), _random_image(g, 8, 8))
    ds = ImageFolder(tmp_path, split="train")
    worst, flips = 0.0, 0
    for _ in range(2000):
        H = _realistic_matrix(g)
        x0, y0 = int(g.integers(0, 1201)), int(g.integers(0, 1201))
        ds._sidecar = lambda stem: H
        want = ds._pair_homography(0, None, None, x0, y0).numpy()
        got = R.matrix(H.reshape(-1), x0, y0)
        assert got.dtype == np.float32 and got.shape == (3, 3)
        ulp = np.spacing(np.maximum(np.abs(want), np.abs(got)).astype(np.float32))
        err = np.abs(got.astype(np.float64) - want.astype(np.float64)) / ulp
        worst, flips = max(worst, float(err.max())), flips + int((got != want).sum())
        assert float(err.max()) <= 1.0
    print(f"pair_batch_ref matrices: {flips} of {2000 * 9} entries differ from the loader's, worst {worst:.2f} ulp (bar 1)")
    assert np.array_equal(R.matrix(None, 5, 7), np.eye(3, dtype=np.float32))
    assert np.array_equal(R.matrix(np.eye(3).reshape(-1), 31, 17), np.eye(3, dtype=np.float32))       # a pure crop shift keeps the identity


# ---------------------------------------------------------------------------------------------------------------- crop_origin
@pytest.mark.parametrize("size, patch", [((96, 128), (64, 64)), ((80, 112), (64, 112)), ((64, 128), (64, 64)), ((66, 65), (64, 64))])
def test_crop_origin_is_the_loaders(tmp_path, size, patch):
    g = np.random.Generator(np.random.PCG64([5, *size]))
    left, right = _random_image(g, *size), _random_image(g, *size)
    _write_pair(tmp_path, "train", "a", left, right)
    ds = ImageFolder(tmp_path, transform=to_tensor, patch_size=patch, split="train")
    (Himg, Wimg), (ph, pw) = size, patch
    ys, xs = set(), set()
    for s in range(40):
        random.seed(s)
        item = ds[0]
        y0, x0 = pair_cache.crop_origin(random.Random(s), Himg, Wimg, ph, pw)
        ys.add(y0)
        xs.add(x0)
        assert torch.equal(item[0], to_tensor(left[y0:y0 + ph, x0:x0 + pw])) and torch.equal(item[1], to_tensor(right[y0:y0 + ph, x0:x0 + pw]))
    if ph == Himg:
        assert ys == {0} and xs == {0}                      # full height: no offset at all, although pw < Wimg
    else:
        assert max(ys) <= Himg - ph - 1 and max(xs) <= max(Wimg - pw - 1, 0)        # the last row / column offsets are never drawn
        assert len(ys) > 1 or Himg - ph - 1 == 0


def test_crop_origin_draw_order_and_refusal():
    class Rec:
        def __init__(self):
            self.calls = []

        def randint(self, a, b):
            self.calls.append((a, b))
            return b

    r = Rec()
    assert pair_cache.crop_origin(r, 100, 64, 64, 64) == (35, 0) and r.calls == [(0, 35), (0, 0)]      # y first; Wimg - pw - 1 = -1: max(..., 0)
    r = Rec()
    assert pair_cache.crop_origin(r, 64, 200, 64, 64) == (0, 0) and r.calls == []
    with pytest.raises(ValueError, match="larger"):
        pair_cache.crop_origin(random.Random(0), 64, 64, 128, 64)


# ----------------------------------------------------------------------------------------------------------------- epoch_plan
SIZES = [(96, 128)] * 3 + [(80, 112)] * 2


def _plan(**kw):
    a = dict(n_pairs=5, sizes=SIZES, batch_size=2, ph=64, pw=64, seed=1, epoch=0, shuffle=True, drop_tail=False)
    a.update(kw)
    return pair_cache.epoch_plan(**a)


def test_epoch_plan_depends_only_on_its_arguments():
    random.seed(0)
    a = _plan()
    random.seed(123)
    random.random()
    b = _plan()
    assert list(a) == list(b) and a.rng.getstate() == b.rng.getstate()
    assert list(_plan(epoch=1)) != list(a) and list(_plan(seed=2)) != list(a)
    for plan in (a, _plan(epoch=1), _plan(epoch=7)):
        assert sorted(i for idx, _ in plan for i in idx) == [0, 1, 2, 3, 4]                # every pair once per epoch
        assert [len(idx) for idx, _ in plan] == [2, 2, 1] and plan.dropped == 0 and plan.left_out == 0
        for idx, org in plan:
            assert len(idx) == len(org)
            for i, (y0, x0) in zip(idx, org):
                assert 0 <= y0 <= SIZES[i][0] - 64 - 1 and 0 <= x0 <= SIZES[i][1] - 64 - 1


def test_epoch_plan_is_the_documented_stream():
    rng = random.Random("1/3")
    order = list(range(5))
    rng.shuffle(order)
    want = []
    for c0 in range(0, 5, 2):
        idx = order[c0:c0 + 2]
        want.append((idx, [pair_cache.crop_origin(rng, *SIZES[i], 64, 64) for i in idx]))
    assert list(_plan(epoch=3)) == want


def test_resumed_plans_equal_the_uninterrupted_run():
    full = [list(_plan(epoch=e)) for e in range(3)]
    resumed = [list(_plan(epoch=e)) for e in range(1, 3)]                # a --resume at epoch 1 builds only the later plans
    assert resumed == full[1:]


def test_validation_plan_is_keyed_by_the_seed_alone():
    a = _plan(epoch=None, shuffle=False, batch_size=4)
    assert [idx for idx, _ in a] == [[0, 1, 2, 3], [4]]
    assert list(a) == list(_plan(epoch=None, shuffle=False, batch_size=4)) and list(a) != list(_plan(epoch=None, shuffle=False, batch_size=4, seed=9))


def test_drop_tail_and_left_out_are_counted():
    p = _plan(drop_tail=True)
    assert [len(idx) for idx, _ in p] == [2, 2] and p.dropped == 1
    assert _plan(drop_tail=True, batch_size=5).dropped == 0
    q = _plan(keep=[0, 2, 3])
    assert q.left_out == 2 and sorted(i for idx, _ in q for i in idx) == [0, 2, 3]
    q = _plan(keep=[0, 2, 3], drop_tail=True)
    assert q.left_out == 2 and q.dropped == 1 and len(q) == 1
    with pytest.raises(ValueError, match="outside"):
        _plan(keep=[5])
    with pytest.raises(ValueError, match="sizes"):
        _plan(n_pairs=4)


def test_cache_listing_and_sidecars_without_a_device(tmp_path):
    g = np.random.Generator(np.random.PCG64(2))
    H = _realistic_matrix(g)
    _write_pair(tmp_path, "train", "a", _random_image(g, 20, 24), _random_image(g, 20, 24), H)
    _write_pair(tmp_path, "train", "b", _random_image(g, 16, 40), _random_image(g, 16, 40))
    _write_pair(tmp_path, "train", "c", _random_image(g, 16, 40), _random_image(g, 16, 40))
    (tmp_path / "train" / "H" / "c.txt").write_text(" ".join(repr(float(v)) for v in (2 * H).reshape(-1)))
    c = pair_cache.DevicePairCache(tmp_path, "train", mode="stream")
    assert c.stems == ["a", "b", "c"] and c.sizes == [(20, 24), (16, 40), (16, 40)] and c.has_h == [True, False, True]
    assert c.h_index == [0, -1, 1] and np.array_equal(c.h_host, np.stack([H.reshape(-1), (2 * H).reshape(-1)]))
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            pair_cache.DevicePairCache(tmp_path, "train", mode="device")
    with pytest.raises(ValueError, match="mode"):
        pair_cache.DevicePairCache(tmp_path, "train", mode="host")


# --------------------------------------------------------------------------------------------------------------- the budget
def test_bytes_needed_by_hand_and_the_budget_refusal():
    # 37 x 53 x 3 = 5883 -> 5888 (23 * 256); 64 x 80 x 3 = 15360 (60 * 256) exactly; 1 x 1 x 3 = 3 -> 256
    assert pair_cache.bytes_needed([(37, 53)]) == 2 * 5888
    assert pair_cache.bytes_needed([(64, 80)]) == 2 * 15360
    assert pair_cache.bytes_needed([(37, 53), (64, 80), (1, 1)], n_matrices=2) == 2 * (5888 + 15360 + 256) + 144
    assert pair_cache.bytes_needed([]) == 0
    assert pair_cache.bytes_needed([(860, 1080)] * 2000) == 2000 * 2 * 2786560             # 860 * 1080 * 3 = 2786400 -> 10885 * 256: 11.1 GB
    pair_cache.check_budget(1000, 1000)
    with pytest.raises(MemoryError) as e:
        pair_cache.check_budget(11146240000, 4294967296)
    assert "11146240000" in str(e.value) and "4294967296" in str(e.value) and 'mode="stream"' in str(e.value)


# ------------------------------------------------------------------------------------------------------------------------ ABI
@pytest.mark.parametrize("fmt", ["bf16", "f16"])
def test_abi_header_bindings_exports(fmt):
    declared = L.declared_symbols("hesic_pair_batch.h")
    assert declared == ["hesic_pair_batch_gather"]
    assert set(declared) == set(L._PAIR_BATCH_SIGS)
    assert not set(declared) & set(L.declared_symbols())                # a header of its own: include/hesic_hip.h does not list it
    assert "hesic_pair_batch.h" not in open(L.header_path("hesic_hip.h")).read()
    assert "#define HESIC_ABI_VERSION 3" in open(L.header_path("hesic_hip.h")).read() and L.ABI_VERSION == 3
    exported = subprocess.check_output(["nm", "-D", "--defined-only", L.LIB_PATH_F16 if fmt == "f16" else L.LIB_PATH], text=True)
    for s in declared:
        assert f" T {s}\n" in exported, s


def test_item_struct_is_48_bytes_in_every_form():
    assert C.sizeof(L.PairItem) == 48
    assert np.dtype(Fn.PAIR_ITEM_DTYPE).itemsize == 48
    assert [n for n, _ in L.PairItem._fields_] == [n for n, _ in Fn.PAIR_ITEM_DTYPE]
    assert [getattr(L.PairItem, n).offset for n, _ in L.PairItem._fields_] == [np.dtype(Fn.PAIR_ITEM_DTYPE).fields[n][1] for n, _ in Fn.PAIR_ITEM_DTYPE]
    text = open(L.header_path("hesic_pair_batch.h")).read()
    for n, _ in Fn.PAIR_ITEM_DTYPE:
        assert n in text


def _call_raw(lib, **kw):
    """hesic_pair_batch_gather with host dummies for pointers: every case below is refused before anything is launched or dereferenced."""
    buf = (C.c_double * 16)()
    p = C.cast(buf, C.c_void_p)
    a = dict(items=p, h_table=p, B=1, ph=4, pw=4, x1=p, x2=p, h_out=p)
    a.update(kw)
    return lib.hesic_pair_batch_gather(a["items"], a["h_table"], a["B"], a["ph"], a["pw"], a["x1"], a["x2"], a["h_out"], None)


@pytest.mark.parametrize("bad, word", [
    (dict(items=None), "null"), (dict(x1=None), "null"), (dict(x2=None), "null"), (dict(h_out=None), "null"),
    (dict(B=0), "shape"), (dict(B=-1), "shape"), (dict(ph=0), "shape"), (dict(pw=0), "shape"), (dict(pw=-4), "shape"),
    (dict(B=8, ph=16384, pw=16384), "overflows"), (dict(B=1, ph=2 ** 31 - 1, pw=2), "overflows"), (dict(B=65536, ph=128, pw=128), "overflows"),
], ids=lambda v: "-".join(f"{k}{x}" for k, x in v.items()) if isinstance(v, dict) else None)
def test_bad_arguments_return_einval_with_a_message(bad, word):
    lib = L.lib()
    assert _call_raw(lib, **bad) == -1
    msg = lib.hesic_last_error().decode()
    assert msg.startswith("pair_batch_gather:") and word in msg, msg


def test_misaligned_pointers_are_refused():
    lib = L.lib()
    buf = (C.c_double * 16)()
    assert _call_raw(lib, x1=C.c_void_p(C.addressof(buf) + 2)) == -1
    assert lib.hesic_last_error().decode().startswith("pair_batch_gather: misaligned")


# ------------------------------------------------------------------------------------------------- the wrapper's host checks
def _items(**kw):
    it = Fn.pair_items(2)
    for f, v in dict(left=4096, right=8192, pitch_px=40, rows=30, x0=3, y0=2, hx=3, hy=2, h_index=-1).items():
        it[f] = v
    for f, v in kw.items():
        it[f][1] = v
    return it


@pytest.mark.parametrize("bad, word", [
    (dict(x0=-1), "columns"), (dict(x0=9), "columns"), (dict(y0=-1), "rows"), (dict(y0=15), "rows"), (dict(h_index=-2), "h_index"),
    (dict(h_index=0), "h_index"), (dict(left=0), "null"), (dict(reserved=1), "reserved"), (dict(pitch_px=0), "stored image"),
], ids=lambda v: "-".join(f"{k}{x}" for k, x in v.items()) if isinstance(v, dict) else None)
def test_wrapper_checks_every_item_before_any_launch(bad, word):
    launches = []
    with L.call_hook(lambda name, args: launches.append(name)):
        Fn.check_pair_items(_items(), 0, 16, 32)                         # x0 + pw = 35 <= 40, y0 + ph = 18 <= 30: accepted
        with pytest.raises(ValueError, match=word) as e:
            Fn.pair_batch_gather(_items(**bad), None, 16, 32)
        assert "item 1" in str(e.value)
        with pytest.raises(ValueError, match="shape"):
            Fn.pair_batch_gather(_items(), None, 0, 32)
        with pytest.raises(ValueError, match="PAIR_ITEM_DTYPE"):
            Fn.pair_batch_gather(np.zeros(2), None, 16, 32)
    assert launches == []


# ------------------------------------------------------------------------------------------------------------------- parser
def test_parser_defaults_are_the_references():
    a = train_folder.parser().parse_args(["root"])
    assert (a.epochs, a.learning_rate, a.aux_learning_rate, a.lmbda, a.batch_size, a.test_batch_size, tuple(a.patch_size), a.num_workers,
            a.save, a.seed) == (100, 1e-4, 1e-3, 1e-2, 16, 64, (256, 256), 3, False, None)
    assert (a.model, a.homography, a.distortion, a.graphed, a.dtype, a.cache, a.valid_split, a.resume) == \
        ("hesic", "sidecar", "mse", False, "bf16", "device", "test", "none")


def test_parser_refuses_bad_patch_sizes(tmp_path, capsys):
    g = np.random.Generator(np.random.PCG64(4))
    for split in ("train", "test"):
        _write_pair(tmp_path, split, "a", _random_image(g, 80, 112), _random_image(g, 80, 112), np.eye(3))
    for patch, word in ((("96", "64"), "multiples of 64"), (("64", "100"), "multiples of 64"), (("0", "64"), "multiples of 64"),
                        (("128", "64"), "larger than"), (("64", "128"), "larger than")):
        with pytest.raises(SystemExit) as e:
            train_folder.main([str(tmp_path), "--patch-size", *patch, "-e", "0"], log=lambda s: None)
        assert e.value.code == 2 and word in capsys.readouterr().err
    with pytest.raises(SystemExit):
        train_folder.main([str(tmp_path), "--homography-checkpoint", "x.pth.tar", "-e", "0"], log=lambda s: None)

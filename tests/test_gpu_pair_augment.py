"""Stereo-aware augmentation in the pair gather on the GPU (include/hesic_pair_augment.h, functional.pair_batch_gather_aug,
pair_cache.DevicePairCache.batch(flags=...), ``--augment`` of ``python -m hesic_amd.train_folder`` / ``train_stage2``).  The kernel is held to
the BITS of tests/pair_augment_ref.py, which tests/test_pair_augment_cpu.py holds to numpy flips, ``numpy.linalg.inv`` and a bilinear warp;
the folder trainers are held to that restatement applied to ``pair_cache.epoch_plan(..., augment=...)``."""
import functools

import numpy as np
import pytest
import torch

import memguard
import pair_augment_ref as A
import pair_batch_ref as R
from hesic_amd import functional as Fn
from hesic_amd import codec, pair_cache, synthetic, train, train_folder, train_stage2

pytestmark = pytest.mark.gpu
DEV = "cuda"
ALL = ("hflip", "vflip", "swap")

STORED = ((37, 53), (40, 64))                                       # (rows, pitch_px) of the stored images, items alternate between them
CROPS = {"16x20_vec": (16, 20), "16x19_scalar": (16, 19), "5x1": (5, 1)}      # 16-byte stores; 4-byte stores with a partial group; one pixel per thread
# where item k's crop sits in its stored image, as (column, row) with 0 = flush with the first and 1 = flush with the last; two rounds so that
# every flag value meets the image's first bytes and its last bytes (under HFLIP a row's first thread reads the crop's LAST columns)
CORNERS = {"a": ((1, 1), (1, 1), (0, 1), (0, 0), (1, 0), (0, 0), (0, 0), (1, 1)),
           "b": ((0, 0), (0, 0), (1, 0), (1, 1), (0, 1), (1, 1), (1, 1), (0, 0))}
H_INDEX = (2, -1, 0, 1, -1, 2, 0, 1)                                # -1 on some items, a table row on the others
LEFT_OFFSET = (0, 1, 2, 3, 3, 2, 1, 0)                              # bytes of each left view past a 256-byte boundary


@functools.lru_cache(maxsize=None)
def _kernel_reference(crop, rnd):
    """(views, table, items, restatement) of a kernel case, computed once; nothing mutates them.  Item k carries flags k."""
    ph, pw = CROPS[crop]
    g = np.random.Generator(np.random.PCG64([17, ph, pw, ord(rnd)]))
    views = []
    for k in range(8):
        h, w = STORED[k % 2]
        a, b = g.integers(0, 256, size=(h, w, 3), dtype=np.uint8), g.integers(0, 256, size=(h, w, 3), dtype=np.uint8)
        a[0, 0], a[-1, -1], b[0, 0], b[-1, -1] = 255, 0, 0, 255
        views.append((a, b))
    table = np.stack([np.eye(3) + g.normal(0, 0.02, size=(3, 3)) for _ in range(3)])
    table[:, 0, 2], table[:, 1, 2] = g.uniform(-60, 60, size=3), g.uniform(-20, 20, size=3)
    table[:, 2, :2] = g.normal(0, 2e-5, size=(3, 2))
    table = table.reshape(3, 9)
    assert (table.astype(np.float32).astype(np.float64) != table).any(axis=1).all()         # not fp32-representable
    items = []
    for k, ((a, b), (cx, cy)) in enumerate(zip(views, CORNERS[rnd])):
        x0, y0 = cx * (a.shape[1] - pw), cy * (a.shape[0] - ph)
        # the re-basing translation is NOT the stored-image origin: the two travel separately in the descriptor
        items.append((a, b, x0, y0, x0 + 100 * k, y0 + 7 * k, H_INDEX[k], k))
    return views, table, items, A.gather(items, table, ph, pw)


def _launch(entry, crop, rnd, flags=None):
    """``entry`` on a case's items from guarded inputs into NaN-filled guarded outputs; returns the outputs after every guard was checked."""
    ph, pw = CROPS[crop]
    views, table, ref_items, _ = _kernel_reference(crop, rnd)
    ins = [memguard.guarded(torch.from_numpy(table).to(DEV), name="h_table")]
    items = Fn.pair_items(8)
    for k, (a, b, x0, y0, hx, hy, hi, f) in enumerate(ref_items):
        ga = memguard.guarded(torch.from_numpy(a).to(DEV), name=f"left{k}", offset=LEFT_OFFSET[k])
        gb = memguard.guarded(torch.from_numpy(b).to(DEV), name=f"right{k}")
        assert ga.data_ptr() % 256 == LEFT_OFFSET[k]
        ins += [ga, gb]
        it = items[k]
        it["left"], it["right"], it["pitch_px"], it["rows"] = ga.data_ptr(), gb.data_ptr(), a.shape[1], a.shape[0]
        it["x0"], it["y0"], it["hx"], it["hy"], it["h_index"], it["reserved"] = x0, y0, hx, hy, hi, f if flags is None else flags[k]
    outs = [memguard.guarded(torch.full(s, float("nan"), device=DEV), name=n)
            for n, s in zip(("x1", "x2", "h"), [(8, 3, ph, pw), (8, 3, ph, pw), (8, 3, 3)])]
    got = entry(items, ins[0], ph, pw, out=outs)
    torch.cuda.synchronize()
    for t in ins + outs:
        t.check()
    for n, g in zip(("x1", "x2", "h"), got):
        assert g.dtype == torch.float32 and not bool(torch.isnan(g).any()), n            # every element was written
    return got, items, ins


@pytest.mark.parametrize("rnd", list(CORNERS))
@pytest.mark.parametrize("crop", list(CROPS))
def test_kernel_equals_the_restatement(crop, rnd):
    ph, pw = CROPS[crop]
    want = _kernel_reference(crop, rnd)[3]
    got, items, ins = _launch(Fn.pair_batch_gather_aug, crop, rnd)
    for n, g, w in zip(("x1", "x2", "h"), got, want):
        assert tuple(g.shape) == w.shape, n
        bad = (g.cpu() != torch.from_numpy(w)).flatten(1).sum(1).tolist()
        print(f"pair_augment_parity {crop} {rnd} {n} elements that differ from the restatement, per item (= flags): {bad} of {g[0].numel()}")
        assert torch.equal(g.cpu(), torch.from_numpy(w)), n
    # the same call without out=: fresh tensors, the same bits
    again = Fn.pair_batch_gather_aug(items, ins[0], ph, pw)
    for g, a in zip(got, again):
        assert torch.equal(g, a)


@pytest.mark.parametrize("crop", list(CROPS))
def test_new_entry_without_flags_equals_the_old_entry(crop):
    new, _, _ = _launch(Fn.pair_batch_gather_aug, crop, "a", flags=[0] * 8)
    old, _, _ = _launch(Fn.pair_batch_gather, crop, "a", flags=[0] * 8)
    _, table, items, _ = _kernel_reference(crop, "a")
    want = R.gather([it[:7] for it in items], table, *CROPS[crop])
    for n, a, b, w in zip(("x1", "x2", "h"), new, old, want):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32)), n
        assert torch.equal(a.cpu(), torch.from_numpy(w)), n


def test_wrapper_refuses_an_unknown_bit_before_any_launch():
    from hesic_amd import _lib as L
    a = torch.zeros(64, 80, 3, dtype=torch.uint8, device=DEV)
    items = Fn.pair_items(2)
    items["left"], items["right"], items["pitch_px"], items["rows"], items["h_index"] = a.data_ptr(), a.data_ptr(), 80, 64, -1
    items["reserved"] = (7, 8)
    launches = []
    with L.call_hook(lambda name, args: launches.append(name)):
        with pytest.raises(ValueError, match="item 1 reserved"):
            Fn.pair_batch_gather_aug(items, None, 64, 64)
        with pytest.raises(ValueError, match="item 0 reserved field must be 0"):
            Fn.pair_batch_gather(items, None, 64, 64)
    assert launches == []


# ------------------------------------------------------------------------------------------------------------------ the folder
SIZES = {"train": [(96, 128)] * 3 + [(80, 112)] * 2, "test": [(96, 128), (80, 112), (96, 128)]}


@pytest.fixture(scope="module")
def folder(tmp_path_factory):
    """ROOT with five training and three test pairs (PNG, ``synthetic.smooth_stereo_pair``) and fp64 sidecars, the fixture of
    tests/test_gpu_pair_batch.py; returns (root, images, rows): ``images[split][i] = (left, right)`` uint8 HWC and ``rows[split][i]`` the
    nine sidecar values.  Nothing mutates them."""
    from PIL import Image
    root = tmp_path_factory.mktemp("augment_pairs")
    images, rows = {}, {}
    for split, first in (("train", 100), ("test", 200)):
        images[split], rows[split] = [], []
        for d in ("left", "right", "H"):
            (root / split / d).mkdir(parents=True)
        for i, (h, w) in enumerate(SIZES[split]):
            x1, x2, H = synthetic.smooth_stereo_pair(first + i, h, w)
            q = codec.quantise(torch.from_numpy(np.stack([x1, x2])))
            Image.fromarray(q[0]).save(root / split / "left" / f"pair{i:02d}.png")
            Image.fromarray(q[1]).save(root / split / "right" / f"pair{i:02d}.png")
            H64 = H.astype(np.float64) * (1.0 + 1e-9 * (i + 1)) + 1e-11          # fp64 entries that are not fp32-representable
            np.save(root / split / "H" / f"pair{i:02d}.npy", H64)
            images[split].append((q[0], q[1]))
            rows[split].append(H64.reshape(9))
    return root, images, rows


def _plan(split, batch, epoch, shuffle=True, drop_tail=False, seed=1, augment=ALL):
    s = SIZES[split]
    return pair_cache.epoch_plan(len(s), s, batch, 64, 64, seed, epoch, shuffle, drop_tail, augment=augment)


def _want(plan, folder, split):
    _, images, rows = folder
    return [tuple(torch.from_numpy(v) for v in b) for b in A.plan_batches(plan, images[split], rows[split], 64, 64)]


def _assert_inputs(got, want):
    assert len(got) == len(want)
    for k, (g, w) in enumerate(zip(got, want)):
        for n, a, b in zip(("x1", "x2", "h_matrix"), g, w):
            assert torch.equal(a, b), (k, n)


class _Recorder:
    """Records every ``step`` of a trainer class: the inputs (copies), and whether they ARE the trainer's static inputs."""

    def __init__(self, monkeypatch, cls):
        self.inputs, self.static, self.trainers, orig = [], [], [], cls.step
        rec = self

        def step(self, x1, x2, h_matrix, *args, **kw):
            rec.inputs.append((x1.cpu(), x2.cpu(), h_matrix.cpu()))
            st = self.static_inputs() if hasattr(self, "static_inputs") else None
            rec.static.append(st is not None and all(a.data_ptr() == b.data_ptr() for a, b in zip(st, (x1, x2, h_matrix))))
            if self not in rec.trainers:
                rec.trainers.append(self)
            return orig(self, x1, x2, h_matrix, *args, **kw)

        monkeypatch.setattr(cls, "step", step)


def _record_validation(monkeypatch, mod):
    """The inputs of every validation batch of ``mod`` (train_folder / train_stage2), as host copies."""
    seen, orig = [], mod.valid_batch_values

    def values(*args, **kw):
        x1, x2, h = [t for t in args if torch.is_tensor(t)][:3]
        seen.append((x1.cpu(), x2.cpu(), h.cpu()))
        return orig(*args, **kw)

    monkeypatch.setattr(mod, "valid_batch_values", values)
    return seen


def test_device_mode_equals_stream_mode_equals_the_restatement(folder):
    root = folder[0]
    dev = pair_cache.DevicePairCache(root, "train", mode="device")
    stream = pair_cache.DevicePairCache(root, "train", mode="stream", workers=2)
    plan = _plan("train", 2, 0)
    assert sorted({f for fl in plan.flags for f in fl}) != [0]
    for (idx, org), fl, want in zip(plan, plan.flags, _want(plan, folder, "train")):
        a, b = dev.batch(idx, org, 64, 64, flags=fl), stream.batch(idx, org, 64, 64, flags=fl)
        for x, y, w in zip(a[:3], b[:3], want):
            assert torch.equal(x, y) and torch.equal(x.cpu(), w)
        assert a[3].tolist() == b[3].tolist() == [True] * len(idx)
    # all eight flag values on one pair, against the plain batch flipped by torch
    x1, x2, _, _ = dev.batch([3] * 8, [(5, 9)] * 8, 64, 64)
    y1, y2, _, _ = dev.batch([3] * 8, [(5, 9)] * 8, 64, 64, flags=list(range(8)))
    for f in range(8):
        dims = [d for d, bit in ((1, 2), (2, 1)) if f & bit]
        a, b = (x2[f], x1[f]) if f & 4 else (x1[f], x2[f])
        assert torch.equal(y1[f], a.flip(dims) if dims else a) and torch.equal(y2[f], b.flip(dims) if dims else b), f
    with pytest.raises(ValueError, match="flags"):
        dev.batch([3], [(5, 9)], 64, 64, flags=[1, 2])
    with pytest.raises(ValueError, match="reserved"):
        dev.batch([3], [(5, 9)], 64, 64, flags=[8])


def test_no_flags_is_the_old_entrys_call(folder):
    from hesic_amd import _lib as L
    dev = pair_cache.DevicePairCache(folder[0], "train", mode="device")
    calls = []
    with L.call_hook(lambda name, args: calls.append(name)):
        dev.batch([0, 3], [(1, 2), (3, 4)], 64, 64)
        dev.batch([0, 3], [(1, 2), (3, 4)], 64, 64, flags=[0, 0])
        dev.batch([0, 3], [(1, 2), (3, 4)], 64, 64, flags=[0, 4])
    assert calls == ["hesic_pair_batch_gather", "hesic_pair_batch_gather", "hesic_pair_batch_gather_aug"]


@pytest.fixture(scope="module")
def plain_validation(folder):
    """(validation batches, records) of a run WITHOUT --augment (one epoch), recorded once."""
    mp = pytest.MonkeyPatch()
    try:
        seen = _record_validation(mp, train_folder)
        hist = train_folder.main([str(folder[0]), "--patch-size", "64", "64", "--batch-size", "2", "--test-batch-size", "2", "-e", "1", "--seed", "1"],
                          log=lambda s: None)
    finally:
        mp.undo()
    assert len(seen) == 2
    return seen, hist


def test_folder_training_feeds_the_augmented_plan_and_plain_validation(folder, tmp_path, monkeypatch, plain_validation):
    rec = _Recorder(monkeypatch, train.Trainer)
    valid = _record_validation(monkeypatch, train_folder)
    hist = train_folder.main([str(folder[0]), "--patch-size", "64", "64", "--batch-size", "2", "--test-batch-size", "2", "--seed", "1", "-e", "2",
                              "--augment", *ALL], log=lambda s: None)
    assert [r["epoch"] for r in hist] == [0, 1] and all(r["steps"] == 3 for r in hist)
    plans = [_plan("train", 2, e) for e in (0, 1)]
    assert plans[0].flags != plans[1].flags
    _assert_inputs(rec.inputs, [b for p in plans for b in _want(p, folder, "train")])
    for r, p in zip(hist, plans):
        assert r["augmented"] == p.augmented() and list(r["augmented"]) == ["hflip", "vflip", "swap"]
    # validation: never augmented -- the batches of a run without the option, and of the plain restatement
    _assert_inputs(valid, plain_validation[0] * 2)
    vplan = _plan("test", 2, None, shuffle=False, augment=())
    _assert_inputs(valid[:2], [tuple(torch.from_numpy(v) for v in b) for b in R.plan_batches(vplan, folder[1]["test"], folder[2]["test"], 64, 64)])


def test_records_without_the_option_have_no_augmented_key(plain_validation):
    assert len(plain_validation[1]) == 1 and "augmented" not in plain_validation[1][0]


def test_resume_is_fed_the_uninterrupted_runs_augmented_batches(folder, tmp_path, monkeypatch):
    common = [str(folder[0]), "--patch-size", "64", "64", "--batch-size", "2", "--test-batch-size", "2", "--save", "--out", str(tmp_path),
              "--augment", *ALL]
    first = train_folder.main(common + ["-e", "1", "--seed", "1"], log=lambda s: None)
    assert [r["epoch"] for r in first] == [0]
    before = torch.load(tmp_path / "checkpoint.pth.tar", map_location="cpu")
    assert set(before) == {"epoch", "state_dict", "loss", "optimizer", "aux_optimizer", "seed"}           # the checkpoint's keys do not change
    rec = _Recorder(monkeypatch, train.Trainer)
    more = train_folder.main(common + ["-e", "2", "--resume", str(tmp_path / "checkpoint.pth.tar")], log=lambda s: None)
    assert [r["epoch"] for r in more] == [1] and more[0]["augmented"] == _plan("train", 2, 1).augmented()
    _assert_inputs(rec.inputs, _want(_plan("train", 2, 1), folder, "train"))          # epoch 1's own plan and flags, from the checkpoint's seed


@pytest.mark.parametrize("cache", ["device", "stream"])
def test_graphed_training_gathers_the_augmented_batch_into_the_static_inputs(folder, monkeypatch, cache):
    rec = _Recorder(monkeypatch, train.GraphedTrainer)
    hist = train_folder.main([str(folder[0]), "--patch-size", "64", "64", "--batch-size", "1", "--test-batch-size", "3", "-e", "1", "--graphed",
                              "--seed", "1", "--cache", cache, "--augment", *ALL], log=lambda s: None)
    assert [r["steps"] for r in hist] == [5]
    (tr,) = rec.trainers
    assert tr.graph is not None and rec.static[0] is False and all(rec.static[tr.warmup:])       # from the capture on: no staging copy
    plan = _plan("train", 1, 0, drop_tail=True)
    assert any(f for fl in plan.flags[tr.warmup:] for f in fl)                                    # a flagged batch is replayed, not only warmed up
    _assert_inputs(rec.inputs, _want(plan, folder, "train"))


def test_stage2_training_feeds_the_flipped_batches(folder, monkeypatch):
    import hesic_amd
    rec = _Recorder(monkeypatch, train.EnhancerTrainer)
    try:
        hist = train_stage2.main([str(folder[0]), "--checkpoint", "synthetic", "--patch-size", "64", "64", "--batch-size", "2", "--test-batch-size",
                                  "3", "--seed", "1", "-e", "1", "--augment", "hflip"], log=lambda s: None)
    finally:
        hesic_amd.set_compute_dtype(torch.bfloat16)
        hesic_amd.set_compute_dtype(torch.float32)
    plan = _plan("train", 2, 0, augment=("hflip",))
    assert hist[0]["steps"] == 3 and hist[0]["augmented"] == plan.augmented() and hist[0]["augmented"]["vflip"] == 0
    assert {f for fl in plan.flags for f in fl} == {0, 1}
    _assert_inputs(rec.inputs, _want(plan, folder, "train"))

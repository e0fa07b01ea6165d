"""Device-resident pair batches on the GPU (include/hesic_pair_batch.h, functional.pair_batch_gather, pair_cache.DevicePairCache,
``python -m hesic_amd.train_folder``).  The kernel is held to the BITS of tests/pair_batch_ref.py, which tests/test_pair_batch_cpu.py holds
to the loader's host path; the folder trainer is held to that restatement applied to ``pair_cache.epoch_plan``."""
import functools
import math

import numpy as np
import pytest
import torch

import memguard
import pair_batch_ref as R
from hesic_amd import functional as Fn
from hesic_amd import codec, homography, models, pair_cache, stereo_h, synthetic, train, train_folder

pytestmark = pytest.mark.gpu
DEV = "cuda"

# (stored (rows, pitch_px), ...), (ph, pw), [(x0, y0, h_index)], byte offset of each left view past a 256-byte boundary
KERNEL_CASES = {
    # x0 mod 4 = 3, 1, 2, 0; item 0 is flush with the last row and column of its image, item 3 with its last row; h_index -1, 0 and the last row
    "b4_32x30": (((37, 53), (64, 80), (41, 45), (33, 32)), (32, 30), [(23, 5, 2), (1, 0, -1), (2, 4, 0), (0, 1, 2)], (0, 0, 0, 0)),
    # pw a multiple of 4: the 16-byte-store path only; ph == rows
    "b1_64x64": (((64, 80),), (64, 64), [(13, 0, 1)], (0,)),
    # pw = 1: every thread owns one pixel; the first pixel of a view that starts 1 byte past a dword, and the last pixel of a view
    "b2_5x1": (((5, 7), (5, 7)), (5, 1), [(0, 0, 0), (6, 0, -1)], (1, 3)),
}


@functools.lru_cache(maxsize=None)
def _kernel_reference(name):
    """(views, table, restatement) of a kernel case, computed once; nothing mutates them."""
    shapes, (ph, pw), where, _ = KERNEL_CASES[name]
    g = np.random.Generator(np.random.PCG64([7, ph, pw]))
    views = [(g.integers(0, 256, size=(h, w, 3), dtype=np.uint8), g.integers(0, 256, size=(h, w, 3), dtype=np.uint8)) for h, w in shapes]
    for a, b in views:
        a[0, 0], a[-1, -1], b[0, 0], b[-1, -1] = 255, 0, 0, 255
    table = np.stack([np.eye(3) + g.normal(0, 0.02, size=(3, 3)) for _ in range(3)])
    table[:, 0, 2], table[:, 1, 2] = g.uniform(-60, 60, size=3), g.uniform(-20, 20, size=3)
    table[:, 2, :2] = g.normal(0, 2e-5, size=(3, 2))
    table = table.reshape(3, 9)
    assert (table.astype(np.float32).astype(np.float64) != table).any(axis=1).all()         # not fp32-representable
    # the re-basing translation is NOT the stored-image origin here: the two travel separately in the descriptor
    items = [(v[0], v[1], x0, y0, x0 + 100 * k, y0 + 7 * k, hi) for k, (v, (x0, y0, hi)) in enumerate(zip(views, where))]
    return views, table, R.gather(items, table, ph, pw)


@pytest.mark.parametrize("name", list(KERNEL_CASES))
def test_kernel_equals_the_restatement(name):
    shapes, (ph, pw), where, offsets = KERNEL_CASES[name]
    views, table, want = _kernel_reference(name)
    B = len(shapes)
    ins = [memguard.guarded(torch.from_numpy(table).to(DEV), name="h_table")]
    items = Fn.pair_items(B)
    for k, ((a, b), (x0, y0, hi), off) in enumerate(zip(views, where, offsets)):
        ga = memguard.guarded(torch.from_numpy(a).to(DEV), name=f"left{k}", offset=off)
        gb = memguard.guarded(torch.from_numpy(b).to(DEV), name=f"right{k}")
        ins += [ga, gb]
        it = items[k]
        it["left"], it["right"], it["pitch_px"], it["rows"] = ga.data_ptr(), gb.data_ptr(), a.shape[1], a.shape[0]
        it["x0"], it["y0"], it["hx"], it["hy"], it["h_index"] = x0, y0, x0 + 100 * k, y0 + 7 * k, hi
    outs = [memguard.guarded(torch.full(s, float("nan"), device=DEV), name=n)
            for n, s in zip(("x1", "x2", "h"), [(B, 3, ph, pw), (B, 3, ph, pw), (B, 3, 3)])]
    got = Fn.pair_batch_gather(items, ins[0], ph, pw, out=outs)
    torch.cuda.synchronize()
    for t in ins + outs:
        t.check()
    for n, g, w in zip(("x1", "x2", "h"), got, want):
        assert g.dtype == torch.float32 and tuple(g.shape) == w.shape, n
        assert not bool(torch.isnan(g).any()), n
        nbad = int((g.cpu() != torch.from_numpy(w)).sum())
        print(f"pair_batch_parity {name} {n} elements that differ from the restatement: {nbad} of {g.numel()}")
        assert torch.equal(g.cpu(), torch.from_numpy(w)), n
    # the same call without out=: fresh tensors, the same bits
    again = Fn.pair_batch_gather(items, ins[0], ph, pw)
    for g, a in zip(got, again):
        assert torch.equal(g, a)


def test_wrapper_refuses_a_bad_item_before_any_launch():
    from hesic_amd import _lib as L
    views, table, _ = _kernel_reference("b1_64x64")
    a = torch.from_numpy(views[0][0]).to(DEV)
    items = Fn.pair_items(1)
    items["left"], items["right"], items["pitch_px"], items["rows"], items["h_index"] = a.data_ptr(), a.data_ptr(), 80, 64, -1
    launches = []
    with L.call_hook(lambda name, args: launches.append(name)):
        for field, value, word in (("x0", 17, "columns"), ("y0", 1, "rows"), ("h_index", 3, "h_index")):
            bad = items.copy()
            bad[field] = value
            with pytest.raises(ValueError, match=word):
                Fn.pair_batch_gather(bad, torch.from_numpy(table).to(DEV), 64, 64)
        with pytest.raises(ValueError, match="out must be"):
            Fn.pair_batch_gather(items, None, 64, 64, out=[torch.empty(1, 3, 64, 64, device=DEV)] * 3)
    assert launches == []


# ------------------------------------------------------------------------------------------------------------------ the folder
SIZES = {"train": [(96, 128)] * 3 + [(80, 112)] * 2, "test": [(96, 128), (80, 112), (96, 128)]}


@pytest.fixture(scope="module")
def folder(tmp_path_factory):
    """ROOT with five training and three test pairs (PNG, ``synthetic.smooth_stereo_pair``) and fp64 sidecars; returns (root, images, rows):
    ``images[split][i] = (left, right)`` uint8 HWC and ``rows[split][i]`` the nine sidecar values.  Nothing mutates them."""
    from PIL import Image
    root = tmp_path_factory.mktemp("pairs")
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


def _plan(split, batch, epoch, shuffle=True, drop_tail=False, seed=1):
    s = SIZES[split]
    return pair_cache.epoch_plan(len(s), s, batch, 64, 64, seed, epoch, shuffle, drop_tail)


def _want(plan, folder, split):
    _, images, rows = folder
    return [tuple(torch.from_numpy(v) for v in b) for b in R.plan_batches(plan, images[split], rows[split], 64, 64)]


def test_stream_mode_equals_device_mode(folder):
    root = folder[0]
    dev = pair_cache.DevicePairCache(root, "train", mode="device")
    stream = pair_cache.DevicePairCache(root, "train", mode="stream", workers=2)
    assert dev.sizes == SIZES["train"] and all(dev.has_h) and dev.arena.numel() == pair_cache.bytes_needed(SIZES["train"])
    assert stream.arena is None and dev.decode_seconds > 0
    plan = _plan("train", 2, 0)
    for (idx, org), want in zip(plan, _want(plan, folder, "train")):
        a, b = dev.batch(idx, org, 64, 64), stream.batch(idx, org, 64, 64)
        for x, y, w in zip(a[:3], b[:3], want):
            assert torch.equal(x, y) and torch.equal(x.cpu(), w)              # pairs of two image sizes share the first batches
        assert a[3].tolist() == b[3].tolist() == [True] * len(idx)
    with pytest.raises(ValueError, match="outside"):
        dev.batch([3], [(17, 0)], 64, 64)                                     # 17 + 64 > 80 rows
    with pytest.raises(MemoryError, match='mode="stream"'):
        pair_cache.DevicePairCache(root, "train", mode="device", budget_bytes=1000)


class _Recorder:
    """Records every ``step`` of a trainer class: the inputs (copies), and whether they ARE the trainer's static inputs."""

    def __init__(self, monkeypatch, cls):
        self.inputs, self.static, self.trainers, orig = [], [], [], cls.step
        rec = self

        def step(self, x1, x2, h_matrix, noise=None):
            rec.inputs.append((x1.cpu(), x2.cpu(), h_matrix.cpu()))
            st = self.static_inputs() if hasattr(self, "static_inputs") else None
            rec.static.append(st is not None and all(a.data_ptr() == b.data_ptr() for a, b in zip(st, (x1, x2, h_matrix))))
            if self not in rec.trainers:
                rec.trainers.append(self)
            return orig(self, x1, x2, h_matrix, noise=noise)

        monkeypatch.setattr(cls, "step", step)


def _finite(rec):
    return all(math.isfinite(v) for part in ("train", "valid") for v in rec[part].values())


def _assert_inputs(got, want):
    assert len(got) == len(want)
    for k, (g, w) in enumerate(zip(got, want)):
        for n, a, b in zip(("x1", "x2", "h_matrix"), g, w):
            assert torch.equal(a, b), (k, n)


def _valid_by_hand(net, folder, lmbda):
    """test_epoch's record recomputed in fp64 on the host from ``models.rate_distortion`` on the same batches."""
    plan = _plan("test", 2, None, shuffle=False)
    vals = []
    with torch.no_grad():
        for x1, x2, h in _want(plan, folder, "test"):
            x1, x2, h = x1.to(DEV), x2.to(DEV), h.to(DEV)
            rd = models.rate_distortion(net(x1, x2, h), x1, x2)
            n = rd["num_pixels"]
            bpp = sum(float(v) for k, v in rd.items() if k.startswith("bits_")) / n
            m1, m2 = float(rd["sse1"]) / (3 * n), float(rd["sse2"]) / (3 * n)
            vals.append({"loss": lmbda * 255 ** 2 * (m1 + m2) + bpp, "mse_loss": m1 + m2, "bpp_loss": bpp, "aux_loss": float(net.aux_loss()),
                         "psnr1": 10 * math.log10(1 / m1), "psnr2": 10 * math.log10(1 / m2)})
    mean = {k: sum(v[k] for v in vals) / len(vals) for k in vals[0]}
    mean["psnr"] = (mean["psnr1"] + mean["psnr2"]) / 2
    mean["psnr_of_mse"] = 10 * math.log10(1 / (mean["mse_loss"] / 2))
    mean["batches"] = len(vals)
    return mean


@pytest.mark.parametrize("model", ["hesic", "joint"])
def test_folder_training_feeds_the_plan_and_checkpoints(folder, tmp_path, monkeypatch, model):
    rec = _Recorder(monkeypatch, train.Trainer)
    common = [str(folder[0]), "--patch-size", "64", "64", "--batch-size", "2", "--test-batch-size", "2", "--save", "--model", model, "--seed", "1"]
    logs = []
    hist = train_folder.main(common + ["-e", "2", "--out", str(tmp_path / "a")], log=logs.append)
    assert [r["epoch"] for r in hist] == [0, 1] and len(logs) == 2 and all(r["steps"] == 3 and _finite(r) for r in hist)
    assert all(r["left_out_no_sidecar"] == 0 and r["dropped_tail"] == 0 for r in hist) and "decode_seconds" in hist[0]
    want = [b for e in (0, 1) for b in _want(_plan("train", 2, e), folder, "train")]
    assert [w[0].shape[0] for w in want] == [2, 2, 1, 2, 2, 1]                    # the ragged tail of one
    _assert_inputs(rec.inputs, want)
    (tr,) = rec.trainers
    assert float(tr.optimizer.step_count) == 6 and float(tr.aux_optimizer.step_count) == 6
    last = torch.load(tmp_path / "a" / "checkpoint.pth.tar", map_location="cpu")
    best = torch.load(tmp_path / "a" / "checkpoint_best_loss.pth.tar", map_location="cpu")
    assert set(last) == {"epoch", "state_dict", "loss", "optimizer", "aux_optimizer", "seed"}
    assert last["epoch"] == 1 and last["seed"] == 1 and last["loss"] == hist[1]["valid_loss"]
    assert best["loss"] == min(r["valid_loss"] for r in hist)
    assert all(float(s["step"]) == 6 for s in last["optimizer"]["state"].values())
    cls = models.HSIC if model == "hesic" else models.HSICJoint
    assert set(last["state_dict"]) == set(cls().state_dict()) and all(not v.is_cuda for v in last["state_dict"].values())
    # the file loads through codec.load_model, and the validation record is the averaging of rate_distortion's sums (1e-6 relative: the same
    # arithmetic on the same sums)
    net = codec.load_model(tmp_path / "a" / "checkpoint.pth.tar", torch.bfloat16, model=model)
    hand = _valid_by_hand(net, folder, 1e-2)
    for k, v in hand.items():
        got = hist[1]["valid"][k]
        print(f"train_folder valid {model} {k}: record {got!r} by hand {v!r}")
        assert abs(got - v) <= 1e-6 * abs(v), k


def test_resume_is_fed_the_uninterrupted_runs_batches(folder, tmp_path, monkeypatch):
    common = [str(folder[0]), "--patch-size", "64", "64", "--batch-size", "2", "--test-batch-size", "2", "--save", "--out", str(tmp_path)]
    first = train_folder.main(common + ["-e", "1", "--seed", "1"], log=lambda s: None)
    assert [r["epoch"] for r in first] == [0]
    rec = _Recorder(monkeypatch, train.Trainer)
    more = train_folder.main(common + ["-e", "2", "--resume", str(tmp_path / "checkpoint.pth.tar")], log=lambda s: None)
    assert [r["epoch"] for r in more] == [1] and more[0]["steps"] == 3 and _finite(more[0])
    _assert_inputs(rec.inputs, _want(_plan("train", 2, 1), folder, "train"))          # epoch 1's own plan, from the checkpoint's seed
    (tr,) = rec.trainers
    assert float(tr.optimizer.step_count) == 6 and float(tr.aux_optimizer.step_count) == 6      # three restored + three taken
    ck = torch.load(tmp_path / "checkpoint.pth.tar", map_location="cpu")
    assert ck["epoch"] == 1 and ck["seed"] == 1


def test_graphed_training_gathers_into_the_static_inputs(folder, tmp_path, monkeypatch):
    rec = _Recorder(monkeypatch, train.GraphedTrainer)
    hist = train_folder.main([str(folder[0]), "--patch-size", "64", "64", "--batch-size", "1", "--test-batch-size", "2", "-e", "2", "--graphed",
                              "--seed", "1"], log=lambda s: None)
    assert [r["steps"] for r in hist] == [5, 5] and all(_finite(r) and r["dropped_tail"] == 0 for r in hist)
    (tr,) = rec.trainers
    assert tr.graph is not None and tr.calls == 10 and tr.warmup == 3
    assert rec.static[0] is False and all(rec.static[tr.warmup:])                 # from the capture (the first replay) on: no staging copy
    _assert_inputs(rec.inputs, [b for e in (0, 1) for b in _want(_plan("train", 1, e, drop_tail=True), folder, "train")])
    assert not (tmp_path / "checkpoint.pth.tar").exists()                         # --save is off


def test_graphed_drops_and_counts_the_ragged_tail(folder, monkeypatch):
    rec = _Recorder(monkeypatch, train.GraphedTrainer)
    hist = train_folder.main([str(folder[0]), "--patch-size", "64", "64", "--batch-size", "2", "--test-batch-size", "3", "-e", "1", "--graphed",
                              "--seed", "1", "--cache", "stream"], log=lambda s: None)
    assert hist[0]["steps"] == 2 and hist[0]["dropped_tail"] == 1 and _finite(hist[0])
    _assert_inputs(rec.inputs, _want(_plan("train", 2, 0, drop_tail=True), folder, "train"))


@pytest.mark.parametrize("source", ["net", "surf"])
def test_homography_from_the_net_and_from_surf(folder, monkeypatch, source):
    rec = _Recorder(monkeypatch, train.Trainer)
    hist = train_folder.main([str(folder[0]), "--patch-size", "64", "64", "--batch-size", "2", "--test-batch-size", "3", "-e", "1", "--seed", "1",
                              "--homography", source], log=lambda s: None)
    assert hist[0]["steps"] == 3 and _finite(hist[0])
    plan = _plan("train", 2, 0)
    hnet = codec.load_homography_net() if source == "net" else None
    invalid = 0
    for (idx, _), (x1, x2, _), got in zip(plan, _want(plan, folder, "train"), rec.inputs):
        x1, x2 = x1.to(DEV), x2.to(DEV)
        assert torch.equal(got[0], x1.cpu()) and torch.equal(got[1], x2.cpu())
        if source == "net":
            xy = homography.window_origins(len(idx), None, 256, hnet.side * 8, 45, plan.rng)      # the epoch's stream, after the plan's draws
            want = homography.h_matrix_from_pair(hnet, x1, x2, xy)
        else:
            H, valid, _ = stereo_h.estimate_homography(x1, x2, pair_ids=idx)
            want = torch.where(valid.view(-1, 1, 1), H, torch.eye(3, device=DEV).expand_as(H))
            invalid += int((~valid).sum())
        assert torch.equal(got[2], want.cpu())
    assert hist[0]["invalid_homographies"] >= invalid and (source == "surf" or hist[0]["invalid_homographies"] == 0)

"""Supervised HomographyNet training on synthetic warps, on the GPU: ``HomographyTrainer.step_supervised`` / ``evaluate_supervised``,
``python -m hesic_amd.homography_train --supervision synthetic`` and ``python -m hesic_amd.homography_eval``.  The net is
``Net(patch_size=32)``, the smallest the trainer tests of tests/test_gpu_homography_net.py use."""
import functools
import json
import random

import numpy as np
import pytest
import torch

import homography_net_ref as R
import homography_train_ref as HT
from hesic_amd import codec, homography, homography_eval, homography_train, synthetic, train

pytestmark = pytest.mark.gpu
DEV = "cuda"


# ----------------------------------------------------------------------------------------------------------------- the trainer
def _inputs(B=4):
    """(patch_a, patch_b, delta): ``homography_net_ref.trainer_inputs`` with the deltas its ``patch_b`` was warped by as the label."""
    _, patch_a, patch_b, _ = R.trainer_inputs(B)
    return patch_a.to(DEV), patch_b.to(DEV), HT.deltas(710, B, 2.0).to(DEV)


def _trainer(P0=None, **kw):
    net = homography.Net(patch_size=32)
    net.load_state_dict(R.net_params(32) if P0 is None else P0)
    net = net.to(DEV)
    return net, train.HomographyTrainer(net, lr=1e-4, seed=0, **kw)


def _ulp_apart(a, b):
    """Largest distance in fp32 ulps between two positive fp32 tensors."""
    return int((a.cpu().contiguous().view(torch.int32).long() - b.cpu().contiguous().view(torch.int32).long()).abs().max())


def test_evaluate_supervised_is_the_eval_mode_forward():
    net, tr = _trainer()
    patch_a, patch_b, delta = _inputs()
    net.train()
    loss, err = tr.evaluate_supervised(patch_a, patch_b, delta)
    assert net.training and net.dropout_state() == (0, 0)               # the mode is left alone, no mask was consumed
    net.eval()
    with torch.no_grad():
        out = net(patch_a, patch_b)
    assert loss.shape == () and loss.is_cuda and torch.equal(loss, torch.nn.functional.mse_loss(out, delta))
    want = torch.linalg.vector_norm(out - delta, dim=-1).mean(-1)
    assert err.shape == (4,) and err.dtype == torch.float32 and err.is_cuda
    print(f"homography_supervised corner_error {err.tolist()} torch {want.tolist()} ulps apart {_ulp_apart(err, want)}")
    assert _ulp_apart(err, want) <= 1
    # delta_hat = 0: the mean corner norm of delta
    ident = homography.corner_error(torch.zeros_like(delta), delta)
    assert _ulp_apart(ident, delta.norm(dim=-1).mean(-1)) <= 1
    assert float(ident.mean()) > 0


def test_two_trainers_with_one_seed_take_the_same_steps():
    patch_a, patch_b, delta = _inputs()
    nets = []
    for _ in range(2):
        net, tr = _trainer()
        losses = []
        for _ in range(3):
            out = tr.step_supervised(patch_a, patch_b, delta)
            assert set(out) == {"loss"} and out["loss"].shape == () and out["loss"].is_cuda and not out["loss"].requires_grad
            losses.append(out["loss"].clone())
        assert net.dropout_state() == (0, 3) and net.training
        nets.append((net, losses))
    assert all(torch.equal(x, y) for x, y in zip(nets[0][1], nets[1][1]))
    for (k, p), q in zip(nets[0][0].named_parameters(), nets[1][0].parameters()):
        assert torch.equal(p, q), k
    assert not torch.equal(nets[0][0].fc[5].bias.cpu(), R.net_params(32)["fc.5.bias"])             # and the steps moved the parameters


def test_state_dict_round_trip_continues_bit_for_bit():
    patch_a, patch_b, delta = _inputs()
    net_a, tr_a = _trainer(clip_max_norm=0.5)
    la = []
    for _ in range(3):
        out = tr_a.step_supervised(patch_a, patch_b, delta)
        assert set(out) == {"loss", "grad_norm", "clip_coef", "skipped"}
        la.append(out["loss"].clone())
    net_b, tr_b = _trainer(clip_max_norm=0.5)
    lb = [tr_b.step_supervised(patch_a, patch_b, delta)["loss"].clone()]
    sd = tr_b.state_dict()
    assert sd["dropout"] == (0, 1)
    net_c, tr_c = _trainer(R.net_params(32, salt=1), clip_max_norm=0.5)
    tr_c.load_state_dict(sd)
    lb += [tr_c.step_supervised(patch_a, patch_b, delta)["loss"].clone() for _ in range(2)]
    assert all(torch.equal(x, y) for x, y in zip(la, lb)), (la, lb)
    for (k, p), q in zip(net_a.named_parameters(), net_c.parameters()):
        assert torch.equal(p, q), k
    assert net_a.dropout_state() == net_c.dropout_state() == (0, 3)


def test_twenty_steps_on_one_batch_lower_the_supervised_loss():
    patch_a, patch_b, delta = _inputs(4)
    net, tr = _trainer()
    first = float(tr.evaluate_supervised(patch_a, patch_b, delta)[0])
    for _ in range(20):
        tr.step_supervised(patch_a, patch_b, delta)
    final = float(tr.evaluate_supervised(patch_a, patch_b, delta)[0])
    print(f"homography_supervised descent: eval-mode MSE before {first:.6f}, after twenty steps {final:.6f}")
    assert final < first, (first, final)


def test_step_supervised_refuses_stream_capture(monkeypatch):
    net, tr = _trainer()
    before = {k: v.clone() for k, v in net.state_dict().items()}
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: True)
    with pytest.raises(RuntimeError, match="step_supervised is eager"):
        tr.step_supervised(*_inputs())
    assert net.dropout_state() == (0, 0) and all(torch.equal(v, before[k]) for k, v in net.state_dict().items())


# ------------------------------------------------------------------------------------------------------------ the folder command
def _write_pairs(root, split, first_seed, n, h, w):
    from PIL import Image
    x1, x2, _ = synthetic.stereo_batch(first_seed, n, h, w)
    for side, x in (("left", x1), ("right", x2)):
        d = root / split / side
        d.mkdir(parents=True, exist_ok=True)
        for i, img in enumerate(codec.quantise(x)):
            Image.fromarray(img).save(d / f"pair{i:02d}.png")


@pytest.fixture(scope="module")
def folder(tmp_path_factory):
    """6 + 2 small PNG pairs, and the runs on them, each made once."""
    base = tmp_path_factory.mktemp("supervised")
    root = base / "data"
    _write_pairs(root, "train", 100, 6, 48, 64)
    _write_pairs(root, "test", 200, 2, 48, 64)
    common = [str(root), "--picsize", "64", "--patchsize", "32", "--rho", "8", "--batch_size", "4", "--seed", "1"]

    @functools.lru_cache(maxsize=None)
    def run(name, *extra, epochs=2):
        logs, out = [], base / name
        hist = homography_train.main(common + ["--epochs", str(epochs), "--out", str(out), *extra], log=logs.append)
        assert [json.loads(line) for line in logs] == hist
        return hist, torch.load(out / "checkpoint.pth.tar", map_location="cpu"), out
    run.root, run.base, run.common = root, base, common
    return run


RECORD = ("epoch", "train_loss", "valid_loss", "best", "steps")
SYNTH = ("supervision", "valid_corner_error", "identity_corner_error", "valid_photometric")


def _same_checkpoint(tag, ca, cb, keys):
    assert set(ca) == set(cb) == keys, (tag, set(ca), set(cb))
    assert all(ca[k] == cb[k] for k in keys - {"state_dict", "optimizer"}), tag
    assert set(ca["state_dict"]) == set(cb["state_dict"])
    for k, v in ca["state_dict"].items():
        assert torch.equal(v, cb["state_dict"][k]), (tag, k)
    sa, sb = ca["optimizer"]["state"], cb["optimizer"]["state"]
    assert set(sa) == set(sb) and len(sa) > 0
    for i in sa:
        for k in ("step", "exp_avg", "exp_avg_sq"):
            assert torch.equal(sa[i][k], sb[i][k]), (tag, i, k)


PHOTO_KEYS = {"state_dict", "loss", "optimizer", "dropout", "epoch", "seed"}
SYNTH_KEYS = PHOTO_KEYS | {"supervision"}


def test_synthetic_training_is_the_same_from_device_and_stream(folder):
    (hd, cd, _), (hs, cs, _) = folder("dev", "--supervision", "synthetic", "--cache", "device"), \
        folder("str", "--supervision", "synthetic", "--cache", "stream")
    assert [r["epoch"] for r in hd] == [0, 1] and all(r["steps"] == 2 and r["supervision"] == "synthetic" for r in hd)
    assert [[r[k] for k in RECORD + SYNTH] for r in hd] == [[r[k] for k in RECORD + SYNTH] for r in hs]
    assert all(np.isfinite([r[k] for k in ("train_loss", "valid_loss") + SYNTH[1:]]).all() for r in hd)
    _same_checkpoint("device_vs_stream", cd, cs, SYNTH_KEYS)
    assert cd["supervision"] == "synthetic" and cd["loss"] == hd[1]["valid_loss"]
    # the identity's corner error does not depend on the net: the same validation deltas in every epoch, well above zero for rho = 8
    assert hd[0]["identity_corner_error"] == hd[1]["identity_corner_error"] > 1.0
    print("homography_supervised folder: " + " ".join(f"epoch {r['epoch']}: valid MSE {r['valid_loss']:.4f} corner error "
                                                      f"{r['valid_corner_error']:.4f} px (identity {r['identity_corner_error']:.4f})" for r in hd))


def test_synthetic_resume_equals_the_uninterrupted_run(folder):
    whole = folder("dev", "--supervision", "synthetic", "--cache", "device")
    _, _, out = folder("half", "--supervision", "synthetic", "--cache", "device", epochs=1)
    more, resumed, _ = folder("half", "--supervision", "synthetic", "--cache", "device", "--resume", str(out / "checkpoint.pth.tar"))
    assert [r["epoch"] for r in more] == [1] and [more[0][k] for k in RECORD + SYNTH] == [whole[0][1][k] for k in RECORD + SYNTH]
    _same_checkpoint("resumed", whole[1], resumed, SYNTH_KEYS)


def test_without_the_option_nothing_changes(folder):
    """The default is the photometric run: the records and the checkpoint of the explicit option, with the parent's keys -- and the
    parameters of one epoch made by hand from the unchanged pieces (``batches``, ``cached_inputs``, ``HomographyTrainer.step``)."""
    plain, named = folder("plain", "--cache", "device", epochs=1), folder("named", "--cache", "device", "--supervision", "photometric", epochs=1)
    assert set(plain[0][0]) == {"epoch", "train_loss", "valid_loss", "best", "steps", "seconds_per_step", "cache", "decode_seconds"}
    assert [[r[k] for k in RECORD] for r in plain[0]] == [[r[k] for k in RECORD] for r in named[0]]
    _same_checkpoint("default_vs_photometric", plain[1], named[1], PHOTO_KEYS)
    a = homography_train.parser().parse_args(folder.common + ["--cache", "device"])
    torch.manual_seed(1)
    net = homography.Net(patch_size=32).to(DEV)
    tr = train.HomographyTrainer(net, lr=a.learning_rate, seed=1)
    pairs = homography_train.list_pairs(folder.root, "train")
    cache = homography_train.build_cache(folder.root, "train", pairs, a)
    rng = random.Random("1/0")
    for items in homography_train.batches(pairs, 4, None, rng, True, False):
        tr.step(*homography_train.cached_inputs(cache, items, a, rng))
    by_hand = homography.checkpoint_state_dict(net)
    assert set(by_hand) == set(plain[1]["state_dict"])
    for k, v in by_hand.items():
        assert torch.equal(v, plain[1]["state_dict"][k]), k


def test_resume_across_supervisions_resets_the_best_loss(folder):
    """Synthetic pre-training, then photometric fine-tuning: the synthetic checkpoint's loss -- set to 0 here, lower than any photometric
    loss -- does not count, the first photometric epoch is the best one; and the other way round."""
    _, ckpt, _ = folder("half", "--supervision", "synthetic", "--cache", "device", epochs=1)
    pre = folder.base / "pretrained"
    pre.mkdir(exist_ok=True)
    torch.save(dict(ckpt, loss=0.0), pre / "checkpoint.pth.tar")
    hist, fine, _ = folder("fine", "--cache", "device", "--resume", str(pre / "checkpoint.pth.tar"))
    assert [r["epoch"] for r in hist] == [1] and hist[0]["best"] is True and "supervision" not in hist[0]
    assert set(fine) == PHOTO_KEYS and fine["loss"] == hist[0]["valid_loss"] > 0.0
    # the same file resumed under its own supervision keeps its loss: nothing beats 0
    same, _, _ = folder("same", "--supervision", "synthetic", "--cache", "device", "--resume", str(pre / "checkpoint.pth.tar"))
    assert same[0]["best"] is False
    # photometric -> synthetic: the supervised MSE (pixels squared) is far above the photometric loss, and still the best so far
    _, _, out = folder("plain", "--cache", "device", epochs=1)
    back, ck, _ = folder("back", "--supervision", "synthetic", "--cache", "stream", "--resume", str(out / "checkpoint.pth.tar"))
    assert back[0]["best"] is True and back[0]["valid_loss"] > torch.load(out / "checkpoint.pth.tar")["loss"] and ck["supervision"] == "synthetic"


# -------------------------------------------------------------------------------------------------------------------- evaluation
def test_homography_eval_lines_summary_and_batch_independence(folder):
    _, _, out = folder("dev", "--supervision", "synthetic", "--cache", "device")
    runs = {}
    for batch, cache in ((1, "device"), (4, "device"), (4, "stream")):
        logs = []
        recs = homography_eval.main([str(folder.root), "--checkpoint", str(out / "checkpoint.pth.tar"), "--split", "train", "--batch", str(batch),
                                     "--rho", "8", "--picsize", "64", "--patchsize", "32", "--seed", "3", "--cache", cache,
                                     "--out", str(folder.base / f"eval{batch}{cache}.json")], log=logs.append)
        assert [json.loads(line) for line in logs] == recs
        assert json.loads((folder.base / f"eval{batch}{cache}.json").read_text()) == recs[-1]
        runs[batch, cache] = recs
    recs = runs[1, "device"]
    lines, summary = recs[:-1], recs[-1]
    assert len(lines) == 6 and [r["stem"] for r in lines] == [f"pair{i:02d}" for i in range(6)]
    assert all(set(r) == {"stem", "corner_error", "identity_corner_error"} and r["corner_error"] > 0 and r["identity_corner_error"] > 0 for r in lines)
    err = np.array([r["corner_error"] for r in lines])
    assert summary["pairs"] == 6 and summary["mean_corner_error"] == float(err.mean()) and summary["median_corner_error"] == float(np.median(err))
    assert summary["under_1px"] == float((err < 1).mean()) and summary["under_3px"] == float((err < 3).mean())
    assert summary["identity_corner_error"] == float(np.mean([r["identity_corner_error"] for r in lines]))
    assert np.isfinite([summary["photometric_identity"], summary["photometric_net"]]).all() and summary["photometric_identity"] > 0
    print(f"homography_supervised eval: {summary}")
    # a pair's figures do not depend on the batch it is evaluated in, nor on the cache mode; the photometric means are per-batch means,
    # weighted by pairs: equal up to the rounding of the batches' means
    corner = ("pairs", "mean_corner_error", "median_corner_error", "identity_corner_error", "under_1px", "under_3px")
    for key in ((4, "device"), (4, "stream")):
        assert runs[key][:-1] == lines, key
        assert [runs[key][-1][k] for k in corner] == [summary[k] for k in corner]
        for k in ("photometric_identity", "photometric_net"):
            assert abs(runs[key][-1][k] - summary[k]) <= 1e-6 * summary[k], (key, k)
    assert runs[4, "device"][-1] == runs[4, "stream"][-1]
    # the synthetic weights load too
    synth = homography_eval.main([str(folder.root), "--checkpoint", "synthetic", "--rho", "8", "--picsize", "64", "--patchsize", "32"], log=lambda _: None)
    assert len(synth) == 3 and synth[-1]["pairs"] == 2

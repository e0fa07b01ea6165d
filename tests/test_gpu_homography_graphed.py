"""``train.GraphedHomographyTrainer``: the HomographyNet step as a HIP-graph replay with the dropout state on the device, bit for bit the
eager ``HomographyTrainer`` -- per kind of step, interleaved, under the step controls, across checkpoints -- and ``homography_train
--graphed`` against the run without the flag."""
import functools
import json

import pytest
import torch

import homography_net_ref as R
import homography_train_ref as HT
from hesic_amd import _lib as L
from hesic_amd import codec, homography, homography_train, synthetic, train

pytestmark = pytest.mark.gpu
DEV = "cuda"


# ----------------------------------------------------------------------------------------------------------------- the trainers
@functools.lru_cache(maxsize=None)
def _batch(kind, B=4, seed=0):
    """One call's arguments on the device: ``homography_net_ref.trainer_inputs`` for ``step``; for ``step_supervised`` its patches with the
    deltas ``patch_b`` was warped by as the label.  Made once per (kind, B, seed) and never written."""
    img_a, patch_a, patch_b, corners = (t.to(DEV) for t in R.trainer_inputs(B, seed))
    if kind == "step":
        return img_a, patch_a, patch_b, corners
    return patch_a, patch_b, HT.deltas(710 + seed, B, 2.0).to(DEV)


def _trainer(cls, P0=None, **kw):
    net = homography.Net(patch_size=32)
    net.load_state_dict(R.net_params(32) if P0 is None else P0)
    net = net.to(DEV)
    return net, cls(net, lr=1e-4, seed=0, **kw)


def _call(tr, kind, args):
    out = (tr.step if kind == "step" else tr.step_supervised)(*args)
    return {k: v.clone() for k, v in out.items()}


def _same_state(tag, a, b):
    (net_a, tr_a), (net_b, tr_b) = a, b
    for (k, p), q in zip(net_a.named_parameters(), net_b.parameters()):
        assert torch.equal(p, q), (tag, k)
    assert torch.equal(tr_a.optimizer.exp_avg, tr_b.optimizer.exp_avg), tag
    assert torch.equal(tr_a.optimizer.exp_avg_sq, tr_b.optimizer.exp_avg_sq), tag
    assert torch.equal(tr_a.optimizer.step_count, tr_b.optimizer.step_count), tag
    assert net_a.dropout_state() == net_b.dropout_state(), tag


def _same_outputs(tag, got, want):
    assert len(got) == len(want)
    for t, (x, y) in enumerate(zip(got, want)):
        assert set(x) == set(y), (tag, t)
        for k in x:
            assert torch.equal(x[k], y[k]) or (bool(torch.isnan(x[k])) and bool(torch.isnan(y[k]))), (tag, t, k, x[k], y[k])


@pytest.mark.parametrize("kind", ["step", "supervised"])
def test_six_steps_are_the_eager_trainers(kind):
    """warmup = 2: two eager steps, one capture and three replays, each on another batch."""
    eager, graphed = _trainer(train.HomographyTrainer), _trainer(train.GraphedHomographyTrainer, warmup=2)
    assert graphed[1].static_inputs(kind) is None and graphed[1].graph_slot(kind) is None
    le, lg = [], []
    for t in range(6):
        args = _batch(kind, 4, t % 3)
        le.append(_call(eager[1], kind, args))
        if t == 4:          # a producer that wrote into the slot's static tensors: nothing is staged
            static = graphed[1].static_inputs(kind)
            for dst, src in zip(static, args):
                dst.copy_(src)
            args = static
        lg.append(_call(graphed[1], kind, args))
        assert set(lg[-1]) == {"loss"} and lg[-1]["loss"].shape == () and lg[-1]["loss"].is_cuda
    slot = graphed[1].graph_slot(kind)
    assert slot.graph is not None and slot.calls == 6 and len(graphed[1]._slots) == 2          # the unused default slot and this kind's
    assert [tuple(t.shape) for t in graphed[1].static_inputs(kind)] == [tuple(t.shape) for t in _batch(kind)]
    _same_outputs(kind, lg, le)
    _same_state(kind, graphed, eager)
    assert graphed[0].dropout_state() == (0, 6) and graphed[1].state_dict()["dropout"] == (0, 6)
    assert len({float(x["loss"]) for x in lg}) > 3                           # the masks and the batches moved
    # evaluate after the replays sees the trained weights (stale packed weights / fc.2 copies would show)
    img_a, patch_a, patch_b, corners = _batch("step", 4, 1)
    assert torch.equal(graphed[1].evaluate(img_a, patch_a, patch_b, corners), eager[1].evaluate(img_a, patch_a, patch_b, corners))
    sup = _batch("supervised", 4, 1)
    for x, y in zip(graphed[1].evaluate_supervised(*sup), eager[1].evaluate_supervised(*sup)):
        assert torch.equal(x, y)
    # ... and so does one more replay after the eval forwards
    _same_outputs(kind + "/after eval", [_call(graphed[1], kind, _batch(kind, 4, 2))], [_call(eager[1], kind, _batch(kind, 4, 2))])
    _same_state(kind + "/after eval", graphed, eager)
    with pytest.raises(NotImplementedError, match="step_pairs"):
        graphed[1].step_pairs(None, None)


def test_the_two_kinds_interleaved_with_a_ragged_batch():
    """Each kind has its own graph; a B = 3 batch in the middle goes the eager route on the same device state, with no second capture."""
    eager, graphed = _trainer(train.HomographyTrainer), _trainer(train.GraphedHomographyTrainer, warmup=2)
    order = [("step", 4), ("supervised", 4), ("step", 4), ("supervised", 4), ("step", 4), ("supervised", 4), ("step", 4),
             ("step", 3), ("supervised", 3), ("supervised", 4), ("step", 4), ("supervised", 4), ("step", 3), ("step", 4)]
    le, lg = [], []
    for t, (kind, B) in enumerate(order):
        le.append(_call(eager[1], kind, _batch(kind, B, t % 3)))
        lg.append(_call(graphed[1], kind, _batch(kind, B, t % 3)))
    _same_outputs("interleaved", lg, le)
    _same_state("interleaved", graphed, eager)
    slots = {kind: graphed[1].graph_slot(kind) for kind in ("step", "supervised")}
    assert slots["step"].graph is not None and slots["supervised"].graph is not None and len(graphed[1]._slots) == 3
    assert (slots["step"].calls, slots["supervised"].calls) == (6, 5)          # the B = 3 calls are not the slots'
    assert graphed[1].static_inputs("step")[0].shape[0] == 4 and graphed[0].dropout_state() == (0, len(order))
    img_a, patch_a, patch_b, corners = _batch("step", 3, 0)
    assert torch.equal(graphed[1].evaluate(img_a, patch_a, patch_b, corners), eager[1].evaluate(img_a, patch_a, patch_b, corners))


def test_controls_under_replay():
    """clip + skip_nonfinite + live_lr: a NaN batch during the replays skips the step as a whole -- parameters and moments stay, the dropout
    step advances -- and ``set_lr`` takes effect on the next replay; both exactly as the eager trainer does."""
    kw = dict(clip_max_norm=0.5, skip_nonfinite=True, live_lr=True)
    eager, graphed = _trainer(train.HomographyTrainer, **kw), _trainer(train.GraphedHomographyTrainer, warmup=2, **kw)
    img_a, patch_a, patch_b, corners = _batch("step", 4, 0)
    bad = patch_b.clone()
    bad[1, 0, 3, 5] = float("nan")
    le, lg = [], []
    for t in range(7):
        args = (img_a, patch_a, bad if t == 3 else patch_b, corners)
        if t == 3:
            before = [{k: v.clone() for k, v in net.state_dict().items()} for net, _ in (eager, graphed)]
            moments = graphed[1].optimizer.exp_avg.clone(), graphed[1].optimizer.exp_avg_sq.clone(), graphed[1].optimizer.step_count.clone()
        if t == 5:
            eager[1].set_lr(5e-5)
            graphed[1].set_lr(5e-5)
        le.append(_call(eager[1], "step", args))
        lg.append(_call(graphed[1], "step", args))
        assert set(lg[-1]) == {"loss", "grad_norm", "clip_coef", "skipped"}
        if t == 3:
            for b4, (net, _) in zip(before, (eager, graphed)):
                assert all(torch.equal(v, b4[k]) for k, v in net.state_dict().items())
            opt = graphed[1].optimizer
            assert torch.equal(opt.exp_avg, moments[0]) and torch.equal(opt.exp_avg_sq, moments[1]) and torch.equal(opt.step_count, moments[2])
            assert graphed[0].dropout_state() == eager[0].dropout_state() == (0, 4)          # the mask was consumed all the same
    assert graphed[1].graph_slot("step").graph is not None
    assert [float(x["skipped"]) for x in lg] == [0, 0, 0, 1, 1, 1, 1] and not bool(torch.isfinite(lg[3]["grad_norm"]))
    _same_outputs("controls", lg, le)
    _same_state("controls", graphed, eager)
    # the new rate moved the parameters differently from a run that kept the old one
    keep = _trainer(train.GraphedHomographyTrainer, warmup=2, **kw)
    for t in range(7):
        keep[1].step(img_a, patch_a, bad if t == 3 else patch_b, corners)
    assert not torch.equal(keep[0].fc[5].bias, graphed[0].fc[5].bias)


def test_set_lr_without_controls_refuses_after_the_capture():
    net, tr = _trainer(train.GraphedHomographyTrainer, warmup=1)
    args = _batch("supervised")
    tr.set_lr(2e-4)                              # before the capture: the eager trainer's set_lr
    tr.step_supervised(*args)
    tr.set_lr(1e-4)
    tr.step_supervised(*args)                    # captures
    with pytest.raises(RuntimeError, match="by value"):
        tr.set_lr(5e-5)
    assert tr.optimizer.param_groups[0]["lr"] == 1e-4
    with pytest.raises(ValueError, match="warmup >= 1"):
        _trainer(train.GraphedHomographyTrainer, warmup=0)
    with pytest.raises(ValueError, match="kind is one of"):
        tr.static_inputs("pairs")
    assert tr.static_inputs("step") is None and tr.graph_slot("supervised").calls == 2


def test_checkpoints_move_between_the_eager_and_the_graphed_trainer():
    args = _batch("step")
    eager = _trainer(train.HomographyTrainer)
    want = [_call(eager[1], "step", args) for _ in range(6)]
    # graphed (two replays) -> eager
    g = _trainer(train.GraphedHomographyTrainer, warmup=2)
    got = [_call(g[1], "step", args) for _ in range(4)]
    sd = g[1].state_dict()
    assert set(sd) == {"state_dict", "optimizer", "dropout"} and sd["dropout"] == (0, 4) and isinstance(sd["dropout"], tuple)
    e2 = _trainer(train.HomographyTrainer, R.net_params(32, salt=1))
    e2[1].load_state_dict(sd)
    got += [_call(e2[1], "step", args) for _ in range(2)]
    _same_outputs("graphed->eager", got, want)
    _same_state("graphed->eager", e2, eager)
    # eager -> graphed
    e3 = _trainer(train.HomographyTrainer)
    got = [_call(e3[1], "step", args) for _ in range(2)]
    g2 = _trainer(train.GraphedHomographyTrainer, R.net_params(32, salt=1), warmup=1)
    g2[1].load_state_dict(e3[1].state_dict())
    assert g2[0].dropout_state() == (0, 2)
    got += [_call(g2[1], "step", args) for _ in range(4)]
    assert g2[1].graph_slot("step").graph is not None
    _same_outputs("eager->graphed", got, want)
    _same_state("eager->graphed", g2, eager)
    # a checkpoint loaded AFTER the capture is what the next replay continues from
    g2[1].load_state_dict(sd)
    _same_outputs("reload", [_call(g2[1], "step", args) for _ in range(2)], want[4:])
    _same_state("reload", g2, eager)


def test_net_launches_with_the_state_off_and_on():
    """Off (the default): the by-value entries, exactly.  On: one take, then the ``_state`` entries.  An eval-mode forward with grad
    (p = 0) needs no state and takes none."""
    net = homography.Net(patch_size=32)
    net.load_state_dict(R.net_params(32))
    net = net.to(DEV).train()
    _, patch_a, patch_b, _ = _batch("step")

    def launches():
        names = []
        with L.call_hook(lambda name, args: names.append(name)):
            with torch.enable_grad():
                out = net(patch_a, patch_b)
                out.sum().backward()
        return out.detach(), [n for n in names if "dropout" in n]

    net.set_dropout_state(5, 7)
    off, names = launches()
    assert [n for n in names if "forward" in n] == ["hesic_flatten_dropout_forward"] * 2
    assert not any("_state" in n for n in names) and net.dropout_state() == (5, 8)
    net.set_dropout_state(5, 7)
    assert net.dropout_on_device() is net and net.dropout_state() == (5, 7)
    on, names = launches()
    assert [n for n in names if "backward" not in n] == ["hesic_dropout_state_take"] + ["hesic_flatten_dropout_forward_state"] * 2
    assert not any(n in ("hesic_flatten_dropout_forward", "hesic_flatten_dropout_backward") for n in names)
    assert torch.equal(on, off) and net.dropout_state() == (5, 8)
    net.eval()
    _, names = launches()
    assert names.count("hesic_flatten_dropout_forward") == 2 and "hesic_dropout_state_take" not in names and net.dropout_state() == (5, 8)
    net.train()
    net.set_dropout_state(1 << 40, 0xFFFFFFFF)                                  # host and device copies; the counter wraps on the device
    launches()
    assert net.dropout_state() == (1 << 40, 0)
    net.dropout_on_device(False)                                                # the host copy takes over where the device stands
    assert net.dropout_state() == (1 << 40, 0)
    _, names = launches()
    assert not any("_state" in n for n in names) and net.dropout_state() == (1 << 40, 1)


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
    """22 + 2 small PNG pairs -- five full batches of four and a ragged one of two per epoch, so that a run with the default warm-up of
    three replays within one epoch -- and the runs on them, each made once."""
    base = tmp_path_factory.mktemp("graphed")
    root = base / "data"
    _write_pairs(root, "train", 100, 22, 64, 64)
    _write_pairs(root, "test", 200, 2, 64, 64)
    common = [str(root), "--picsize", "64", "--patchsize", "32", "--rho", "8", "--batch_size", "4", "--seed", "1"]

    @functools.lru_cache(maxsize=None)
    def run(name, *extra, epochs=2):
        logs, out = [], base / name
        hist = homography_train.main(common + ["--epochs", str(epochs), "--out", str(out), *extra], log=logs.append)
        assert [json.loads(line) for line in logs] == hist
        return hist, torch.load(out / "checkpoint.pth.tar", map_location="cpu"), torch.load(out / "checkpoint_best_loss.pth.tar", map_location="cpu"), out
    return run


RECORD = ("epoch", "train_loss", "valid_loss", "best", "steps")
SYNTH = ("supervision", "valid_corner_error", "identity_corner_error", "valid_photometric")


def _same_checkpoint(tag, ca, cb):
    assert set(ca) == set(cb), (tag, set(ca), set(cb))
    assert all(ca[k] == cb[k] for k in set(ca) - {"state_dict", "optimizer"}), tag
    assert set(ca["state_dict"]) == set(cb["state_dict"])
    for k, v in ca["state_dict"].items():
        assert torch.equal(v, cb["state_dict"][k]), (tag, k)
    sa, sb = ca["optimizer"]["state"], cb["optimizer"]["state"]
    assert set(sa) == set(sb) and len(sa) > 0
    for i in sa:
        for k in ("step", "exp_avg", "exp_avg_sq"):
            assert torch.equal(sa[i][k], sb[i][k]), (tag, i, k)
    assert ca["optimizer"]["param_groups"] == cb["optimizer"]["param_groups"], tag


@pytest.mark.parametrize("supervision", ["photometric", "synthetic"])
def test_graphed_folder_runs_are_the_plain_run(folder, supervision, monkeypatch):
    replays, replayed = [], train.GraphedHomographyTrainer._replayed
    monkeypatch.setattr(train.GraphedHomographyTrainer, "_replayed", lambda self: (replays.append(1), replayed(self))[1])
    sup, keys = ("--supervision", supervision), RECORD + (SYNTH if supervision == "synthetic" else ())
    plain = folder(f"plain-{supervision}", *sup, "--cache", "device")
    assert all(r["steps"] == 6 for r in plain[0]) and plain[1]["dropout"] == (1, 12)
    for cache in ("device", "stream"):
        got = folder(f"graphed-{cache}-{supervision}", *sup, "--cache", cache, "--graphed")
        assert [[r[k] for k in keys] for r in got[0]] == [[r[k] for k in keys] for r in plain[0]], cache
        assert [set(r) for r in got[0]] == [set(r) for r in plain[0]]
        _same_checkpoint(f"{cache}/last", got[1], plain[1])
        _same_checkpoint(f"{cache}/best", got[2], plain[2])
    # per run: ten full batches, of which three warm up; the capture and the six after it are graph launches; the ragged batches are eager
    assert len(replays) == 2 * 7


@pytest.mark.parametrize("supervision", ["photometric", "synthetic"])
def test_a_resume_may_flip_the_flag(folder, supervision):
    sup, keys = ("--supervision", supervision), RECORD + (SYNTH if supervision == "synthetic" else ())
    whole = folder(f"plain-{supervision}", *sup, "--cache", "device")
    for first, second in ((("--graphed",), ()), ((), ("--graphed",))):
        name = f"half-{'g' if first else 'e'}-{supervision}"
        half = folder(name, *sup, "--cache", "device", *first, epochs=1)
        more = folder(name, *sup, "--cache", "device", *second, "--resume", str(half[3] / "checkpoint.pth.tar"))
        assert [r["epoch"] for r in more[0]] == [1] and [more[0][0][k] for k in keys] == [whole[0][1][k] for k in keys]
        _same_checkpoint(f"{name}/last", more[1], whole[1])
        _same_checkpoint(f"{name}/best", more[2], whole[2])

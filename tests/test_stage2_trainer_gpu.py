"""``train.EnhancerTrainer`` / ``train.GraphedEnhancerTrainer`` on a real MI355X at B = 2, 128 x 128 (the size of the existing stage-2 test):
the two steps recorded from the reference (tests/golden/stage2_128.npz) under ``test_stage2_trainer_follows_the_reference_steps``'s bars, the
frozen model, eager against replay bit for bit, the step controls and the f16-inference / bf16-training switch.

The file name sorts behind the suite's other GPU files on purpose: these tests capture graphs and take streams from torch's round-robin pool,
and the one-rank RCCL captures of ``test_gpu_models.py`` / ``test_gpu_train_controls.py`` (which share that pool with the process group's stream)
keep the process history they always had."""
import math

import pytest
import torch

from conftest import load_golden
from hesic_amd import synthetic

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF, F16, F32 = torch.bfloat16, torch.float16, torch.float32
LAMBDA = 0.0067


@pytest.fixture(autouse=True)
def _bf16_then_reset():
    import hesic_amd
    hesic_amd.set_compute_dtype(BF)
    yield
    hesic_amd.set_compute_dtype(BF)
    hesic_amd.set_compute_dtype(F32)


def _models():
    from hesic_amd import models
    from test_oracle_golden import _en_params
    hs = models.HSIC()
    synthetic.fill_state_dict_(hs.state_dict())
    en = models.Independent_EN()
    en.load_state_dict(_en_params(), strict=True)
    return hs.to(DEV), en.to(DEV)


def _batch(seed=11):
    return tuple(t.to(DEV) for t in synthetic.stereo_batch(seed, 2, 128, 128))


def _bits(t):
    return t.detach().clone().view(torch.int32)


def _snapshot(tr):
    o = tr.optimizer
    return [_bits(t) for t in (tr.group.flat_p, o.exp_avg, o.exp_avg_sq, o.step_count)]


@pytest.mark.parametrize("dtype,tol_loss,tol_gn", [(F32, 2e-3, 2e-2), (BF, 3e-2, 0.15)], ids=["f32", "bf16"])
def test_enhancer_trainer_follows_the_reference_steps(dtype, tol_loss, tol_gn):
    """The quantities and the bars of ``test_stage2_trainer_follows_the_reference_steps``; the frozen model is untouched, and without controls a
    step issues one mirror launch, one Adam launch and no control launch (bf16: the fused criterion; the launch hook is thread-local and the
    backward pass runs on autograd's thread, so only the forward's ``hesic_en_loss`` is on the tape)."""
    import hesic_amd
    from hesic_amd import _lib as L
    from hesic_amd.train import EnhancerTrainer
    g = load_golden("stage2_128.npz")
    hesic_amd.set_compute_dtype(dtype)
    hs, en = _models()
    frozen = {k: p.detach().clone() for k, p in hs.named_parameters()}
    tr = EnhancerTrainer(hs, en, lr=1e-4, lmbda=LAMBDA)
    assert not tr.controls and tr.optimizer.ctl is None and tr.mirror_layers == 40
    x1, x2, Hm = _batch()
    bad = []
    for step in range(2):
        names = []
        with L.call_hook(lambda name, args: names.append(name)):
            c = tr.step(x1, x2, Hm)
        assert set(c) == {"loss", "mse_loss"} and not c["loss"].requires_grad
        assert names.count("hesic_c32_mirror_weights") == 1 and names.count("hesic_adam_step") == 1
        assert not [n for n in names if n in L._TRAIN_CTL_SIGS]
        assert names.count("hesic_en_loss") == (1 if dtype == BF else 0)
        print(f"enhancer_trainer {dtype} step {step}: loss {float(c['loss'])!r} ref {float(g[f'loss{step}'])!r}  "
              f"mse {float(c['mse_loss'])!r} ref {float(g[f'mse{step}'])!r}")
        assert float(c["loss"]) == pytest.approx(float(g[f"loss{step}"]), rel=tol_loss), step
        assert float(c["mse_loss"]) == pytest.approx(float(g[f"mse{step}"]), rel=tol_loss), step
        if step == 0:
            for name, p in en.named_parameters():
                gn, ref = float(p.grad.double().norm()), float(g["gn_" + name])
                if abs(gn - ref) > tol_gn * ref:
                    bad.append((name, gn, ref))
    assert not bad, bad[:6]
    for name, p in en.named_parameters():
        assert float(p.detach().double().norm()) == pytest.approx(float(g["pn_" + name]), rel=1e-4 if dtype == F32 else 2e-3), name
    # the compression model stayed frozen
    assert not hs.training and all(p.grad is None for p in hs.parameters())
    assert all(torch.equal(p.detach(), frozen[k]) for k, p in hs.named_parameters())


def test_six_graphed_steps_equal_six_eager_steps_bit_for_bit():
    import hesic_amd
    from hesic_amd.train import EnhancerTrainer, GraphedEnhancerTrainer
    hesic_amd.set_compute_dtype(BF)
    batches = [_batch(11), _batch(12)]
    snaps, losses = {}, {}
    for key, cls, kw in (("eager", EnhancerTrainer, {}), ("graphed", GraphedEnhancerTrainer, {"warmup": 3})):
        hs, en = _models()
        tr = cls(hs, en, lr=1e-4, lmbda=LAMBDA, **kw)
        losses[key] = []
        for step in range(6):
            c = tr.step(*batches[step % 2])
            losses[key].append(float(c["loss"]))
        torch.cuda.synchronize()
        snaps[key] = _snapshot(tr)
        if key == "graphed":
            assert tr.graph is not None and tr.calls == 6 and tr.static_inputs()[0].shape == (2, 3, 128, 128)
            assert not hs.training and all(p.grad is None for p in hs.parameters())
    print("eager", losses["eager"], "graphed", losses["graphed"])
    assert losses["eager"] == losses["graphed"]
    assert float(snaps["eager"][3].view(F32)) == 6.0
    for name, a, b in zip(("parameters", "exp_avg", "exp_avg_sq", "step"), snaps["eager"], snaps["graphed"]):
        assert torch.equal(a, b), f"{name}: {int((a != b).sum())} of {a.numel()} words differ"


CLIP = 1e-2        # far below the norm of the criterion's gradient at lambda * 255^2 ~ 436: every step is clipped


@pytest.fixture(scope="module")
def controlled():
    """A graphed trainer on the control path (clip + skip + live rate), warm-up 1, after three steps (one eager, the capture, one replay)."""
    import hesic_amd
    from hesic_amd.train import GraphedEnhancerTrainer
    hesic_amd.set_compute_dtype(BF)
    hs, en = _models()
    tr = GraphedEnhancerTrainer(hs, en, lr=1e-4, lmbda=LAMBDA, clip_max_norm=CLIP, skip_nonfinite=True, live_lr=True, warmup=1)
    stats = []
    for step in range(3):
        before = tr.optimizer.exp_avg.clone()
        c = tr.step(*_batch(11 + step % 2))
        torch.cuda.synchronize()
        stats.append({k: float(v) for k, v in c.items()} | {"buf": float(tr.group.flat_g.double().norm()),
                                                           "m_before": before, "m_after": tr.optimizer.exp_avg.clone(),
                                                           "g": tr.group.flat_g.clone()})
    return tr, stats


def test_a_binding_clip_scales_the_gradient_the_update_uses(controlled):
    tr, stats = controlled
    assert tr.graph is not None
    for s in stats:
        print({k: v for k, v in s.items() if not torch.is_tensor(v)})
        assert set(s) >= {"loss", "mse_loss", "grad_norm", "clip_coef", "skipped"}
        assert abs(s["grad_norm"] - s["buf"]) <= 1e-6 * s["buf"]                     # the buffer is left unscaled
        coef = float(torch.tensor(CLIP, dtype=F32) / (torch.tensor(s["grad_norm"], dtype=F32) + 1e-6))
        assert s["clip_coef"] == pytest.approx(coef, rel=1e-6) and s["clip_coef"] < 1.0 and s["skipped"] == 0.0
        # Adam's first moment took (1 - beta1) * coef * g: the update of the scaled gradient
        want = 0.9 * s["m_before"].double() + 0.1 * s["clip_coef"] * s["g"].double()
        torch.testing.assert_close(s["m_after"].double(), want, rtol=1e-5, atol=1e-12)


def test_a_nan_target_skips_the_step_as_a_whole_and_counts_it(controlled):
    tr, _ = controlled
    from hesic_amd import _lib as L
    x1, x2, Hm = _batch(11)
    before = _snapshot(tr)
    assert float(tr.optimizer.ctl[L.CTL_SKIPPED]) == 0.0
    poisoned = x2.clone()
    poisoned[1, 2, 37, 61] = float("nan")
    c = tr.step(x1, poisoned, Hm)
    torch.cuda.synchronize()
    assert float(c["skipped"]) == 1.0 and not math.isfinite(float(c["grad_norm"])) and math.isnan(float(c["loss"]))
    for a, b in zip(_snapshot(tr), before):
        assert torch.equal(a, b)
    c = tr.step(x1, x2, Hm)
    torch.cuda.synchronize()
    after = _snapshot(tr)
    assert float(c["skipped"]) == 1.0 and math.isfinite(float(c["grad_norm"]))
    assert float(after[3].view(F32)) == float(before[3].view(F32)) + 1
    assert bool(torch.isfinite(tr.group.flat_p).all()) and not torch.equal(after[0], before[0])


def test_set_lr_takes_effect_under_replay_with_live_lr_and_raises_without(controlled):
    tr, _ = controlled
    x1, x2, Hm = _batch(12)
    before = _snapshot(tr)
    tr.set_lr(0.0)
    tr.step(x1, x2, Hm)
    torch.cuda.synchronize()
    mid = _snapshot(tr)
    assert torch.equal(mid[0], before[0])                                             # rate 0: no parameter moved by a single bit
    assert float(mid[3].view(F32)) == float(before[3].view(F32)) + 1 and not torch.equal(mid[1], before[1])
    tr.set_lr(1e-4)
    tr.step(x1, x2, Hm)
    torch.cuda.synchronize()
    assert not torch.equal(_snapshot(tr)[0], mid[0])

    from hesic_amd.train import GraphedEnhancerTrainer
    hs, en = _models()
    plain = GraphedEnhancerTrainer(hs, en, lr=1e-4, lmbda=LAMBDA, warmup=1)
    plain.step(x1, x2, Hm)
    plain.set_lr(2e-4)                                                                # before the capture the rate is still the host's
    plain.step(x1, x2, Hm)
    assert plain.graph is not None
    with pytest.raises(RuntimeError, match="live_lr=True"):
        plain.set_lr(1e-4)
    assert plain.optimizer.param_groups[0]["lr"] == 2e-4


def test_f16_inference_with_bf16_training_leaves_the_compute_dtype_alone():
    import hesic_amd
    from hesic_amd import functional as Fn
    from hesic_amd.train import EnhancerTrainer
    hesic_amd.set_compute_dtype(F16)
    hs, en = _models()
    tr = EnhancerTrainer(hs, en, lr=1e-4, lmbda=LAMBDA)
    assert tr.train_dtype == BF
    x1, x2, Hm = _batch()
    c0 = tr.step(x1, x2, Hm)
    assert Fn.compute_dtype() == F16 and math.isfinite(float(c0["loss"]))
    epoch = Fn._cache_epoch
    c1 = tr.step(x1, x2, Hm)
    assert Fn._cache_epoch == epoch and Fn.compute_dtype() == F16
    assert float(c1["loss"]) < float(c0["loss"]) * 1.5
    with pytest.raises(ValueError, match="train_dtype"):
        EnhancerTrainer(hs, en, train_dtype=F16)


def test_replays_survive_an_eager_use_of_the_frozen_model_between_them():
    """A new pack-cache epoch followed by an eager forward of the frozen model (a validation pass of a user's loop) replaces -- and frees -- the
    model's cached packed weights, which a captured step reads by address.  The trainer notices the moved epoch, runs the next step eagerly
    and captures again; a plain replay leaves the epoch alone (it bumps the enhancer's version counters instead).  Four steps with such a pass
    in the middle must leave the eager trainer's bits."""
    from hesic_amd import functional as Fn
    from hesic_amd.train import EnhancerTrainer, GraphedEnhancerTrainer
    batches = [_batch(11), _batch(12)]
    snaps = {}
    for key, cls, kw in (("eager", EnhancerTrainer, {}), ("graphed", GraphedEnhancerTrainer, {"warmup": 1})):
        hs, en = _models()
        tr = cls(hs, en, lr=1e-4, lmbda=LAMBDA, **kw)
        for step in range(4):
            if step == 2:
                Fn.invalidate_weight_cache()
                with torch.no_grad():
                    hs(*batches[0])
            tr.step(*batches[step % 2])
        torch.cuda.synchronize()
        snaps[key] = _snapshot(tr)
        if key == "graphed":
            assert tr.graph is not None and tr.calls == 2          # re-captured: one eager step, then the capture
            epoch, versions = Fn._epoch_n, [p._version for p in tr.group.params]
            tr.step(*batches[0])                                   # a plain replay
            assert Fn._epoch_n == epoch and all(p._version > v for p, v in zip(tr.group.params, versions))
    for name, a, b in zip(("parameters", "exp_avg", "exp_avg_sq", "step"), snaps["eager"], snaps["graphed"]):
        assert torch.equal(a, b), f"{name}: {int((a != b).sum())} of {a.numel()} words differ"

"""Device-resident step controls (include/hesic_train_ctl.h) on the GPU: the two-launch gradient norm with its clip coefficient and
non-finite guard, the Adam update that reads rate / coefficient / decision from the control block against ``hesic_adam_step`` and
``torch.optim.Adam`` + ``clip_grad_norm_``, and ``Trainer`` / ``GraphedTrainer`` on the control path: reported values, eager against replay,
a learning rate changed under replay, a skipped step, the default path untouched.

Bars.  ``grad_norm``: the kernel sums fp64 squares (relative error ~ n * 2^-53), takes one correctly rounded fp64 root and rounds ONCE to fp32
(<= 2^-24 relative); the fp64 reference ``g.double().norm()`` carries ~1e-15: 1e-6 relative holds with a factor of ten to spare.
``clip_coef`` is the fp32 formula evaluated from the returned fp32 norm: equality.  Everything that compares the control-path update with
``hesic_adam_step`` on the same inputs is bit-exact."""
import ctypes as C
import os

import pytest
import torch

import memguard as MG
from hesic_amd import synthetic
from hesic_amd import _lib as L

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.fixture(autouse=True)
def _bf16_then_reset():
    import hesic_amd
    hesic_amd.set_compute_dtype(torch.bfloat16)
    yield
    hesic_amd.set_compute_dtype(torch.float32)


# ------------------------------------------------------------------------------------------------ helpers
def _ctl(lr=1e-3, max_norm=0.0, skip=0.0):
    """A control block as the host would write it, inside NaN guards."""
    b = [0.0] * L.CTL_FLOATS
    b[L.CTL_LR], b[L.CTL_MAX_NORM], b[L.CTL_SKIP_NONFINITE], b[L.CTL_CLIP_COEF], b[L.CTL_APPLIED] = lr, max_norm, skip, 1.0, 1.0
    return MG.guarded(torch.tensor(b, dtype=torch.float32, device=DEV), name="ctl")


def _partials():
    """Poisoned: every partial the second launch reads must have been written by the first."""
    return MG.guarded(torch.full((L.GRAD_NORM_MAX_BLOCKS,), float("nan"), dtype=torch.float64, device=DEV), name="partials")


def _norm(g, ctl, partials, also=None):
    L.call("hesic_grad_norm_ctl", L.ptr(g), g.numel(), L.ptr(partials), L.ptr(ctl), L.ptr(also), L.stream())


def _wide_values(n, seed):
    """Magnitudes 1e-20 ... 1e18 with random signs: fp32 squares of the small ones vanish, fp32 sums of the large ones' squares overflow."""
    gen = torch.Generator().manual_seed(seed)
    e = torch.rand(n, generator=gen, dtype=torch.float64) * 38.0 - 20.0
    e[0], e[-1] = -20.0, 18.0                                              # both ends of the range are present (one element: the upper)
    sign = torch.where(torch.rand(n, generator=gen) < 0.5, -1.0, 1.0).double()
    return (sign * 10.0 ** e).float()


def _coef(max_norm, norm):
    """torch.nn.utils.clip_grad_norm_'s coefficient, in fp32 tensors as torch evaluates it."""
    return torch.clamp(torch.tensor(max_norm, dtype=torch.float32) / (torch.tensor(norm, dtype=torch.float32) + 1e-6), max=1.0)


def _bits(t):
    return t.detach().clone().view(torch.int32 if t.dtype == torch.float32 else torch.int64).cpu()


# ------------------------------------------------------------------------------------------------ the norm kernel
@pytest.mark.parametrize("offset", [0, 4], ids=["aligned16", "one-element-later"])
@pytest.mark.parametrize("numel", [1, 3, 4096, 4097, 1024 * 4096 + 5])
def test_grad_norm_matches_fp64_and_is_reproducible(numel, offset):
    g = MG.guarded(_wide_values(numel, numel).to(DEV), name="g", offset=offset)
    assert g.data_ptr() % 16 == offset
    ref = float(g.double().norm())
    big = float(torch.tensor(0.5 * ref, dtype=torch.float32))             # an fp32 value: the block holds fp32
    outs = []
    for max_norm in (big, big, 4.0 * big, 0.0):                           # clipped (twice: reproducibility), norm below the bar, clipping off
        ctl, partials = _ctl(max_norm=max_norm, skip=1.0), _partials()
        _norm(g, ctl, partials)
        torch.cuda.synchronize()
        MG.check_all([g, ctl, partials])
        got = ctl.cpu()
        norm = float(got[L.CTL_GRAD_NORM])
        assert abs(norm - ref) <= 1e-6 * ref, (norm, ref)
        want = _coef(max_norm, norm) if max_norm > 0 else torch.tensor(1.0)
        assert float(got[L.CTL_CLIP_COEF]) == float(want), (float(got[L.CTL_CLIP_COEF]), float(want))
        assert float(got[L.CTL_APPLIED]) == 1.0 and float(got[L.CTL_SKIPPED]) == 0.0       # finite values, guard on: applied
        assert float(got[L.CTL_LR]) == float(torch.tensor(1e-3)) and float(got[L.CTL_MAX_NORM]) == max_norm       # inputs are left alone
        nb = min(L.GRAD_NORM_MAX_BLOCKS, -(-numel // 4096))
        assert bool(torch.isfinite(partials[:nb]).all()) and bool(torch.isnan(partials[nb:]).all())      # one partial per block, no more
        outs.append((_bits(ctl), _bits(partials[:nb])))
    assert float(outs[0][0].view(torch.float32)[L.CTL_CLIP_COEF]) < 1.0 and float(outs[2][0].view(torch.float32)[L.CTL_CLIP_COEF]) == 1.0
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])       # bit-identical from run to run
    assert torch.equal(outs[0][1], outs[2][1])


@pytest.mark.parametrize("bad", [float("nan"), float("inf")], ids=["nan", "inf"])
@pytest.mark.parametrize("numel,offset", [(3, 4), (4097, 0), (1024 * 4096 + 5, 4)])
def test_one_non_finite_element_at_the_end_decides_the_step(numel, offset, bad):
    v = _wide_values(numel, 7)
    v[-1] = bad
    g = MG.guarded(v.to(DEV), name="g", offset=offset)
    on, off, partials = _ctl(skip=1.0), _ctl(skip=0.0), _partials()
    _norm(g, on, partials)
    _norm(g, off, partials)
    follower, free = _ctl(skip=1.0), _ctl(skip=1.0)                         # a clean buffer of another group, tied / not tied to the first
    clean = MG.guarded(_wide_values(5, 9).to(DEV), name="clean")
    _norm(clean, follower, partials, also=on)
    _norm(clean, free, partials, also=off)
    _norm(g, on, partials)                                                  # a second skipped call counts up
    torch.cuda.synchronize()
    MG.check_all([g, on, off, partials, follower, free, clean])
    assert float(on[L.CTL_APPLIED]) == 0.0 and float(on[L.CTL_SKIPPED]) == 2.0 and not bool(torch.isfinite(on[L.CTL_GRAD_NORM]))
    assert float(off[L.CTL_APPLIED]) == 1.0 and float(off[L.CTL_SKIPPED]) == 0.0
    assert float(follower[L.CTL_APPLIED]) == 0.0 and float(follower[L.CTL_SKIPPED]) == 1.0 and bool(torch.isfinite(follower[L.CTL_GRAD_NORM]))
    assert float(free[L.CTL_APPLIED]) == 1.0 and float(free[L.CTL_SKIPPED]) == 0.0


def test_a_finite_gradient_beyond_the_fp32_norm_range_is_still_applied():
    g = MG.guarded(torch.full((4096,), 3.0e38, device=DEV), name="g")      # norm 1.9e40: finite in fp64, infinity once rounded to fp32
    ctl, partials = _ctl(max_norm=1.0, skip=1.0), _partials()
    _norm(g, ctl, partials)
    torch.cuda.synchronize()
    assert float(ctl[L.CTL_APPLIED]) == 1.0 and float(ctl[L.CTL_SKIPPED]) == 0.0
    assert float(ctl[L.CTL_GRAD_NORM]) == float("inf") and float(ctl[L.CTL_CLIP_COEF]) == 0.0


# ------------------------------------------------------------------------------------------------ Adam on the control path
SHAPES = [(128, 128, 5, 5), (128,), (3, 1, 1), (960, 960, 1, 1), (1,), (37, 5)] * 6          # test_multi_tensor_adam_matches_torch_adam's
NUMELS = [int(torch.Size(s).numel()) for s in SHAPES]
TOTAL = sum(NUMELS)                                                        # 7 989 102: not a multiple of the 4096-element block


def _flat(tag, scale_by_tensor=False, gain=1.0):
    parts = []
    for i, s in enumerate(SHAPES):
        t = synthetic._uniform(f"tc.{tag}.{i}", s, -1, 1).reshape(-1)
        parts.append(t * (10.0 ** (i % 5 - 3)) * gain if scale_by_tensor else t)
    return torch.cat(parts)


class _State:
    """p, m, v (guarded) and the step counter of one flat buffer."""

    def __init__(self, p0):
        self.p = MG.guarded(p0.to(DEV), name="p")
        self.m = MG.guarded(torch.zeros(TOTAL, device=DEV), name="m")
        self.v = MG.guarded(torch.zeros(TOTAL, device=DEV), name="v")
        self.step = torch.zeros((), dtype=torch.float32, device=DEV)

    def chunk(self, g, lr):
        c = L.AdamChunk()
        c.p[0], c.g[0], c.m[0], c.v[0], c.step[0], c.numel[0] = self.p.data_ptr(), g.data_ptr(), self.m.data_ptr(), self.v.data_ptr(), self.step.data_ptr(), TOTAL
        c.n, c.lr, c.beta1, c.beta2, c.eps = 1, lr, 0.9, 0.999, 1e-8
        return c

    def plain(self, g, lr):
        L.call("hesic_adam_step", C.byref(self.chunk(g, lr)), L.stream())

    def ctl_step(self, g, ctl):
        L.call("hesic_adam_step_ctl", C.byref(self.chunk(g, 123.0)), L.ptr(ctl), L.stream())           # chunk.lr is ignored

    def same_as(self, other):
        torch.cuda.synchronize()
        MG.check_all([self.p, self.m, self.v, other.p, other.m, other.v])
        return torch.equal(_bits(self.p), _bits(other.p)) and torch.equal(_bits(self.m), _bits(other.m)) and \
            torch.equal(_bits(self.v), _bits(other.v)) and float(self.step) == float(other.step)


@pytest.fixture(scope="module")
def p0():
    return _flat("p")


@pytest.mark.parametrize("clipped", [False, True], ids=["coef=1", "coef<1"])
def test_adam_ctl_is_bit_identical_to_adam_step(p0, clipped):
    """Three steps.  Unclipped: the same update as ``hesic_adam_step`` bit for bit.  Clipped: bit for bit ``hesic_adam_step`` fed the fp32
    products g * coef from memory -- the product is rounded once and never fused into the moment updates."""
    a, b, partials = _State(p0), _State(p0), _partials()
    for step in range(3):
        g = MG.guarded(_flat(f"g{step}", scale_by_tensor=True).to(DEV), name="g")
        g_before = _bits(g)
        max_norm = float(torch.tensor(0.25 * float(g.double().norm()) / (step + 1), dtype=torch.float32)) if clipped else 0.0
        ctl = _ctl(lr=1e-3, max_norm=max_norm)
        _norm(g, ctl, partials)
        a.ctl_step(g, ctl)
        coef = ctl[L.CTL_CLIP_COEF].clone()
        assert (float(coef) < 0.26 / (step + 1)) if clipped else (float(coef) == 1.0)
        b.plain(g * coef if clipped else g, 1e-3)
        assert a.same_as(b), step
        g.check()
        ctl.check()
        assert torch.equal(_bits(g), g_before)                             # the gradient buffer itself is not scaled
    assert float(a.step) == 3.0


def test_adam_ctl_with_clipping_follows_torch_adam_and_clip_grad_norm(p0):
    """Six steps against ``clip_grad_norm_`` + ``torch.optim.Adam`` on per-tensor parameters; the gradient grows from step to step, so
    does the clipping.  The bars are test_multi_tensor_adam_matches_torch_adam's."""
    a, partials = _State(p0), _partials()
    ps = [t.clone().reshape(s).to(DEV).requires_grad_() for t, s in zip(p0.split(NUMELS), SHAPES)]
    opt = torch.optim.Adam(ps, lr=1e-3)
    max_norm = float(torch.tensor(0.7 * float(_flat("h0", True).double().norm()), dtype=torch.float32))
    coefs = []
    for step in range(6):
        gf = _flat(f"h{step}", scale_by_tensor=True, gain=1.0 + 0.5 * step).to(DEV)
        for p, gp, s in zip(ps, gf.split(NUMELS), SHAPES):
            p.grad = gp.clone().reshape(s)
        torch.nn.utils.clip_grad_norm_(ps, max_norm)
        opt.step()
        ctl = _ctl(lr=1e-3, max_norm=max_norm, skip=1.0)
        _norm(gf, ctl, partials)
        a.ctl_step(gf, ctl)
        coefs.append(float(ctl[L.CTL_CLIP_COEF]))
    assert all(c < 1.0 for c in coefs) and len(set(coefs)) == 6, coefs
    torch.testing.assert_close(a.p, torch.cat([p.detach().reshape(-1) for p in ps]), rtol=2e-6, atol=2e-7)
    assert float(a.step) == 6.0


def test_adam_ctl_changes_nothing_when_the_step_is_not_applied(p0):
    a, partials = _State(p0), _partials()
    ok = _flat("k0", True).to(DEV)
    ctl = _ctl(lr=1e-3, skip=1.0)
    _norm(ok, ctl, partials)
    a.ctl_step(ok, ctl)                                                    # one applied step: non-trivial moments
    before = (_bits(a.p), _bits(a.m), _bits(a.v))
    bad = ok.clone()
    bad[-1] = float("nan")
    _norm(bad, ctl, partials)
    a.ctl_step(bad, ctl)
    torch.cuda.synchronize()
    MG.check_all([a.p, a.m, a.v, ctl])
    assert float(ctl[L.CTL_APPLIED]) == 0.0 and float(ctl[L.CTL_SKIPPED]) == 1.0
    assert float(a.step) == 1.0
    assert torch.equal(_bits(a.p), before[0]) and torch.equal(_bits(a.m), before[1]) and torch.equal(_bits(a.v), before[2])
    _norm(ok, ctl, partials)
    a.ctl_step(ok, ctl)                                                    # and the next clean one is applied again
    torch.cuda.synchronize()
    assert float(a.step) == 2.0 and float(ctl[L.CTL_SKIPPED]) == 1.0 and not torch.equal(_bits(a.p), before[0])


# ------------------------------------------------------------------------------------------------ Trainer / GraphedTrainer
CLIP = 1e-2        # far below the norm of the R-D gradient at lmbda * 255^2 ~ 436 on the synthetic weights: every step is clipped
CONTROLS = dict(clip_max_norm=CLIP, skip_nonfinite=True)
NAMES = ("encoder1.g_a_conv2.weight", "decoder2.after_conv.bias", "entropy_bottleneck1._biases.0", "entropy_bottleneck1.quantiles")


def _inputs():
    return tuple(t.to(DEV) for t in synthetic.stereo_batch(0, 2, 128, 128))


def _noise_for(step):
    shp = {"z1": (2, 128, 2, 2), "z2": (2, 128, 2, 2)}
    return {k: synthetic._uniform(f"gt.noise.{step}.{k}", shp.get(k, (2, 192, 8, 8)), -0.5, 0.5).to(DEV)
            for k in ("z1", "y1", "y1b", "y1w", "z2", "y2", "y2b")}


def _make(cls, **kw):
    from hesic_amd import models
    net = models.HSIC()
    synthetic.fill_state_dict_(net.state_dict())
    return cls(net.to(DEV), lr=1e-4, aux_lr=1e-3, lmbda=0.0067, **kw)


def _snapshot(tr):
    o, a = tr.optimizer, tr.aux_optimizer
    return [_bits(t) for t in (tr.main_group.flat_p, tr.aux_group.flat_p, o.exp_avg, o.exp_avg_sq, a.exp_avg, a.exp_avg_sq, o.step_count, a.step_count)]


@pytest.fixture(scope="module")
def runs():
    """Five steps of the eager and of the graphed trainer (warmup=1: steps 2-5 are replays) on the control path, with what each step
    reported next to the norm of the main flat gradient buffer read after the step."""
    import hesic_amd
    from hesic_amd.train import Trainer, GraphedTrainer
    hesic_amd.set_compute_dtype(torch.bfloat16)
    x1, x2, Hm = _inputs()
    out = {}
    for key, cls, kw in (("eager", Trainer, {}), ("graphed", GraphedTrainer, {"warmup": 1})):
        tr = _make(cls, **CONTROLS, **kw)
        trace, stats = [], []
        for step in range(5):
            c = tr.step(x1, x2, Hm, noise=_noise_for(step))
            trace.append([float(c["loss"]), float(c["bpp_loss"]), float(c["mse_loss"]), float(c["aux_loss"])])
            stats.append((float(c["grad_norm"]), float(c["clip_coef"]), float(c["skipped"]), float(tr.main_group.flat_g.double().norm())))
        out[key] = {"tr": tr, "trace": trace, "stats": stats,
                    "finals": {k: v.detach().float().clone() for k, v in tr.model.named_parameters() if k in NAMES}}
    return out


@pytest.mark.parametrize("key", ["eager", "graphed"])
def test_reported_norm_is_the_norm_of_the_unscaled_flat_gradient(runs, key):
    print(key, runs[key]["stats"])
    for norm, coef, skipped, buf in runs[key]["stats"]:
        assert abs(norm - buf) <= 1e-6 * buf, (norm, buf)                 # the buffer is left unscaled, so its norm is the reported one
        assert coef == float(_coef(CLIP, norm)) and coef < 1.0
        assert skipped == 0.0
    if key == "graphed":
        assert runs[key]["tr"].graph is not None


def test_graphed_trace_follows_the_eager_one_on_the_control_path(runs):
    """test_graphed_trainer_follows_the_eager_trace's bars (kind "hsic")."""
    for a, b in zip(runs["eager"]["trace"], runs["graphed"]["trace"]):
        for u, v in zip(a, b):
            assert u == pytest.approx(v, rel=2e-3), (runs["eager"]["trace"], runs["graphed"]["trace"])
    for k in NAMES:
        torch.testing.assert_close(runs["graphed"]["finals"][k], runs["eager"]["finals"][k], rtol=1e-2,
                                   atol=2 * 5 * 1e-3 if "entropy_bottleneck" in k else 2 * 5 * 1e-4 + 1e-4)


def test_a_replay_reads_the_learning_rate_from_the_device(runs):
    tr = runs["graphed"]["tr"]
    x1, x2, Hm = _inputs()
    before = _snapshot(tr)
    tr.set_lr(0.0, 0.0)
    tr.step(x1, x2, Hm, noise=_noise_for(5))
    torch.cuda.synchronize()
    mid = _snapshot(tr)
    assert torch.equal(mid[0], before[0]) and torch.equal(mid[1], before[1])           # rate 0: no parameter moved by a single bit
    assert float(tr.optimizer.step_count) == float(before[6].view(torch.float32)) + 1   # yet the step was applied (moments, counters)
    assert not torch.equal(mid[2], before[2])
    tr.set_lr(1e-4, 1e-3)
    tr.step(x1, x2, Hm, noise=_noise_for(6))
    torch.cuda.synchronize()
    after = _snapshot(tr)
    assert not torch.equal(after[0], mid[0]) and not torch.equal(after[1], mid[1])     # restored: parameters move again
    tr.optimizer.param_groups[0]["lr"] = 0.0                                           # a scheduler's way: plain mutation of param_groups
    tr.step(x1, x2, Hm, noise=_noise_for(7))
    torch.cuda.synchronize()
    last = _snapshot(tr)
    assert torch.equal(last[0], after[0]) and not torch.equal(last[1], after[1])       # main frozen, aux still at its own rate
    tr.set_lr(1e-4, 1e-3)


def test_loading_a_checkpoint_refreshes_the_rate_on_the_device(runs):
    """``FlatAdam.state_dict()`` keeps torch's format; a load on the control path also puts the checkpoint's rate into the control block."""
    opt = runs["graphed"]["tr"].optimizer
    sd = opt.state_dict()
    assert set(sd["state"][0]) == {"step", "exp_avg", "exp_avg_sq"} and sd["param_groups"][0]["lr"] == 1e-4
    moments = _bits(opt.exp_avg)
    sd["param_groups"][0]["lr"] = 5e-5
    opt.load_state_dict(sd)
    assert opt.param_groups[0]["lr"] == 5e-5 and float(opt.ctl[L.CTL_LR]) == float(torch.tensor(5e-5))
    assert torch.equal(_bits(opt.exp_avg), moments)
    runs["graphed"]["tr"].set_lr(1e-4)
    assert float(opt.ctl[L.CTL_LR]) == float(torch.tensor(1e-4))


def test_a_replay_with_a_nan_pixel_is_skipped_as_a_whole(runs):
    tr = runs["graphed"]["tr"]
    x1, x2, Hm = _inputs()
    before = _snapshot(tr)
    assert float(tr.aux_optimizer.ctl[L.CTL_SKIPPED]) == 0.0
    poisoned = x1.clone()
    poisoned[0, 1, 37, 61] = float("nan")
    c = tr.step(poisoned, x2, Hm, noise=_noise_for(8))
    torch.cuda.synchronize()
    assert float(c["skipped"]) == 1.0 and not bool(torch.isfinite(c["grad_norm"]))
    for a, b in zip(_snapshot(tr), before):                                            # parameters, moments, both step counts
        assert torch.equal(a, b)
    c = tr.step(x1, x2, Hm, noise=_noise_for(9))
    torch.cuda.synchronize()
    after = _snapshot(tr)
    assert float(c["skipped"]) == 1.0 and bool(torch.isfinite(c["grad_norm"]))
    assert float(after[6].view(torch.float32)) == float(before[6].view(torch.float32)) + 1
    assert float(after[7].view(torch.float32)) == float(before[7].view(torch.float32)) + 1
    assert bool(torch.isfinite(tr.main_group.flat_p).all()) and bool(torch.isfinite(tr.aux_group.flat_p).all())
    assert not torch.equal(after[0], before[0])


def test_defaults_issue_no_new_launch_and_a_captured_rate_cannot_be_set():
    """Without a control keyword a step is the launches it always was (two ``hesic_adam_step``, none of the new entry points); and once such a
    step is captured, ``set_lr`` refuses instead of being silently ignored by every replay."""
    from hesic_amd.train import GraphedTrainer
    x1, x2, Hm = _inputs()
    tr = _make(GraphedTrainer, warmup=1)
    assert not tr.controls and tr.optimizer.ctl is None and tr.aux_optimizer.ctl is None
    names = []
    with L.call_hook(lambda name, args: names.append(name)):
        c = tr.step(x1, x2, Hm, noise=_noise_for(0))                                   # the warm-up step: eager
    assert not [n for n in names if n in L._TRAIN_CTL_SIGS] and names.count("hesic_adam_step") == 2
    assert not {"grad_norm", "clip_coef", "skipped"} & set(c)
    tr.set_lr(2e-4, 2e-3)                                                              # before the capture the rate is still the host's
    names = []
    with L.call_hook(lambda name, args: names.append(name)):
        tr.step(x1, x2, Hm, noise=_noise_for(1))                                       # captured
    assert tr.graph is not None and not [n for n in names if n in L._TRAIN_CTL_SIGS]
    with pytest.raises(RuntimeError, match="live_lr=True"):
        tr.set_lr(1e-4)
    assert tr.optimizer.param_groups[0]["lr"] == 2e-4


def test_the_norm_is_taken_after_the_reduce(monkeypatch):
    """One RCCL rank with ``force_collectives``: in the eager warm-up step every all-reduce of the main group is issued before the norm's
    launches; in the replay the reported norm is that of the reduced buffer."""
    import torch.distributed as dist
    from hesic_amd.train import GraphedTrainer
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    os.environ.setdefault("MASTER_PORT", "29534")
    created = not dist.is_initialized()
    if created:
        dist.init_process_group("nccl", rank=0, world_size=1)
    try:
        x1, x2, Hm = _inputs()
        tr = _make(GraphedTrainer, warmup=1, force_collectives=True, bucket_mb=16.0, **CONTROLS)
        assert tr.main_reducer.active and len(tr.main_reducer.buckets) >= 4
        events, real = [], dist.all_reduce

        def logged(buf, *a, **kw):
            lo = buf.data_ptr()
            events.append("main" if tr.main_group.flat_g.data_ptr() <= lo < tr.main_group.flat_g.data_ptr() + 4 * tr.main_group.numel else "aux")
            return real(buf, *a, **kw)

        monkeypatch.setattr(dist, "all_reduce", logged)
        with L.call_hook(lambda name, args: events.append(name) if name in L._TRAIN_CTL_SIGS else None):
            tr.step(x1, x2, Hm, noise=_noise_for(0))
        assert events.count("main") == len(tr.main_reducer.buckets) and events.count("hesic_grad_norm_ctl") == 2
        first_norm = events.index("hesic_grad_norm_ctl")
        assert all(e == "main" for e in events[:first_norm]) and first_norm == len(tr.main_reducer.buckets)
        assert events[first_norm + 1] == "hesic_adam_step_ctl" and events[-2:] == ["hesic_grad_norm_ctl", "hesic_adam_step_ctl"]
        assert set(events[first_norm + 2:-2]) == {"aux"}
        monkeypatch.setattr(dist, "all_reduce", real)
        for step in (1, 2):
            c = tr.step(x1, x2, Hm, noise=_noise_for(step))
            buf = float(tr.main_group.flat_g.double().norm())
            assert abs(float(c["grad_norm"]) - buf) <= 1e-6 * buf and float(c["clip_coef"]) == float(_coef(CLIP, float(c["grad_norm"])))
        assert tr.graph is not None
    finally:
        if created:
            dist.destroy_process_group()

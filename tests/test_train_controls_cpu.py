"""Step controls of the trainer (clip_max_norm / skip_nonfinite / live_lr), host side: the new header against the ctypes table and the
two libraries' exports, the argument checks of the entry points, the constructor's refusals, and the host-module semantics (torch's
``clip_grad_norm_`` + an isfinite test around ``torch.optim.Adam``) against a hand-written loop.  No GPU."""
import copy
import ctypes as C
import os
import subprocess

import pytest
import torch


def _lib():
    from hesic_amd import _lib as L
    if not os.path.exists(L.LIB_PATH):
        import __graft_entry__ as ge
        ge.build()
    return L


# ------------------------------------------------------------------------------------------------ header, table, exports, argument checks
def test_header_declares_what_the_table_binds():
    L = _lib()
    declared = L.declared_symbols("hesic_train_ctl.h")
    assert declared == ["hesic_adam_step_ctl", "hesic_grad_norm_ctl"] and set(declared) == set(L._TRAIN_CTL_SIGS)
    assert not set(declared) & set(L.declared_symbols())                # a header of its own: include/hesic_hip.h does not list them
    text = open(L.header_path("hesic_train_ctl.h")).read()
    for name, value in (("LR", L.CTL_LR), ("MAX_NORM", L.CTL_MAX_NORM), ("SKIP_NONFINITE", L.CTL_SKIP_NONFINITE), ("GRAD_NORM", L.CTL_GRAD_NORM),
                        ("CLIP_COEF", L.CTL_CLIP_COEF), ("APPLIED", L.CTL_APPLIED), ("SKIPPED", L.CTL_SKIPPED), ("FLOATS", L.CTL_FLOATS)):
        assert f"#define HESIC_TRAIN_CTL_{name} {value} " in text, name
    assert f"#define HESIC_GRAD_NORM_MAX_BLOCKS {L.GRAD_NORM_MAX_BLOCKS}\n" in text


@pytest.mark.parametrize("fmt", ["bf16", "f16"])
def test_both_libraries_export_and_check_the_entry_points(fmt):
    L = _lib()
    l = L.lib(torch.float16 if fmt == "f16" else torch.bfloat16)
    assert l.hesic_abi_version() == 3
    exported = subprocess.check_output(["nm", "-D", "--defined-only", L.LIB_PATH_F16 if fmt == "f16" else L.LIB_PATH], text=True)
    for s in L._TRAIN_CTL_SIGS:
        assert f" T {s}\n" in exported, s
    p = C.c_void_p(4096)                                                 # never dereferenced: every call below is refused on the host
    for args in ((None, 16, p, p, None, None), (p, 16, None, p, None, None), (p, 16, p, None, None, None), (p, 0, p, p, None, None),
                 (p, -3, p, p, p, None)):
        assert l.hesic_grad_norm_ctl(*args) == -1, args
        assert b"grad_norm_ctl" in l.hesic_last_error()
    c = L.AdamChunk()
    c.n = 1
    c.p[0] = c.g[0] = c.m[0] = c.v[0] = c.step[0] = 4096
    c.numel[0] = 0
    assert l.hesic_adam_step_ctl(None, p, None) == -1 and b"adam_step_ctl" in l.hesic_last_error()
    assert l.hesic_adam_step_ctl(C.byref(c), None, None) == -1 and b"adam_step_ctl" in l.hesic_last_error()
    assert l.hesic_adam_step_ctl(C.byref(c), p, None) == -1 and b"adam_step_ctl" in l.hesic_last_error()          # numel = 0
    c.numel[0], c.m[0] = 8, None
    assert l.hesic_adam_step_ctl(C.byref(c), p, None) == -1 and b"adam_step_ctl" in l.hesic_last_error()          # a null tensor
    c.m[0], c.n = 4096, 0
    assert l.hesic_adam_step_ctl(C.byref(c), p, None) == -1 and b"adam_step_ctl" in l.hesic_last_error()          # an empty chunk


# ------------------------------------------------------------------------------------------------ a toy model with an aux group
class _Bottleneck(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.scale = torch.nn.Parameter(torch.linspace(0.5, 1.5, 16))           # main loss only, stepped by the aux optimiser
        self.quantiles = torch.nn.Parameter(torch.linspace(-1.0, 1.0, 16))      # aux loss only

    def forward(self, h):
        return h * self.scale


class _Net(torch.nn.Module):
    def __init__(self):
        super().__init__()
        torch.manual_seed(3)
        self.body = torch.nn.Sequential(torch.nn.Linear(5, 16), torch.nn.Tanh())
        self.shared = torch.nn.Linear(16, 16)                                   # used twice per forward
        self.head = torch.nn.Linear(16, 2)
        self.bottleneck = _Bottleneck()

    def parameters(self, recurse=True):
        for m in (self.body, self.shared, self.head):
            yield from m.parameters()

    def aux_parameters(self):
        yield from self.bottleneck.parameters()

    def aux_loss(self):
        return (self.bottleneck.quantiles - 0.25).abs().sum()

    def forward(self, x):
        return self.head(self.shared(torch.tanh(self.shared(self.bottleneck(self.body(x))))))


def _data():
    g = torch.Generator().manual_seed(4)
    return torch.randn(12, 5, generator=g), torch.randn(12, 2, generator=g) * 3.0


def _loss(net, x, y, gain=1.0):
    return ((net(x) - y) ** 2).mean() * gain


def _trainer(net, **kw):
    from hesic_amd.train import Trainer

    class ToyTrainer(Trainer):
        gain = 1.0

        def _forward_loss(self, x, y, _h, noise):
            return {"loss": _loss(self.model, x, y, self.gain)}

    return ToyTrainer(net, lr=1e-2, aux_lr=1e-1, **kw)


class _HandLoop:
    """The reference's order written out with torch alone: zero -> main backward -> clip_grad_norm_(parameters()) -> Adam -> aux backward ->
    aux Adam."""

    def __init__(self, net, max_norm):
        self.net, self.max_norm = net, max_norm
        self.opt = torch.optim.Adam(list(net.parameters()), lr=1e-2)
        self.aux = torch.optim.Adam(list(net.aux_parameters()), lr=1e-1)

    def step(self, x, y):
        self.opt.zero_grad()
        self.aux.zero_grad()
        _loss(self.net, x, y).backward()
        norm = torch.nn.utils.clip_grad_norm_(list(self.net.parameters()), self.max_norm)
        self.opt.step()
        self.net.aux_loss().backward()
        self.aux.step()
        return norm


def _first_norm():
    net = _Net()
    x, y = _data()
    _loss(net, x, y).backward()
    return float(torch.linalg.vector_norm(torch.stack([torch.linalg.vector_norm(p.grad) for p in net.parameters()])))


def _all_params(net):
    return [p.detach().clone() for p in list(net.parameters()) + list(net.aux_parameters())]


def _same_state(a, b):
    assert a["param_groups"] == b["param_groups"]
    assert a["state"].keys() == b["state"].keys()
    for k in a["state"]:
        for f, v in a["state"][k].items():
            assert torch.equal(torch.as_tensor(v), torch.as_tensor(b["state"][k][f])), (k, f)


# ------------------------------------------------------------------------------------------------ constructor refusals
@pytest.mark.parametrize("bad", [0, -1, -0.5, float("nan"), float("inf"), -float("inf")])
def test_clip_max_norm_must_be_finite_and_positive(bad):
    with pytest.raises(ValueError, match="clip_max_norm"):
        _trainer(_Net(), clip_max_norm=bad)


@pytest.mark.parametrize("kw", [{"skip_nonfinite": 1}, {"skip_nonfinite": "yes"}, {"live_lr": 0}, {"live_lr": None}, {"skip_nonfinite": 1.0}])
def test_flags_must_be_bools(kw):
    with pytest.raises(TypeError, match=next(iter(kw))):
        _trainer(_Net(), **kw)


def test_control_path_is_on_exactly_when_a_keyword_is_set():
    assert not _trainer(_Net()).controls
    assert _trainer(_Net(), clip_max_norm=2).controls and _trainer(_Net(), skip_nonfinite=True).controls and _trainer(_Net(), live_lr=True).controls
    c = _trainer(_Net()).step(*_data(), None)
    assert set(c) == {"loss", "aux_loss"}                                # the default step returns what it always did


# ------------------------------------------------------------------------------------------------ host semantics
def test_clipped_steps_land_exactly_where_the_hand_written_loop_lands():
    n0 = _first_norm()
    max_norm = 0.5 * n0                                                  # below the first step's norm: that step is clipped for sure
    x, y = _data()
    tr, ref = _trainer(_Net(), clip_max_norm=max_norm), _HandLoop(_Net(), max_norm)
    coefs = []
    for step in range(4):
        c = tr.step(x, y, None)
        norm = ref.step(x, y)
        assert float(c["grad_norm"]) == float(norm), step
        want = torch.clamp(max_norm / (norm + 1e-6), max=1.0)
        assert float(c["clip_coef"]) == float(want) and float(c["skipped"]) == 0.0
        coefs.append(float(want))
    assert coefs[0] == pytest.approx(0.5, rel=1e-4) and coefs[0] < 1.0
    for a, b in zip(_all_params(tr.model), _all_params(ref.net)):
        assert torch.equal(a, b)
    _same_state(tr.optimizer.state_dict(), ref.opt.state_dict())
    _same_state(tr.aux_optimizer.state_dict(), ref.aux.state_dict())


def test_a_non_finite_step_is_skipped_as_a_whole():
    x, y = _data()
    tr = _trainer(_Net(), skip_nonfinite=True)
    tr.step(x, y, None)
    before = _all_params(tr.model)
    sd, sd_aux = copy.deepcopy(tr.optimizer.state_dict()), copy.deepcopy(tr.aux_optimizer.state_dict())
    tr.gain = float("inf")
    c = tr.step(x, y, None)
    assert not bool(torch.isfinite(c["grad_norm"])) and float(c["skipped"]) == 1.0
    for a, b in zip(_all_params(tr.model), before):
        assert torch.equal(a, b)
    _same_state(tr.optimizer.state_dict(), sd)
    _same_state(tr.aux_optimizer.state_dict(), sd_aux)
    tr.gain = 1.0
    c = tr.step(x, y, None)                                              # the next clean step is applied
    assert float(c["skipped"]) == 1.0 and float(tr.optimizer.state_dict()["state"][0]["step"]) == 2.0
    assert any(not torch.equal(a, b) for a, b in zip(_all_params(tr.model), before))
    assert all(bool(torch.isfinite(p).all()) for p in _all_params(tr.model))


def test_without_the_guard_a_non_finite_step_is_applied_as_torch_would():
    x, y = _data()
    tr = _trainer(_Net(), live_lr=True)
    tr.gain = float("inf")
    c = tr.step(x, y, None)
    assert float(c["skipped"]) == 0.0 and float(tr.optimizer.state_dict()["state"][0]["step"]) == 1.0


def test_set_lr_changes_the_next_step():
    x, y = _data()
    tr, ref = _trainer(_Net(), live_lr=True), _HandLoop(_Net(), float("inf"))
    tr.step(x, y, None)
    ref.step(x, y)
    tr.set_lr(3e-3, 2e-2)
    ref.opt.param_groups[0]["lr"], ref.aux.param_groups[0]["lr"] = 3e-3, 2e-2
    assert tr.optimizer.param_groups[0]["lr"] == 3e-3 and tr.aux_optimizer.param_groups[0]["lr"] == 2e-2
    tr.step(x, y, None)
    ref.step(x, y)
    for a, b in zip(_all_params(tr.model), _all_params(ref.net)):
        assert torch.equal(a, b)
    before = _all_params(tr.model)
    tr.set_lr(0.0)                                                       # the aux rate is kept when it is not given
    assert tr.aux_optimizer.param_groups[0]["lr"] == 2e-2
    tr.step(x, y, None)
    after = _all_params(tr.model)
    n_main = len(list(tr.model.parameters()))
    assert all(torch.equal(a, b) for a, b in zip(after[:n_main], before[:n_main]))
    assert any(not torch.equal(a, b) for a, b in zip(after[n_main:], before[n_main:]))

"""HomographyNet in training mode, the part that needs no GPU: the reference of tests/homography_net_ref.py pinned against known answers,
the golden outputs and the oracle; torch's tie rule, which ``hesic_maxpool2_backward`` restates; the Linear kernels' bar model against
torch's own fp32 evaluation; the C ABI of include/hesic_homography_net.h with its argument checks; the errors of the public interface."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import conv_grad_ref as G
import homography_net_ref as R
from conftest import GOLDEN, T, load_golden
from hesic_amd import _lib as L
from hesic_amd import synthetic
from oracle import hesic_oracle as O


# ------------------------------------------------------------------------------------------------------------------------ Philox
@pytest.mark.parametrize("counter,key,want", [
    ((0, 0, 0, 0), (0, 0), "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
    ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, "408f276d 41c83b0e a20bc7c6 6d5451fd"),
    ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0), "d16cfe09 94fdcceb 5001e420 24126ea1"),
])
def test_philox_known_answers(counter, key, want):
    got = R.philox4x32_10(np.array(counter, dtype=np.uint64), key)
    assert " ".join(f"{int(v):08x}" for v in got) == want


def test_masks():
    m = R.keep_mask(3, 2048, 0.5, 7, 0, 0)
    frac = float(m.float().mean())
    assert 0.47 <= frac <= 0.53                                        # +-12 sigma of a fair coin over 6144 draws
    assert torch.equal(m, R.keep_mask(3, 2048, 0.5, 7, 0, 0))          # a function of its arguments
    for other in (R.keep_mask(3, 2048, 0.5, 7, 0, 1), R.keep_mask(3, 2048, 0.5, 7, 1, 0), R.keep_mask(3, 2048, 0.5, 8, 0, 0),
                  R.keep_mask(3, 2048, 0.5, 7 + (1 << 32), 0, 0)):
        assert 0.4 < float((other != m).float().mean()) < 0.6          # another site / step / seed (low and high word): an independent mask
    assert bool(R.keep_mask(2, 64, 0.0, 1, 2, 3).all())                # p = 0 keeps everything
    assert R.thr_scale(0.0) == (0, 1.0) and R.thr_scale(0.5) == (1 << 31, 2.0)
    assert R.thr_scale(0.3)[1] == float(np.float32(1.0) / (np.float32(1.0) - np.float32(0.3)))
    # the package derives the same kernel arguments
    from hesic_amd import functional as Fn
    for p in (0.0, 0.3, 0.5, 0.999):
        assert Fn.dropout_args(p, 5, 6, 1) == (*R.thr_scale(p), 5, 6, 1)
    for p in (-0.1, 1.0, 1.5, 0.999999999):          # the last one is 1.0f
        with pytest.raises(ValueError):
            Fn.dropout_args(p)


def test_flatten_dropout_reference():
    x = synthetic._uniform("fd.cpu", (2, 8, 3, 4), -1, 1)
    assert torch.equal(R.flatten_dropout(x, 0.0, 3, 1, 0), x.reshape(2, -1))
    y = R.flatten_dropout(x, 0.3, 3, 1, 0)
    keep = R.keep_mask(2, 96, 0.3, 3, 1, 0)
    assert torch.equal(y[~keep], torch.zeros(int((~keep).sum()))) and torch.equal(y[keep], x.reshape(2, -1)[keep] * np.float32(R.thr_scale(0.3)[1]))
    g = synthetic._uniform("fd.cpu.g", (2, 96), -1, 1)
    xl = x.clone().requires_grad_()
    (ga,) = torch.autograd.grad(xl.reshape(2, -1) * (keep.float() * R.thr_scale(0.3)[1]), xl, g)
    assert torch.equal(R.flatten_dropout_backward(g, x.shape, 0.3, 3, 1, 0), ga)


# ------------------------------------------------------------------------------------------------------------------ restatement
def _golden_params():
    shapes = [l.split() for l in open(os.path.join(GOLDEN, "homo_state_keys.txt"))]
    return synthetic.fill_homography_state_dict_({s[0]: torch.empty([int(v) for v in s[1:]]) for s in shapes})


def test_restatement_matches_golden_and_oracle():
    P = _golden_params()
    assert {k: tuple(v.shape) for k, v in R.net_params(128).items()} == {k: tuple(v.shape) for k, v in P.items()}
    assert all(torch.equal(v, P[k]) for k, v in R.net_params(128).items())
    a, b, _ = synthetic.homography_batch(0, 2)
    delta = R.net_forward({k: v.double() for k, v in P.items()}, a, b)
    assert float((delta - T(load_golden("homo.npz")["delta"]).double()).abs().max()) < 2e-4
    assert float((delta - O.homography_net(P, a, b).double()).abs().max()) < 2e-4
    assert torch.equal(R.net_forward(P, a, b, dtype=torch.float32), O.homography_net(P, a, b))
    # other patch sizes, and train mode is eval mode times the masks
    P32 = R.net_params(32)
    a, b, _ = synthetic.homography_batch(1, 3, patch=32)
    assert R.net_forward(P32, a, b, dtype=torch.float32).shape == (3, 4, 2)
    ones = [torch.ones(3, 2048), torch.ones(3, 1024)]
    assert torch.equal(R.net_forward(P32, a, b, ones, torch.float32), R.net_forward(P32, a, b, None, torch.float32))
    m = R.net_masks(3, 32, 5, 0)
    assert m[0].shape == (3, 2048) and m[1].shape == (3, 1024) and set(m[0].unique().tolist()) == {0.0, 2.0}
    assert not torch.equal(R.net_forward(P32, a, b, m, torch.float32), R.net_forward(P32, a, b, None, torch.float32))


# --------------------------------------------------------------------------------------------------------------------- tie rule
def first_max_backward(x, gy):
    """The stated rule, spelled out: scan (0,0), (0,1), (1,0), (1,1); a later element wins only if strictly greater; everything else zero."""
    B, Cc, H, W = x.shape
    gx = torch.zeros_like(x)
    for wy in range(H // 2):
        for wx in range(W // 2):
            win = x[:, :, 2 * wy:2 * wy + 2, 2 * wx:2 * wx + 2].reshape(B, Cc, 4)
            best, arg = win[..., 0].clone(), torch.zeros(B, Cc, dtype=torch.long)
            for pos in range(1, 4):
                up = win[..., pos] > best
                best, arg = torch.where(up, win[..., pos], best), torch.where(up, torch.full_like(arg, pos), arg)
            for pos in range(4):
                gx[:, :, 2 * wy + pos // 2, 2 * wx + pos % 2] = torch.where(arg == pos, gy[:, :, wy, wx], torch.zeros(()))
    return gx


@pytest.mark.parametrize("shape", [(3, 64, 10, 12), (1, 4, 7, 5), (2, 8, 6, 9)])
def test_torch_max_pool_tie_rule(shape):
    x = R.pool_input(shape, f"mp.tie{shape}")
    assert float((x == 0).float().mean()) >= 0.3
    gy = synthetic._uniform(f"mp.tie.g{shape}", (shape[0], shape[1], shape[2] // 2, shape[3] // 2), -1, 1)
    xl = x.clone().requires_grad_()
    (ga,) = torch.autograd.grad(F.max_pool2d(xl, 2, 2), xl, gy)
    want = first_max_backward(x, gy)
    assert torch.equal(ga, want)
    assert float(want[:, :, 0, 0].abs().min()) > 0 and float(want[:, :, :2, :2].abs().sum((2, 3)).min()) > 0      # the all-zero window: (0,0) gets it
    if shape[2] % 2:
        assert not bool(ga[:, :, -1].any())
    if shape[3] % 2:
        assert not bool(ga[:, :, :, -1].any())


# -------------------------------------------------------------------------------------------------------------------- bar model
@pytest.mark.parametrize("act", [G.ACT_NONE, G.ACT_RELU], ids=["none", "relu"])
@pytest.mark.parametrize("tag", sorted(R.LINEAR_CASES))
def test_torch_fp32_linear_is_inside_the_bars(tag, act):
    """The bars admit a correct implementation: every element of torch's fp32 ``F.linear`` + autograd is inside its bar (8 x the unit bound).
    Its largest ratio to the unit bound over all cases is 1.39 (dW of the two-row case, where n = B = 2 leaves the bound at one rounding)."""
    got = R.linear_torch_fp32(tag, act)
    ref = R.linear_reference(tag, act, y_saved=got["y"])
    ref["y16"] = ref["dx16"] = False                      # torch stores fp32 here
    worst = 0.0
    for q in ("y", "dx", "dw", "db"):
        ok, ratio, msg = G.check(ref, q, got[q])
        worst = max(worst, ratio)
        assert ok, msg
    print(f"homography_net_parity torch_fp32 {tag} act={act} max ratio {worst:.3f}")
    if act == G.ACT_RELU:                                 # ReLU kills whole outputs: their gradient terms vanish and the bar is 0 there
        assert bool((ref["S"]["dx"] >= 0).all()) and float((ref["g"] == 0).float().mean()) > 0.2


# -------------------------------------------------------------------------------------------------------------------------- ABI
@pytest.mark.parametrize("fmt", ["bf16", "f16"])
def test_abi_header_bindings_exports(fmt):
    declared = L.declared_symbols("hesic_homography_net.h")
    assert declared == ["hesic_bias_grad", "hesic_flatten_dropout_backward", "hesic_flatten_dropout_forward", "hesic_linear_dgrad",
                        "hesic_linear_forward", "hesic_linear_forward_ws_bytes", "hesic_linear_wgrad", "hesic_maxpool2_backward",
                        "hesic_narrow_in_wgrad"]
    assert set(declared) == set(L._HOMOGRAPHY_NET_SIGS)
    assert not set(declared) & set(L.declared_symbols())                # a header of its own: include/hesic_hip.h does not list them
    assert f"#define HESIC_LINEAR_MAX_ROWS {L.LINEAR_MAX_ROWS}\n" in open(L.header_path("hesic_homography_net.h")).read()
    assert f"#define HESIC_DET_MAX_BLOCKS {L.DET_MAX_BLOCKS}\n" in open(L.header_path("hesic_homography_net.h")).read()
    assert "#define HESIC_ABI_VERSION 3" in open(L.header_path("hesic_hip.h")).read() and L.ABI_VERSION == 3
    exported = subprocess.check_output(["nm", "-D", "--defined-only", L.LIB_PATH_F16 if fmt == "f16" else L.LIB_PATH], text=True)
    for s in declared:
        assert f" T {s}\n" in exported, s


@pytest.mark.parametrize("fmt", [torch.bfloat16, torch.float16], ids=["bf16", "f16"])
def test_bad_arguments_are_errors_not_launches(fmt):
    """Every refusal happens on the host, before any HIP call: this runs without a GPU."""
    lib = L.lib(fmt)
    p = C.c_void_p(256)          # never dereferenced: the checks fail first

    def refused(rc, *words):
        msg = lib.hesic_last_error().decode()
        assert rc != 0 and all(w in msg for w in words), (rc, msg)

    ws = lib.hesic_linear_forward_ws_bytes
    assert ws(4, 2048, 1024) > 0 and ws(65, 2048, 1024) == 0
    assert ws(2, 2048, 1024) * 2 == ws(4, 2048, 1024)
    refused(lib.hesic_linear_forward(p, p, p, p, 65, 2048, 1024, 0, L.F32, p, 1 << 30, None), "linear_forward", "B=65")
    refused(lib.hesic_linear_forward(p, p, p, p, 0, 2048, 1024, 0, L.F32, p, 1 << 30, None), "B=0")
    refused(lib.hesic_linear_forward(p, p, p, p, 4, 2050, 1024, 0, L.F32, p, 1 << 30, None), "In=2050")
    refused(lib.hesic_linear_forward(p, p, p, p, 4, 2048, 0, 0, L.F32, p, 1 << 30, None), "Out=0")
    refused(lib.hesic_linear_forward(None, p, p, p, 4, 2048, 1024, 0, L.F32, p, 1 << 30, None), "null")
    refused(lib.hesic_linear_forward(p, p, p, p, 4, 2048, 1024, 0, L.F32, None, 0, None), "null")
    refused(lib.hesic_linear_forward(p, p, p, p, 4, 2048, 1024, 0, L.F32, p, 16, None), "workspace")
    refused(lib.hesic_linear_forward(p, p, p, p, 4, 2048, 1024, L.ACT_LEAKY, L.F32, p, 1 << 30, None), "act=2")
    refused(lib.hesic_linear_forward(p, p, p, p, 4, 2048, 1024, 0, 7, p, 1 << 30, None), "dtype")
    refused(lib.hesic_linear_forward(p, p, p, p, 1, 65537 * 1024, 1, 0, L.F32, p, 1 << 30, None), "too large")
    refused(lib.hesic_linear_dgrad(p, p, p, 65, 2048, 1024, L.F32, None), "linear_dgrad", "B=65")
    refused(lib.hesic_linear_dgrad(p, p, p, 4, 2046, 1024, L.F32, None), "In=2046")
    refused(lib.hesic_linear_dgrad(p, None, p, 4, 2048, 1024, L.F32, None), "null")
    refused(lib.hesic_linear_wgrad(p, p, p, p, 65, 2048, 1024, 0, L.F32, None), "linear_wgrad", "B=65")
    refused(lib.hesic_linear_wgrad(p, p, p, p, 4, 2049, 1024, 0, L.F32, None), "In=2049")
    refused(lib.hesic_linear_wgrad(p, p, None, p, 4, 2048, 1024, 0, L.F32, None), "null")
    for fn, name in ((lib.hesic_flatten_dropout_forward, "flatten_dropout_forward"), (lib.hesic_flatten_dropout_backward, "flatten_dropout_backward")):
        refused(fn(p, p, 2, 1, 6, 0, 1.0, 0, 0, 0, L.F32, None), name, "multiple of 4")          # F = 6
        refused(fn(p, p, 2, 3, 6, 0, 1.0, 0, 0, 0, L.F32, None), "multiple of 4")                # F = 18
        refused(fn(p, p, 2, 4, 6, 0, 1.0, 0, 0, 0, L.F32, None), "C=6")                          # F = 24 but C % 4 != 0
        refused(fn(None, p, 2, 4, 8, 0, 1.0, 0, 0, 0, L.F32, None), "null")
        refused(fn(p, None, 2, 4, 8, 0, 1.0, 0, 0, 0, L.F32, None), "null")
        refused(fn(p, p, 0, 4, 8, 0, 1.0, 0, 0, 0, L.F32, None), "B=0")
    refused(lib.hesic_maxpool2_backward(p, p, p, 2, 8, 8, 6, L.F32, None), "maxpool2_backward", "C=6")      # vector width 4 (fp32)
    refused(lib.hesic_maxpool2_backward(p, p, p, 2, 8, 8, 12, L.H16, None), "C=12")                         # vector width 8 (16-bit)
    refused(lib.hesic_maxpool2_backward(p, None, p, 2, 8, 8, 8, L.F32, None), "null")
    refused(lib.hesic_maxpool2_backward(p, p, None, 2, 8, 8, 8, L.F32, None), "null")
    refused(lib.hesic_maxpool2_backward(p, p, p, 2, 1, 8, 8, L.F32, None), "H=1")
    refused(lib.hesic_bias_grad(p, p, p, 100, 48, 0, L.F32, None), "bias_grad", "C=48")
    refused(lib.hesic_bias_grad(p, None, p, 100, 64, 0, L.F32, None), "null")
    refused(lib.hesic_narrow_in_wgrad(p, p, p, p, 2, 3, 8, 8, 64, 0, L.F32, None), "narrow_in_wgrad", "Cin=3")
    refused(lib.hesic_narrow_in_wgrad(p, p, p, None, 2, 2, 8, 8, 64, 0, L.F32, None), "null")
    refused(lib.hesic_narrow_in_wgrad(p, p, p, p, 2, 2, 8, 8, 48, 0, L.F32, None), "Cout=48")


# ----------------------------------------------------------------------------------------------------------------------- errors
def test_public_interface_errors():
    from hesic_amd import homography, train
    net = homography.Net(patch_size=32)
    a = torch.zeros(1, 1, 32, 32)
    with pytest.raises(RuntimeError, match="no CPU fallback"):          # unchanged: inference ...
        with torch.no_grad():
            net.eval()(a, a)
    with pytest.raises(RuntimeError, match="no CPU fallback"):          # ... and now the training route too
        net.train()(a, a)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        net.eval()(a, a)
    with pytest.raises(NotImplementedError, match="float32"):
        homography.Net(patch_size=32, dtype=torch.bfloat16).train()(a, a)
    net.fc[1].p = 1.0
    with pytest.raises(ValueError, match=r"\[0, 1\)"):
        net.train()(a, a)
    assert net.dropout_state() == (0, 0)
    net.set_dropout_state(11, 5)
    assert net.dropout_state() == (11, 5)
    assert "inference-only" not in (homography.__doc__ + homography.Net.forward.__doc__ if homography.Net.forward.__doc__ else homography.__doc__)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        train.HomographyTrainer(homography.Net(patch_size=32))
    with pytest.raises(NotImplementedError):
        train.HomographyTrainer(homography.Net(patch_size=32, dtype=torch.bfloat16))
    with pytest.raises(ValueError):
        train.HomographyTrainer(homography.Net(patch_size=32), clip_max_norm=-1.0)


# ---------------------------------------------------------------------------------------------------------------------- descent
def test_reference_descends_with_margin():
    """The GPU descent test's premise, on the reference itself: 30 Adam steps (lr 1e-4) on one fixed batch with the masks of seed 0 take the
    fp32 loop's eval loss well below where it started, and the fp64 loop agrees."""
    inputs = R.trainer_inputs()
    P0 = R.net_params(32)
    L0 = R.eval_loss(P0, inputs)
    l32, P32 = R.train_loop(P0, inputs, 30, 1e-4, 0, dtype=torch.float32)
    l64, P64 = R.train_loop(P0, inputs, 30, 1e-4, 0, dtype=torch.float64)
    Lr, Lr64 = R.eval_loss(P32, inputs), R.eval_loss(P64, inputs)
    print(f"homography_net_parity descent_reference L0 {L0:.6f} fp32 {Lr:.6f} fp64 {Lr64:.6f} first-step |fp32 - fp64| {abs(l32[0] - l64[0]):.2e}")
    assert Lr <= 0.8 * L0 and abs(Lr - Lr64) <= 0.05 * (L0 - Lr64)

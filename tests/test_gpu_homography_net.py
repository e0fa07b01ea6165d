"""HomographyNet in training mode on the GPU (include/hesic_homography_net.h, functional._MaxPool2Fn / _FlattenDropoutFn / _LinearFn,
homography.Net with grad, train.HomographyTrainer) against tests/homography_net_ref.py.  Every parity test prints
``homography_net_parity <case> <errors>`` before it asserts; the values measured when the tests were written are in
profiles/homography_net_parity.json."""
import contextlib

import pytest
import torch
import torch.nn.functional as F

import conv_grad_ref as G
import homography_net_ref as R
import homography_train_ref as HT
from conftest import T, load_golden
from hesic_amd import _lib as L
from hesic_amd import functional as Fn
from hesic_amd import homography, synthetic, train

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _nhwc(x):
    return x.to(DEV).contiguous(memory_format=torch.channels_last)


# ------------------------------------------------------------------------------------------------------------------- max pool
@pytest.mark.parametrize("shape,h16", [((3, 64, 10, 12), False), ((1, 4, 7, 5), False), ((2, 8, 6, 9), True)], ids=["f32_3x64x10x12", "f32_1x4x7x5", "h16_2x8x6x9"])
def test_maxpool_backward_equals_torch(shape, h16):
    x = R.pool_input(shape, f"mp.gpu{shape}")
    gy = synthetic._uniform(f"mp.gpu.g{shape}", (shape[0], shape[1], shape[2] // 2, shape[3] // 2), -1, 1)
    if h16:
        x, gy = G.bf(x), G.bf(gy)
    assert float((x == 0).float().mean()) >= 0.3
    xl = x.clone().requires_grad_()
    (want,) = torch.autograd.grad(F.max_pool2d(xl, 2, 2), xl, gy)
    dt = torch.bfloat16 if h16 else torch.float32
    xd, gd = _nhwc(x.to(dt)), _nhwc(gy.to(dt))
    gx = torch.full_like(xd, float("nan"))                   # an element the kernel leaves out shows
    B, Cc, H, W = shape
    L.call("hesic_maxpool2_backward", L.ptr(xd), L.ptr(gd), L.ptr(gx), B, H, W, Cc, L.dt(xd), L.stream())
    assert torch.equal(gx.float().cpu(), want)
    # and through autograd (homography.max_pool2)
    xa = xd.clone().requires_grad_()
    y = homography.max_pool2(xa)
    assert torch.equal(y.float().cpu(), F.max_pool2d(x, 2, 2))
    (ga,) = torch.autograd.grad(y, xa, gd)
    assert torch.equal(ga.float().cpu(), want)


# ---------------------------------------------------------------------------------------------------------- flatten + dropout
def _flatten_dropout(fwd, src, dst, B, HW, Cc, p, seed, step, site):
    L.call("hesic_flatten_dropout_forward" if fwd else "hesic_flatten_dropout_backward", L.ptr(src), L.ptr(dst), B, HW, Cc,
           *Fn.dropout_args(p, seed, step, site), L.dt(src), L.stream())


@pytest.mark.parametrize("shape", [(3, 16, 128), (2, 256, 128), (5, 1, 1024), (1, 1, 8)], ids=lambda s: "x".join(map(str, s)))
def test_flatten_dropout_is_bit_equal(shape):
    B, HW, Cc = shape
    side = int(round(HW ** 0.5))
    x = synthetic._uniform(f"fd.x{shape}", (B, Cc, side, side), -2, 2)                    # logical NCHW
    g = synthetic._uniform(f"fd.g{shape}", (B, Cc * HW), -2, 2)
    xd, gd = _nhwc(x), g.to(DEV)
    site = 1 if HW == 1 else 0
    for p in (0.0, 0.5, 0.3):
        for seed in (1, (5 << 32) + 9):
            for step in (0, 3):
                y = torch.full((B, Cc * HW), float("nan"), device=DEV)
                gx = torch.full_like(xd, float("nan"))
                _flatten_dropout(True, xd, y, B, HW, Cc, p, seed, step, site)
                _flatten_dropout(False, gd, gx, B, HW, Cc, p, seed, step, site)
                want_y = R.flatten_dropout(x, p, seed, step, site)
                want_g = R.flatten_dropout_backward(g, x.shape, p, seed, step, site)
                assert torch.equal(y.cpu().view(torch.int32), want_y.view(torch.int32)), (p, seed, step)
                assert torch.equal(gx.cpu().view(torch.int32), want_g.contiguous().view(torch.int32)), (p, seed, step)
                if p == 0.0:
                    assert torch.equal(y.cpu(), x.reshape(B, -1))                      # the plain permutation
    if shape == (3, 16, 128):          # 16-bit storage: the fp32 product is rounded once into the storage type
        xb = G.bf(x).to(torch.bfloat16)
        y = torch.empty((B, Cc * HW), dtype=torch.bfloat16, device=DEV)
        _flatten_dropout(True, _nhwc(xb), y, B, HW, Cc, 0.3, 1, 0, 0)
        assert torch.equal(y.cpu().view(torch.int16), R.flatten_dropout(xb, 0.3, 1, 0, 0).view(torch.int16))
    # through autograd
    xa = xd.clone().requires_grad_()
    cfg = Fn.dropout_args(0.5, 7, 2, site)
    ya = Fn.flatten_dropout(xa if HW > 1 else xa.reshape(B, Cc), cfg)
    (ga,) = torch.autograd.grad(ya, xa, gd)
    assert torch.equal(ya.detach().cpu(), R.flatten_dropout(x, 0.5, 7, 2, site))
    assert torch.equal(ga.cpu(), R.flatten_dropout_backward(g, x.shape, 0.5, 7, 2, site))


# --------------------------------------------------------------------------------------------------------------------- Linear
def _linear_forward(x, w, b, act):
    B, In = x.shape
    Out = w.shape[0]
    nws = int(L.lib().hesic_linear_forward_ws_bytes(B, In, Out))
    ws = torch.full((nws // 4,), float("nan"), device=DEV)
    y = torch.full((B, Out), float("nan"), dtype=x.dtype, device=DEV)
    L.call("hesic_linear_forward", L.ptr(x), L.ptr(w), L.ptr(b), L.ptr(y), B, In, Out, act, L.dt(x), L.ptr(ws), nws, L.stream())
    return y


def _linear_dgrad(g, w):
    B, Out = g.shape
    gx = torch.full((B, w.shape[1]), float("nan"), dtype=g.dtype, device=DEV)
    L.call("hesic_linear_dgrad", L.ptr(g), L.ptr(w), L.ptr(gx), B, w.shape[1], Out, L.dt(g), L.stream())
    return gx


def _linear_wgrad(x, g, dw, db, accumulate):
    L.call("hesic_linear_wgrad", L.ptr(x), L.ptr(g), L.ptr(dw), L.ptr(db), x.shape[0], x.shape[1], g.shape[1], accumulate, L.dt(x), L.stream())


@pytest.mark.parametrize("act", [G.ACT_NONE, G.ACT_RELU], ids=["none", "relu"])
@pytest.mark.parametrize("tag", sorted(R.LINEAR_CASES))
def test_linear_kernels_inside_their_bars(tag, act):
    """Every element of y, gx, dW and db inside bar_e = 8 sqrt(n) 2^-24 S_e (+ 2^-8 |ref_e| for 16-bit y / gx); accumulate on = accumulate
    off added to what was there, exactly; the same bits in a second run."""
    B, In, Out, h16 = R.LINEAR_CASES[tag]
    dt = torch.bfloat16 if h16 else torch.float32
    x, w, b, gy = R.linear_operands(tag)
    xd, wd, bd, gd = x.to(dt).to(DEV), w.to(DEV), b.to(DEV), gy.to(dt).to(DEV)
    y = _linear_forward(xd, wd, bd, act)
    g = gd
    if act:
        g = torch.empty_like(y)
        L.call("hesic_act_backward", L.ptr(y), L.ptr(gd), L.ptr(g), y.numel(), act, L.dt(y), L.stream())
    gx = _linear_dgrad(g, wd)
    dw, db = torch.full_like(wd, float("nan")), torch.full_like(bd, float("nan"))
    _linear_wgrad(xd, g, dw, db, 0)
    base_w, base_b = torch.full_like(wd, 0.375), torch.linspace(-1, 1, Out, device=DEV)
    acc_w, acc_b = base_w.clone(), base_b.clone()
    _linear_wgrad(xd, g, acc_w, acc_b, 1)
    ref = R.linear_reference(tag, act, y_saved=y.float().cpu())
    ratios, msgs = {}, []
    for q, got in (("y", y), ("dx", gx), ("dw", dw), ("db", db)):
        ok, ratios[q], msg = G.check(ref, q, got.float())
        if not ok:
            msgs.append(msg)
    print(f"homography_net_parity linear {tag} act={act} ratio to the unit bound: " + " ".join(f"{q} {v:.3f}" for q, v in ratios.items()))
    assert not msgs, msgs
    assert torch.equal(acc_w, base_w + dw) and torch.equal(acc_b, base_b + db)
    # run to run
    assert torch.equal(_linear_forward(xd, wd, bd, act), y) and torch.equal(_linear_dgrad(g, wd), gx)
    dw2, db2 = torch.empty_like(wd), torch.empty_like(bd)
    _linear_wgrad(xd, g, dw2, db2, 0)
    assert torch.equal(dw2, dw) and torch.equal(db2, db)


def test_linear_row_does_not_depend_on_batch():
    x, w, b, gy = R.linear_operands("b5_1024_8")
    xd, wd, bd, gd = x.to(DEV), w.to(DEV), b.to(DEV), gy.to(DEV)
    for act in (G.ACT_NONE, G.ACT_RELU):
        assert torch.equal(_linear_forward(xd, wd, bd, act)[2], _linear_forward(xd[2:3].contiguous(), wd, bd, act)[0])
    assert torch.equal(_linear_dgrad(gd, wd)[2], _linear_dgrad(gd[2:3].contiguous(), wd)[0])
    # and with the wide layer's shapes, across the row-tile count (row 2 of 64 rows, alone)
    x, w, b, gy = R.linear_operands("b64_2048_1024")
    xd, wd, bd, gd = x.to(DEV), w.to(DEV), b.to(DEV), gy.to(DEV)
    assert torch.equal(_linear_forward(xd, wd, bd, G.ACT_RELU)[2], _linear_forward(xd[2:3].contiguous(), wd, bd, G.ACT_RELU)[0])
    assert torch.equal(_linear_dgrad(gd, wd)[2], _linear_dgrad(gd[2:3].contiguous(), wd)[0])


def test_linear_autograd_slots_and_large_batch_route():
    """``functional.linear``: plain gradients without a slot, direct write / add with the flat-slot protocol, and more than 64 rows through
    the 1x1 conv route -- all inside the same bars."""
    tag = "b3_520_8"
    x, w, b, gy = R.linear_operands(tag)
    lin = torch.nn.Linear(520, 8).to(DEV)
    with torch.no_grad():
        lin.weight.copy_(w)
        lin.bias.copy_(b)
    xd = x.to(DEV).requires_grad_()
    y = Fn.linear(xd, lin.weight, lin.bias, act=L.ACT_RELU)
    dx, dw, db = torch.autograd.grad(y, (xd, lin.weight, lin.bias), gy.to(DEV))
    ref = R.linear_reference(tag, G.ACT_RELU, y_saved=y.detach().cpu())
    for q, got in (("y", y), ("dx", dx), ("dw", dw), ("db", db)):
        ok, _, msg = G.check(ref, q, got)
        assert ok, msg
    group = train.FlatGroup(lin.parameters())
    group.zero_grad()
    prev = Fn.grad_slots_active(True)
    try:
        for _ in range(2):                                   # first backward writes the cleared slots, the second adds
            Fn.linear(xd, lin.weight, lin.bias, act=L.ACT_RELU).backward(gy.to(DEV))
    finally:
        Fn.grad_slots_active(prev)
    assert [s.writes for s in group.slots] == [2, 2]
    assert torch.equal(lin.weight.grad, dw + dw) and torch.equal(lin.bias.grad, db + db)
    # 65 rows
    tag = "b65_512_32"
    x, w, b, gy = R.linear_operands(tag)
    xd, wd, bd = x.to(DEV).requires_grad_(), w.to(DEV).requires_grad_(), b.to(DEV).requires_grad_()
    y = Fn.linear(xd, wd, bd, act=L.ACT_RELU)
    dx, dw, db = torch.autograd.grad(y, (xd, wd, bd), gy.to(DEV))
    ref = R.linear_reference(tag, G.ACT_RELU, y_saved=y.detach().cpu())
    for q, got in (("y", y), ("dx", dx), ("dw", dw), ("db", db)):
        ok, ratio, msg = G.check(ref, q, got)
        print(f"homography_net_parity linear_conv_route {tag} {q} {ratio:.3f}")
        assert ok, msg


# ------------------------------------------------------------------------------------------- order-fixed conv parameter gradients
@pytest.mark.parametrize("shape,h16", [((3, 2, 9, 11, 64), False), ((2, 2, 32, 32, 128), False), ((2, 2, 8, 8, 64), True)], ids=["3x9x11_c64", "2x32x32_c128", "h16_2x8x8_c64"])
def test_order_fixed_conv_gradients(shape, h16):
    """``hesic_bias_grad`` and ``hesic_narrow_in_wgrad`` against the fp64 conv reference of tests/conv_grad_ref.py (bar 8 sqrt(n) 2^-24 S_e per
    element), the same bits in a second run, accumulate = overwrite added to what was there."""
    B, Cin, H, W, Cout = shape
    x = synthetic._uniform(f"det.x{shape}", (B, Cin, H, W), 0, 1)
    w = synthetic._uniform(f"det.w{shape}", (Cout, Cin, 3, 3), -0.5, 0.5)
    b = synthetic._uniform(f"det.b{shape}", (Cout,), -0.05, 0.05)
    gy = synthetic._uniform(f"det.g{shape}", (B, Cout, H, W), -1, 1)
    if h16:
        gy = G.bf(gy)
    ref = G.reference(x, w, b, gy, stride=1, pad=1)
    xd, gd = x.to(DEV), _nhwc(gy.to(torch.bfloat16 if h16 else torch.float32))

    def run(acc, dw, db):
        ws = torch.full((L.DET_MAX_BLOCKS * Cout * Cin * 9,), float("nan"), device=DEV)
        L.call("hesic_bias_grad", L.ptr(gd), L.ptr(db), L.ptr(ws), B * H * W, Cout, acc, L.dt(gd), L.stream())
        ws.fill_(float("nan"))
        L.call("hesic_narrow_in_wgrad", L.ptr(xd), L.ptr(gd), L.ptr(dw), L.ptr(ws), B, Cin, H, W, Cout, acc, L.dt(gd), L.stream())
        return dw, db

    dw, db = run(0, torch.full((Cout, Cin, 3, 3), float("nan"), device=DEV), torch.full((Cout,), float("nan"), device=DEV))
    dw2, db2 = run(0, torch.empty_like(dw), torch.empty_like(db))
    assert torch.equal(dw2, dw) and torch.equal(db2, db)
    base_w, base_b = torch.full_like(dw, 0.375), torch.linspace(-1, 1, Cout, device=DEV)
    aw, ab = run(1, base_w.clone(), base_b.clone())
    assert torch.equal(aw, base_w + dw) and torch.equal(ab, base_b + db)
    for q, got in (("dw", dw), ("db", db)):
        ok, ratio, msg = G.check(ref, q, got)
        print(f"homography_net_parity order_fixed {'x'.join(map(str, shape))}{'_h16' if h16 else ''}_{q} {ratio:.3f}")
        assert ok, msg


@pytest.mark.parametrize("cin,order_fixed", [(2, False), (3, True)], ids=["cin2_usual_kernels", "cin3_order_fixed_bias"])
def test_narrow_conv_backward_keeps_the_forward_dtype(cin, order_fixed, monkeypatch):
    """A conv with few input channels whose forward ran at fp32 and whose backward runs with the global compute dtype set to bf16: the
    backward uses the type the forward gave its output (a gy taken for bf16 would miss these fp32 bars by orders of magnitude).  Outside
    ``deterministic_conv_grads`` this is the usual strided kernels; inside, with Cin != 2, the bias comes from ``hesic_bias_grad`` and the
    usual weight-gradient kernel runs without a bias output."""
    B, H, W, Cout = 2, 9, 11, 64
    x = synthetic._uniform(f"nc.x{cin}", (B, cin, H, W), 0, 1)
    w = synthetic._uniform(f"nc.w{cin}", (Cout, cin, 3, 3), -0.5, 0.5)
    b = synthetic._uniform(f"nc.b{cin}", (Cout,), -0.05, 0.05)
    gy = synthetic._uniform(f"nc.g{cin}", (B, Cout, H, W), -1, 1)
    xd, wd, bd = x.to(DEV).requires_grad_(), w.to(DEV).requires_grad_(), b.to(DEV).requires_grad_()
    launches, real_call = [], L.call

    def recording_call(name, *args):          # the backward runs on autograd's own thread: ``call_hook`` (thread-local) would not see it
        launches.append(name)
        return real_call(name, *args)

    prev = Fn.compute_dtype()
    try:
        Fn.set_compute_dtype(torch.float32)
        with Fn.deterministic_conv_grads() if order_fixed else contextlib.nullcontext():
            y = Fn.conv2d(xd, wd, bd, kernel_size=3, stride=1, padding=1, act=L.ACT_RELU)
        Fn.set_compute_dtype(torch.bfloat16)
        monkeypatch.setattr(L, "call", recording_call)
        dx, dw, db = torch.autograd.grad(y, (xd, wd, bd), _nhwc(gy))
        monkeypatch.undo()
    finally:
        Fn.set_compute_dtype(prev)
    assert y.dtype == torch.float32
    assert ("hesic_bias_grad" in launches) == order_fixed and "hesic_narrow_in_wgrad" not in launches and "hesic_sconv2d_wgrad" in launches
    ref = G.reference(x, w, b, gy, stride=1, pad=1, act=G.ACT_RELU, y_saved=y.detach().cpu(), y16=False, dx16=False)
    for q, got in (("y", y), ("dx", dx), ("dw", dw), ("db", db)):
        ok, ratio, msg = G.check(ref, q, got)
        print(f"homography_net_parity narrow_conv cin{cin}{'_order_fixed' if order_fixed else ''}_{q} {ratio:.3f}")
        assert ok, msg


# ---------------------------------------------------------------------------------------------------------------- the network
def _net(patch_size, P):
    net = homography.Net(patch_size=patch_size)
    net.load_state_dict(P)
    return net.to(DEV)


@pytest.mark.parametrize("name,patch,B,training", [("p32_b3_eval", 32, 3, False), ("p32_b3_train", 32, 3, True), ("p128_b2_train", 128, 2, True)])
def test_network_gradient(name, patch, B, training):
    """delta and every parameter's gradient of sum(delta * g) against the fp64 restatement, per tensor || . - ref || / || ref ||, under
    8 x the largest such ratio torch's own fp32 CPU autograd of the restatement reaches on the same inputs."""
    P = R.net_params(patch)
    a, b, _ = synthetic.homography_batch(3, B, patch=patch)
    g = synthetic._uniform(f"net.g.{name}", (B, 4, 2), -1, 1)
    seed, step = 21, 4
    masks = R.net_masks(B, patch, seed, step) if training else None
    d64, g64 = R.net_grads(P, a, b, g, masks, torch.float64)
    d32, g32 = R.net_grads(P, a, b, g, masks, torch.float32)
    floor = {"delta": R.rel_err(d32, d64), **{k: R.rel_err(g32[k], g64[k]) for k in g64}}
    bar = G.C_BAR * max(floor.values())
    net = _net(patch, P).train(training)
    net.set_dropout_state(seed, step)
    ad, bd, gd = a.to(DEV), b.to(DEV), g.to(DEV)
    with torch.enable_grad():
        delta = net(ad, bd)
        assert net.dropout_state() == (seed, step + int(training))
        (delta * gd).sum().backward()
    got = {"delta": R.rel_err(delta, d64), **{k: R.rel_err(p.grad, g64[k]) for k, p in net.named_parameters()}}
    print(f"homography_net_parity network {name} bar {bar:.3e} (8 x fp32 CPU floor {max(floor.values()):.3e}); HIP worst {max(got.values()):.3e} "
          + " ".join(f"{k}={v:.2e}/{floor[k]:.2e}" for k, v in got.items()))
    assert set(got) == set(floor) and len(got) == 21
    bad = {k: v for k, v in got.items() if not v <= bar}
    assert not bad, (bar, bad)
    # the backward does not read the global compute dtype: set to bf16 between forward and backward, the gradients keep their bits
    first = {k: p.grad.clone() for k, p in net.named_parameters()}
    net.zero_grad(set_to_none=True)
    net.set_dropout_state(seed, step)
    prev = Fn.compute_dtype()
    with torch.enable_grad():
        delta2 = net(ad, bd)
        Fn.set_compute_dtype(torch.bfloat16)
        try:
            (delta2 * gd).sum().backward()
        finally:
            Fn.set_compute_dtype(prev)
    assert torch.equal(delta2, delta)
    for k, p in net.named_parameters():
        assert torch.equal(p.grad, first[k]), k


def test_inference_is_unchanged_by_training_calls():
    P = R.net_params(128)
    net = _net(128, P).eval()
    a, b, _ = synthetic.homography_batch(0, 2)
    ad, bd = a.to(DEV), b.to(DEV)
    launches = []
    with torch.no_grad(), L.call_hook(lambda name, args: launches.append(name)):
        before = net(ad, bd)
    assert "hesic_linear_forward" not in launches and "hesic_flatten_dropout_forward" not in launches and launches.count("hesic_maxpool2_forward") == 3
    assert float((before.cpu() - T(load_golden("homo.npz")["delta"])).abs().max()) < 2e-3
    net.train()
    with torch.enable_grad():
        net(ad, bd).sum().backward()
    net.eval()
    with torch.enable_grad():
        eval_grad = net(ad, bd)                                  # eval mode with grad: no dropout, the training kernels
    with torch.no_grad():
        after = net(ad, bd)
    assert torch.equal(after, before)
    assert float((eval_grad.detach() - before).abs().max()) < 2e-3
    # train mode under no_grad: dropout on, no graph
    net.train()
    net.set_dropout_state(3, 0)
    with torch.no_grad():
        dropped = net(ad, bd)
    assert not dropped.requires_grad and net.dropout_state() == (3, 1) and not torch.equal(dropped, before)
    masks = R.net_masks(2, 128, 3, 0)
    want = R.net_forward({k: v.double() for k, v in P.items()}, a, b, masks)
    bar = G.C_BAR * R.rel_err(R.net_forward(P, a, b, masks, torch.float32), want)          # 8 x the fp32 CPU floor, as in the network test
    print(f"homography_net_parity train_mode_no_grad delta {R.rel_err(dropped, want):.3e} bar {bar:.3e}")
    assert R.rel_err(dropped, want) <= bar


# ----------------------------------------------------------------------------------------------------------------- the trainer
def _trainer(P0, **kw):
    net = _net(32, P0)
    return net, train.HomographyTrainer(net, lr=1e-4, seed=0, **kw)


def test_trainer_trace():
    """Three steps against the fp64 CPU loop with the same masks: |loss - ref| <= 8 |fp32 CPU loss - fp64 CPU loss| + LOSS_BAR max(1, |ref|)."""
    P0, inputs, _, l64, _ = R.trainer_reference(3, True)
    l32 = R.trainer_reference(30, False)[3][:3]
    net, tr = _trainer(P0)
    dev = [t.to(DEV) for t in inputs]
    prev = Fn.compute_dtype()
    got = []
    for _ in range(3):
        out = tr.step(*dev)
        assert set(out) == {"loss"} and out["loss"].shape == () and out["loss"].is_cuda and not out["loss"].requires_grad
        got.append(float(out["loss"]))
    assert Fn.compute_dtype() == prev and net.dropout_state() == (0, 3)
    bars = [G.C_BAR * abs(a - b) + HT.LOSS_BAR * max(1.0, abs(b)) for a, b in zip(l32, l64)]
    print("homography_net_parity trainer_trace " + " ".join(f"step{t}: hip {got[t]:.9f} fp32 {l32[t]:.9f} fp64 {l64[t]:.9f} bar {bars[t]:.2e}"
                                                          for t in range(3)))
    for t in range(3):
        assert abs(got[t] - l64[t]) <= bars[t], (t, got[t], l64[t], bars[t])


def test_trainer_descends_and_caches_follow():
    P0, inputs, L0, _, P32 = R.trainer_reference(30, False)
    Lref = R.eval_loss(P32, inputs)
    net, tr = _trainer(P0)
    dev = [t.to(DEV) for t in inputs]
    net.train()
    first = float(tr.evaluate(*dev))
    assert net.training                                          # evaluate leaves the module's mode alone
    for _ in range(30):
        tr.step(*dev)
    final = float(tr.evaluate(*dev))
    print(f"homography_net_parity trainer_descent L0 {L0:.6f} (hip {first:.6f}) reference (fp32 CPU, same masks) {Lref:.6f} hip {final:.6f}")
    assert Lref < L0 and final <= L0 - 0.5 * (L0 - Lref)
    # an eval forward after training == the restatement with the trained parameters (stale packed weights / fc.2 copies would show)
    trained = {k: v.detach().cpu() for k, v in net.state_dict().items()}
    a, b = inputs[1], inputs[2]
    d64 = R.net_forward({k: v.double() for k, v in trained.items()}, a, b)
    d32 = R.net_forward(trained, a, b, dtype=torch.float32)
    net.eval()
    with torch.no_grad():
        got = net(dev[1], dev[2])
    # the bar of the network test on delta: 8 x the fp32 CPU floor of these inputs
    bar = G.C_BAR * R.rel_err(d32, d64)
    print(f"homography_net_parity trainer_eval_after_training delta {R.rel_err(got, d64):.3e} bar {bar:.3e}")
    assert R.rel_err(got, d64) <= bar


def test_trainer_resume_is_bit_identical():
    P0, inputs = R.net_params(32), R.trainer_inputs()
    dev = [t.to(DEV) for t in inputs]
    net_a, tr_a = _trainer(P0, clip_max_norm=0.5, live_lr=True)
    la = []
    for t in range(4):
        if t == 3:
            tr_a.set_lr(5e-5)
        out = tr_a.step(*dev)
        assert set(out) == {"loss", "grad_norm", "clip_coef", "skipped"} and float(out["skipped"]) == 0.0
        la.append(out["loss"].clone())
    net_b, tr_b = _trainer(P0, clip_max_norm=0.5, live_lr=True)
    lb = [tr_b.step(*dev)["loss"].clone() for _ in range(2)]
    sd = tr_b.state_dict()
    assert set(sd) == {"state_dict", "optimizer", "dropout"} and sd["dropout"] == (0, 2)
    net_c, tr_c = _trainer(R.net_params(32, salt=1), clip_max_norm=0.5, live_lr=True)
    tr_c.load_state_dict(sd)
    lb.append(tr_c.step(*dev)["loss"].clone())
    tr_c.set_lr(5e-5)
    lb.append(tr_c.step(*dev)["loss"].clone())
    print("homography_net_parity trainer_resume max |loss difference| " + f"{max(float((x - y).abs()) for x, y in zip(la, lb)):.3e}")
    assert all(torch.equal(x, y) for x, y in zip(la, lb)), (la, lb)
    for (k, p), q in zip(net_a.named_parameters(), net_c.parameters()):
        assert torch.equal(p, q), k
    assert net_a.dropout_state() == net_c.dropout_state() == (0, 4)
    assert torch.equal(tr_a.optimizer.exp_avg_sq, tr_c.optimizer.exp_avg_sq)


def test_trainer_step_refuses_stream_capture(monkeypatch):
    """The step is eager (the mask's step counter is a by-value kernel argument): while a stream is capturing it raises before it launches
    or changes anything.  (The capture state is patched: nothing is recorded into a graph here.)"""
    P0, inputs = R.net_params(32), R.trainer_inputs()
    net, tr = _trainer(P0)
    dev = [t.to(DEV) for t in inputs]
    launches = []
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: True)
    with L.call_hook(lambda name, args: launches.append(name)):
        with pytest.raises(RuntimeError, match="eager"):
            tr.step(*dev)
    monkeypatch.undo()
    assert not launches and net.dropout_state() == (0, 0)
    assert bool(torch.isfinite(tr.step(*dev)["loss"]))

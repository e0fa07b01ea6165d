"""``hesic_en_loss``, ``hesic_en_loss_grad`` and ``hesic_c32_mirror_weights`` (csrc/en_train.hip) on a real MI355X, in both libraries.

Every operand, output and workspace is ``memguard.guarded``; outputs and the workspace start as NaN bytes and every guard is checked after the
call.  The gradient map must equal the numpy restatement (tests/en_train_ref.py) bit for bit, zeros in channels 3..31 included.  The sums: every
term is an exact, non-negative fp64 number, so whatever the order of the additions each sum lies within ``(n + 8) * 2^-53`` relative of the exact
value (``en_train_ref.sum_bar``; a derived bar, not a measured one).  Each case prints its figures before it asserts.  (The file runs next to
``test_stage2_trainer_gpu.py``, behind the suite's other GPU files: see there.)"""
import numpy as np
import pytest
import torch

import en_train_ref as R
import memguard
from hesic_amd import synthetic

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF, F16, F32 = torch.bfloat16, torch.float16, torch.float32
K = 0.0067 * 255 ** 2
# (1,1,1): one element, the scalar tail alone; (2,3,5): image 1's span starts 4-byte but not 16-byte aligned; (1,17,129): 1644 four-element groups
# and a tail of 3; (3,64,64): three trips of one block per image; (1,37,37): 4107 elements, one past a block's share: two partials per image
SHAPES = [(1, 1, 1), (2, 3, 5), (1, 17, 129), (3, 64, 64), (1, 37, 37)]


@pytest.fixture(params=["bf16", "f16"])
def fmt(request):
    import hesic_amd
    hesic_amd.set_compute_dtype({"bf16": BF, "f16": F16}[request.param])
    yield request.param
    hesic_amd.set_compute_dtype(BF)
    hesic_amd.set_compute_dtype(F32)


def _fn():
    from hesic_amd import functional as Fn
    return Fn


def _operands(shape, offset=0, tag="g"):
    """Four guarded fp32 (B,3,H,W) tensors: enhanced images a little outside [0, 1], targets inside; ``offset`` bytes past a 256-byte boundary."""
    B, H, W = shape
    host, dev = [], []
    for v in (1, 2):
        b = synthetic._uniform(f"en.gpu.{tag}.b{v}", (B, 3, H, W), 0, 1).float()
        a = (b + synthetic._uniform(f"en.gpu.{tag}.e{v}", (B, 3, H, W), -0.2, 0.2) * (0.5 if v == 2 else 1.0)).float()
        host += [a, b]
    for t, name in zip(host, ("a1", "b1", "a2", "b2")):
        dev.append(memguard.guarded(t.to(DEV), name=name, offset=offset))
    return host, dev


def _run_loss(dev, shape):
    Fn = _fn()
    from hesic_amd import _lib as L
    need = L.lib().hesic_en_loss_ws_bytes(*shape)
    assert need > 0
    ws = memguard.guarded(torch.full((need,), 0xFF, dtype=torch.uint8, device=DEV), name="workspace")
    out = memguard.guarded(torch.full((4,), float("nan"), dtype=torch.float64, device=DEV), name="out")
    assert Fn.en_loss(*dev, K, out=out, ws=ws) is out
    torch.cuda.synchronize()
    memguard.check_all(dev + [ws, out])
    return out.cpu().clone(), ws.cpu().clone()


def _run_grad(dev, shape, fmt, seed=None):
    Fn = _fn()
    B, H, W = shape
    h16 = {"bf16": BF, "f16": F16}[fmt]
    maps = [memguard.guarded(torch.full((B, H, W, 32), float("nan"), dtype=h16, device=DEV).permute(0, 3, 1, 2), name=f"g{v}") for v in (1, 2)]
    sd = None if seed is None else memguard.guarded(torch.tensor([seed], dtype=F32, device=DEV), name="seed")
    g1, g2 = Fn.en_loss_grad(*dev, K, seed=sd, out=maps)
    torch.cuda.synchronize()
    memguard.check_all(dev + maps + ([sd] if sd is not None else []))
    return [g.permute(0, 2, 3, 1).contiguous().view(torch.int16).cpu().numpy().view(np.uint16) for g in (g1, g2)]


@pytest.mark.parametrize("offset", [0, 4], ids=["aligned", "plus4"])
@pytest.mark.parametrize("seed", [None, 0.37], ids=["noseed", "seed"])
@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_gradient_map_equals_the_restatement_bit_for_bit(fmt, shape, seed, offset):
    host, dev = _operands(shape, offset)
    got = _run_grad(dev, shape, fmt, seed)
    for v in (0, 1):
        want = R.grad_map_bits(host[2 * v].numpy(), host[2 * v + 1].numpy(), K, fmt, seed)
        diff = int((got[v] != want).sum())
        print(f"en_loss_grad {fmt} {shape} seed={seed} +{offset} view{v + 1} differing={diff} nonzero={int((want != 0).sum())}")
        assert got[v].shape == want.shape and diff == 0
        assert not got[v][..., 3:].any() and (want[..., :3] != 0).any()


@pytest.mark.parametrize("offset", [0, 4], ids=["aligned", "plus4"])
@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_sums_are_within_the_derived_bar_of_the_exact_sums(fmt, shape, offset):
    """``offset`` = 4 puts every operand one element past a 16-byte boundary: the 4-byte loads, which must give the aligned call's bits."""
    host, dev = _operands(shape, offset)
    got, _ = _run_loss(dev, shape)
    want = R.loss_values(*(t.numpy() for t in host), K)
    n = host[0].numel()
    bar = R.sum_bar(n)
    for i, name in enumerate(("sse1", "sse2")):
        rel = abs(float(got[i]) - want[i]) / want[i]
        print(f"en_loss {fmt} {shape} +{offset} {name} rel={rel:.3e} bar={bar:.3e}")
        assert rel <= bar
    # mse_loss and loss are fp64 arithmetic on the kernel's own sums: two divisions and an addition, one multiplication
    mse = float(got[0]) / n + float(got[1]) / n
    assert float(got[2]) == mse and float(got[3]) == K * mse
    if offset:
        _, dev0 = _operands(shape, 0)
        assert torch.equal(_run_loss(dev0, shape)[0].view(torch.int64), got.view(torch.int64))


def test_workspace_holds_one_partial_per_block_and_their_ordered_sum(fmt):
    """(1,37,37): two partials per (view, image); the finishing launch adds them in index order."""
    shape = (1, 37, 37)
    host, dev = _operands(shape)
    got, ws = _run_loss(dev, shape)
    parts = ws.view(torch.float64)
    assert parts.numel() == 4 and bool(torch.isfinite(parts).all()) and bool((parts > 0).all())
    assert float(got[0]) == float(parts[0]) + float(parts[1]) and float(got[1]) == float(parts[2]) + float(parts[3])


@pytest.mark.parametrize("shape", [(3, 64, 64), (1, 37, 37)], ids=str)
def test_second_run_and_graph_replay_are_bit_identical(fmt, shape):
    Fn = _fn()
    host, dev = _operands(shape)
    first, first_g = _run_loss(dev, shape)[0], _run_grad(dev, shape, fmt)
    again, again_g = _run_loss(dev, shape)[0], _run_grad(dev, shape, fmt)
    assert torch.equal(first.view(torch.int64), again.view(torch.int64))
    assert all(np.array_equal(a, b) for a, b in zip(first_g, again_g))
    B, H, W = shape
    from hesic_amd import _lib as L
    h16 = {"bf16": BF, "f16": F16}[fmt]
    ws = torch.full((L.lib().hesic_en_loss_ws_bytes(*shape),), 0xFF, dtype=torch.uint8, device=DEV)
    out = torch.full((4,), float("nan"), dtype=torch.float64, device=DEV)
    maps = [torch.full((B, H, W, 32), float("nan"), dtype=h16, device=DEV).permute(0, 3, 1, 2) for _ in range(2)]
    graph = torch.cuda.CUDAGraph()
    torch.cuda.synchronize()
    with torch.cuda.graph(graph):
        Fn.en_loss(*dev, K, out=out, ws=ws)
        Fn.en_loss_grad(*dev, K, out=maps)
    for _ in range(2):
        out.fill_(float("nan"))
        for m in maps:
            m.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out.cpu().view(torch.int64), first.view(torch.int64))
        for m, want in zip(maps, first_g):
            assert np.array_equal(m.permute(0, 2, 3, 1).contiguous().view(torch.int16).cpu().numpy().view(np.uint16), want)
    memguard.check_all(dev)


def test_one_nan_reaches_its_element_and_its_views_sums_alone(fmt):
    shape = (2, 17, 19)
    host, dev = _operands(shape, tag="nan")
    with torch.no_grad():
        dev[3][1, 2, 5, 7] = float("nan")               # a target of view 2
    host[3][1, 2, 5, 7] = float("nan")
    got, _ = _run_loss(dev, shape)
    want = R.loss_values(*(t.numpy() for t in host), K)
    assert abs(float(got[0]) - want[0]) <= R.sum_bar(host[0].numel()) * want[0]
    assert torch.isnan(got[1]) and torch.isnan(got[2]) and torch.isnan(got[3])
    g = _run_grad(dev, shape, fmt)
    h16 = {"bf16": BF, "f16": F16}[fmt]
    nan = [torch.isnan(torch.from_numpy(m.view(np.int16)).view(h16).float()) for m in g]
    assert int(nan[0].sum()) == 0 and int(nan[1].sum()) == 1 and bool(nan[1][1, 5, 7, 2])
    w1 = R.grad_map_bits(host[0].numpy(), host[1].numpy(), K, fmt)
    w2 = R.grad_map_bits(host[2].numpy(), host[3].numpy(), K, fmt)
    keep = ~nan[1].numpy()
    assert np.array_equal(g[0], w1) and np.array_equal(g[1][keep], w2[keep])


# ----------------------------------------------------------------------------------------------------------------------------- the mirror
def _flat_enhancer():
    """The 40 conv weights of an ``Independent_EN`` in one flat fp32 buffer (64-float slots, NaN between them) and the table entries."""
    from hesic_amd import models
    from test_oracle_golden import _en_params
    en = models.Independent_EN()
    en.load_state_dict(_en_params(), strict=True)
    ws = [p.detach() for p in en.parameters() if p.dim() == 4]
    entries, so, do = [], 0, 0
    for w in ws:
        entries.append((so, do, w.shape[0], w.shape[1], 32))
        so += -(-w.numel() // 64) * 64 + 64
        do += -(-w.shape[1] * 32 * 9 // 64) * 64 + 64
    src = torch.full((so,), float("nan"))
    for w, e in zip(ws, entries):
        src[e[0]:e[0] + w.numel()] = w.reshape(-1)
    return ws, entries, src, do


def test_mirror_kernel_equals_mirror_t_for_every_layer_in_one_launch(fmt):
    Fn = _fn()
    ws, entries, src, dst_numel = _flat_enhancer()
    assert len(ws) == 40 and {tuple(w.shape[:2]) for w in ws} == {(32, 6), (32, 32), (3, 32)}
    srcd = memguard.guarded(src.to(DEV), name="flat parameters")
    dst = memguard.guarded(torch.full((dst_numel,), float("nan"), device=DEV), name="mirrored weights")
    table = memguard.guarded(Fn.mirror_table(entries, DEV), name="table", fill=0)
    Fn.c32_mirror_weights(srcd, dst, table, len(entries))
    torch.cuda.synchronize()
    memguard.check_all([srcd, dst, table])
    host = dst.cpu()
    written = torch.zeros(dst_numel, dtype=torch.bool)
    for w, (so, do, co, ci, cp) in zip(ws, entries):
        got = host[do:do + ci * cp * 9].view(ci, cp, 3, 3)
        assert torch.equal(got, Fn._mirror_t(w, 32)), (co, ci)
        assert np.array_equal(got.numpy(), R.mirror(w.numpy(), 32))
        written[do:do + ci * cp * 9] = True
    assert bool(torch.isnan(host[~written]).all())              # nothing between the layers' slots was touched


def test_mirror_kernel_skips_an_entry_that_does_not_fit(fmt):
    """An entry whose destination ends one float past the buffer is left out as a whole; its neighbour is written."""
    Fn = _fn()
    w = synthetic._uniform("en.gpu.mw", (32, 32, 3, 3), -1, 1).float()
    src = memguard.guarded(w.reshape(-1).to(DEV), name="flat parameters")
    dst = memguard.guarded(torch.full((2 * 9216,), float("nan"), device=DEV), name="mirrored weights")
    table = memguard.guarded(Fn.mirror_table([(0, 0, 32, 32, 32), (0, 9216 + 1, 32, 32, 32), (1, 9216, 32, 32, 32), (0, 9216, 33, 32, 32)], DEV),
                             name="table", fill=0)
    Fn.c32_mirror_weights(src, dst, table, 4)
    torch.cuda.synchronize()
    memguard.check_all([src, dst, table])
    host = dst.cpu()
    assert torch.equal(host[:9216].view(32, 32, 3, 3), Fn._mirror_t(w, 32)) and bool(torch.isnan(host[9216:]).all())

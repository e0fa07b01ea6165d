"""The dropout state in device memory (include/hesic_homography_net.h): ``hesic_dropout_state_take`` and the ``_state`` forms of the
flatten + dropout entries against the by-value entries, bit for bit -- eagerly, and as a captured graph that draws a new mask per replay."""
import numpy as np
import pytest
import torch

import dropout_state_ref as S
import memguard
from hesic_amd import _lib as L
from hesic_amd import functional as Fn
from hesic_amd import synthetic

pytestmark = pytest.mark.gpu
DEV = "cuda"

# (B, HW, C): the tile kernel below one 32 x 32 tile (HW % 4 == 0); the tile kernel with ragged tiles in both directions; the flat kernel at
# the second site (HW = 1); the flat kernel with an odd HW
SHAPES = [(2, 16, 8), (2, 36, 40), (3, 1, 1024), (2, 9, 4)]
P = 0.5
ids = dict(ids=lambda s: "x".join(map(str, s)))


def _dtype(name):
    return torch.float32 if name == "f32" else L.h16_dtype()


def _operands(shape, dtype):
    """The NHWC map (B, HW, C) and the flat gradient (B, C * HW), on the device."""
    B, HW, Cc = shape
    x = synthetic._uniform(f"ds.x{shape}", (B, HW, Cc), -2, 2).to(dtype).to(DEV)
    g = synthetic._uniform(f"ds.g{shape}", (B, Cc * HW), -1, 1).to(dtype).to(DEV)
    return x, g


def _by_value(fwd, src, dst, shape, seed, step, site):
    B, HW, Cc = shape
    L.call("hesic_flatten_dropout_forward" if fwd else "hesic_flatten_dropout_backward", L.ptr(src), L.ptr(dst), B, HW, Cc,
           *Fn.dropout_args(P, seed, step, site), L.dt(src), L.stream())


def _from_state(fwd, src, dst, shape, taken, site):
    B, HW, Cc = shape
    thr, scale, _, _, _ = Fn.dropout_args(P, 0, 0, site)
    L.call("hesic_flatten_dropout_forward_state" if fwd else "hesic_flatten_dropout_backward_state", L.ptr(src), L.ptr(dst), B, HW, Cc,
           thr, scale, L.ptr(taken), site, L.dt(src), L.stream())


def _words(t):
    return [int(v) & 0xFFFFFFFF for v in t.tolist()]


def _bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int16)


@pytest.mark.parametrize("dtype", ["f32", "h16"])
@pytest.mark.parametrize("shape", SHAPES, **ids)
def test_state_entries_give_the_by_value_bits(shape, dtype):
    dt = _dtype(dtype)
    x, g = _operands(shape, dt)
    for seed, step in ((0, 0), (0x0123456789ABCDEF, 41)):
        state = Fn.dropout_state(seed, step, DEV)
        taken = Fn.dropout_state_take(state)
        assert _words(taken) == S.state_words(seed, step).tolist() == S.take(S.state_words(seed, step))[0].tolist()
        assert _words(state) == S.take(S.state_words(seed, step))[1].tolist()
        for site in (0, 1):
            y, yv = (torch.full((shape[0], shape[1] * shape[2]), float("nan"), dtype=dt, device=DEV) for _ in range(2))
            gx, gxv = (torch.full(x.shape, float("nan"), dtype=dt, device=DEV) for _ in range(2))
            _from_state(True, x, y, shape, taken, site)
            _from_state(False, g, gx, shape, taken, site)
            _by_value(True, x, yv, shape, seed, step, site)
            _by_value(False, g, gxv, shape, seed, step, site)
            assert torch.equal(_bits(y), _bits(yv)), (seed, step, site)
            assert torch.equal(_bits(gx), _bits(gxv)), (seed, step, site)
            assert not bool(torch.isnan(y.float()).any()) and not bool(torch.isnan(gx.float()).any())
            dropped = float((y == 0).float().mean())
            assert 0.2 < dropped < 0.8, dropped           # p = 0.5: it is a mask, not the plain permutation
        assert _words(taken) == S.state_words(seed, step).tolist()         # the _state entries only read it


def test_take_wraps_and_leaves_the_seed_alone():
    seed = 0xFEDCBA9876543210
    state = Fn.dropout_state(seed, 0xFFFFFFFF, DEV)
    taken = Fn.dropout_state_take(state)
    assert _words(taken) == [0x76543210, 0xFEDCBA98, 0xFFFFFFFF, 0]
    assert _words(state) == [0x76543210, 0xFEDCBA98, 0, 0]
    again = Fn.dropout_state_take(state)
    assert _words(again) == [0x76543210, 0xFEDCBA98, 0, 0] and _words(state) == [0x76543210, 0xFEDCBA98, 1, 0]
    assert _words(taken) == [0x76543210, 0xFEDCBA98, 0xFFFFFFFF, 0]      # a fresh tensor per take


@pytest.mark.parametrize("dtype", ["f32", "h16"])
@pytest.mark.parametrize("shape", SHAPES, **ids)
def test_a_captured_graph_draws_a_new_mask_per_replay(shape, dtype):
    """take + forward + backward captured once, replayed three times: replay k gives the by-value entries' bits at ``step0 + k``."""
    dt = _dtype(dtype)
    x, g = _operands(shape, dt)
    seed, step0, site = 11, 0xFFFFFFFE, 0 if shape[1] > 1 else 1            # the counter wraps on the way
    state = Fn.dropout_state(seed, step0, DEV)
    taken = torch.zeros_like(state)
    y = torch.empty((shape[0], shape[1] * shape[2]), dtype=dt, device=DEV)
    gx = torch.empty(x.shape, dtype=dt, device=DEV)
    graph = torch.cuda.CUDAGraph()
    torch.cuda.synchronize()
    with torch.cuda.graph(graph):
        L.call("hesic_dropout_state_take", L.ptr(state), L.ptr(taken), L.stream())
        _from_state(True, x, y, shape, taken, site)
        _from_state(False, g, gx, shape, taken, site)
    assert _words(state) == S.state_words(seed, step0).tolist()           # a capture runs nothing
    seen = []
    for k in range(3):
        graph.replay()
        step = (step0 + k) & 0xFFFFFFFF
        yv, gxv = torch.empty_like(y), torch.empty_like(gx)
        _by_value(True, x, yv, shape, seed, step, site)
        _by_value(False, g, gxv, shape, seed, step, site)
        assert torch.equal(_bits(y), _bits(yv)) and torch.equal(_bits(gx), _bits(gxv)), k
        assert _words(taken) == S.state_words(seed, step).tolist()
        seen.append(y.clone())
    assert _words(state) == S.state_words(seed, (step0 + 3) & 0xFFFFFFFF).tolist()
    assert not torch.equal(seen[0], seen[1]) and not torch.equal(seen[1], seen[2])


def test_a_null_taken_is_refused():
    x, g = _operands(SHAPES[0], torch.float32)
    y = torch.empty((2, 128), device=DEV)
    thr, scale, _, _, _ = Fn.dropout_args(P, 0, 0, 0)
    for name, src, dst in (("hesic_flatten_dropout_forward_state", x, y), ("hesic_flatten_dropout_backward_state", g, torch.empty_like(x))):
        with pytest.raises(RuntimeError, match="null taken"):
            L.call(name, L.ptr(src), L.ptr(dst), 2, 16, 8, thr, scale, None, 0, L.dt(src), L.stream())
    state = Fn.dropout_state(1, 2, DEV)
    for a, b in ((None, state), (state, None), (state, state)):
        with pytest.raises(RuntimeError, match="dropout_state_take"):
            L.call("hesic_dropout_state_take", L.ptr(a), L.ptr(b), L.stream())
    assert _words(state) == [1, 0, 2, 0]
    # the checks of the by-value entries hold here too
    with pytest.raises(RuntimeError, match="multiple of 4"):
        L.call("hesic_flatten_dropout_forward_state", L.ptr(x), L.ptr(y), 2, 16, 6, thr, scale, L.ptr(state), 0, L.F32, L.stream())


@pytest.mark.parametrize("dtype", ["f32", "h16"])
@pytest.mark.parametrize("shape", SHAPES, **ids)
def test_nothing_is_written_outside_the_outputs(shape, dtype):
    dt = _dtype(dtype)
    x0, g0 = _operands(shape, dt)
    B, HW, Cc = shape
    x, g = memguard.guarded(x0, name="x"), memguard.guarded(g0, name="gy")
    y = memguard.guarded(torch.zeros((B, Cc * HW), dtype=dt, device=DEV), name="y")
    gx = memguard.guarded(torch.zeros_like(x0), name="gx")
    state = memguard.guarded(Fn.dropout_state(3, 9, DEV), name="state")
    taken = memguard.guarded(torch.zeros(4, dtype=torch.int32, device=DEV), name="taken")
    site = 0 if HW > 1 else 1
    L.call("hesic_dropout_state_take", L.ptr(state), L.ptr(taken), L.stream())
    _from_state(True, x, y, shape, taken, site)
    _from_state(False, g, gx, shape, taken, site)
    memguard.check_all([x, g, y, gx, state, taken])
    assert torch.equal(x, x0) and torch.equal(g, g0)                       # the inputs are read only
    assert _words(taken) == [3, 0, 9, 0] and _words(state) == [3, 0, 10, 0]
    yv, gxv = torch.empty_like(y), torch.empty_like(gx)
    _by_value(True, x0, yv, shape, 3, 9, site)
    _by_value(False, g0, gxv, shape, 3, 9, site)
    assert torch.equal(_bits(y), _bits(yv)) and torch.equal(_bits(gx), _bits(gxv))

"""CPU self-test of tests/memguard.py: guarded views keep values and strides, ``check()`` sees one-element overruns on either side,
reads past the end return poison, and the ``torch`` proxy intercepts only the listed modules and only inside the block."""
import types

import pytest
import torch

import memguard as MG


def _sources():
    g = torch.Generator().manual_seed(0)
    x = torch.randn(2, 8, 5, 7, generator=g)
    return {
        "contiguous": x,
        "channels_last": x.contiguous(memory_format=torch.channels_last),
        "column_crop": x[..., 1:6],
        "batch_slice_cl": x.to(torch.bfloat16).contiguous(memory_format=torch.channels_last)[1:],
    }


@pytest.mark.parametrize("kind", list(_sources()))
@pytest.mark.parametrize("fill", [MG.NAN_FILL, MG.BIG_FILL])
def test_guarded_view_equals_source(kind, fill):
    t = _sources()[kind]
    v = MG.guarded(t, fill=fill, name=kind)
    assert v.shape == t.shape and v.dtype == t.dtype and v.stride() == t.stride()
    assert torch.equal(v, t)
    assert v.data_ptr() % MG.ALIGN == 0
    v.check()
    assert MG.guarded(t, offset=16).data_ptr() % MG.ALIGN == 16


@pytest.mark.parametrize("kind", list(_sources()))
@pytest.mark.parametrize("side", ["before", "after"])
def test_one_element_overrun_fails_check(kind, side):
    t = _sources()[kind]
    v = MG.guarded(t, name=kind)
    span = 1 + sum((n - 1) * s for n, s in zip(v.shape, v.stride()))
    flat = torch.as_strided(v, (span + 2,), (1,), v.storage_offset() - 1)      # one element either side of the span
    flat[0 if side == "before" else span + 1] = 0
    with pytest.raises(AssertionError, match=kind):
        v.check()


def test_write_into_a_gap_between_rows_fails_check():
    v = MG.guarded(_sources()["column_crop"], name="crop")
    torch.as_strided(v, (1,), (1,), v.storage_offset() + 5)[0] = 1.0          # column 6 of row 0: inside the span, outside the view
    with pytest.raises(AssertionError, match="between the view's elements"):
        v.check()


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16])
def test_read_past_the_end_is_poison(dtype):
    t = torch.ones(3, 5, dtype=dtype)
    for fill, expect in ((MG.NAN_FILL, "nan"), (MG.BIG_FILL, "big")):
        v = MG.guarded(t, fill=fill)
        past = torch.as_strided(v, (4,), (1,), v.storage_offset() + v.numel()).float()
        before = torch.as_strided(v, (4,), (1,), v.storage_offset() - 4).float()
        for r in (past, before):
            if expect == "nan" or dtype == torch.float16:      # 0x7F7F is a NaN in float16
                assert bool(torch.isnan(r).all())
            else:
                assert bool((r > 3e38).all())


def test_proxy_intercepts_listed_modules_only():
    mod = types.ModuleType("fake_ops")
    mod.torch = torch
    exec("def alloc(x):\n    return torch.empty((2, 3)), torch.empty_like(x), torch.empty(4, dtype=torch.int32), "
         "torch.empty((1, 8, 2, 2), memory_format=torch.channels_last)\n", mod.__dict__)
    other = types.ModuleType("other_ops")
    other.torch = torch
    exec("def alloc():\n    return torch.empty((2, 3))\n", other.__dict__)
    x = torch.zeros(3, 4, 5).permute(2, 0, 1)
    with MG.poisoned_allocations([mod], MG.NAN_FILL, device_types=("cpu",)) as rec:
        a, b, i, cl = mod.alloc(x)
        o = other.alloc()
        assert mod.torch is not torch and other.torch is torch
    assert len(rec) == 4 and not hasattr(o, "_memguard")
    assert bool(torch.isnan(a).all()) and bool(torch.isnan(b).all())
    assert b.stride() == torch.empty_like(x).stride() and cl.stride() == (32, 1, 16, 8)
    assert bool((i == 0).all())                           # integer bodies are never poisoned
    assert mod.torch is torch


def test_proxy_is_removed_after_an_exception():
    mod = types.ModuleType("fake_ops")
    mod.torch = torch
    with pytest.raises(RuntimeError, match="boom"):
        with MG.poisoned_allocations([mod], device_types=("cpu",)):
            raise RuntimeError("boom")
    assert mod.torch is torch


def test_exit_check_names_the_overwritten_allocation():
    mod = types.ModuleType("fake_ops")
    mod.torch = torch
    exec("def bad():\n    y = torch.empty(8)\n    torch.as_strided(y, (9,), (1,), y.storage_offset())[8] = 0\n    return y\n", mod.__dict__)
    with pytest.raises(AssertionError, match=r"bad: empty\(8,\) float32"):
        with MG.poisoned_allocations([mod], device_types=("cpu",)):
            mod.bad()

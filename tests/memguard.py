"""Guarded tensors and poisoned allocations: out-of-bounds reads and writes detected by value.

Most kernels address memory through buffer resources whose bounds are a 2 GiB record count; an address they must not touch
gets a "poisoned" offset >= 2^31.  An offset computed wrongly for a ragged tail therefore reads or writes whatever lies next to
the tensor, and on fresh allocations that is usually zeros or finite leftovers that padding taps multiply by zero.  The helpers
here put every tensor inside one larger allocation whose bytes outside the view hold a poison pattern:

- ``guarded(t, lead, trail, fill)`` -- a tensor with ``t``'s values, shape, dtype and strides, placed ``lead`` bytes into a buffer
  whose other bytes (the guards, and for non-dense views the gaps between rows) are ``fill``.  ``.check()`` asserts the guards
  are intact.
- ``poisoned_allocations(modules, fill)`` -- inside the block, ``torch.empty`` / ``torch.empty_like`` as seen from ``modules``
  return such views with the body poisoned too, so a kernel that reads an output (or a workspace) before writing it, or leaves
  part of it unwritten, yields NaN / 3.4e38 instead of whatever the caching allocator had lying around.  Every allocation's
  guards are checked on exit.

Fills: ``0xFF`` bytes are NaN in f32, bf16 and f16 (shows a read of poison through a sum or product); ``0x7F`` bytes are 3.4e38
in f32 and bf16 (shows it through max / select / fmax reductions, which skip NaN).

Integer allocations (symbols, index tables) are poisoned in their guards only; their bodies are zero-filled so a poisoned value
can never become an address.  ``uint8`` allocations are workspaces or packed weight images: their bodies are poisoned only when
the allocating function is listed in ``POISON_U8_BODIES`` (its kernels were read and hold floating-point data there), and
zero-filled otherwise.

Not intercepted: ``Tensor.new_empty`` (one call site in ``models.py``, a 1x1 probe tensor that is never read by a kernel) and
allocations made by torch itself (``torch.zeros``, results of torch ops).
"""
from __future__ import annotations

import contextlib
import sys

import pytest
import torch

ALIGN = 256            # the caching allocator's alignment: ``lead`` keeps a guarded view's data_ptr() at this alignment (plus ``offset``)
NAN_FILL = 0xFF
BIG_FILL = 0x7F

# functions (by code name) whose uint8 allocations hold floating-point data only -- their bodies are poisoned like float tensors.
# Each was checked against its kernels: the bytes are fp32 partial sums / packed 16-bit or fp32 weights that every launch writes
# before it reads them (no counters, flags or offsets live in them).
POISON_U8_BODIES = {
    "_wide_conv": "split-K fp32 partial tiles (conv_igemm.hip)",
    "conv2d_hilo": "split-K fp32 partial tiles (conv_hilo.hip)",
    "_wide_conv_grads": "wgrad fp32 K-slice partials (wgrad.hip)",
    "_narrow_conv_grads": "sconv wgrad fp32 partials (sconv.hip)",
    "conv3x3_c32_wgrad": "c32 wgrad fp32 per-block partials (enh.hip)",
    "_gdn_backward": "GDN backward fp32 per-block partials (gdn.hip)",
}

_INT_DTYPES = (torch.int8, torch.int16, torch.int32, torch.int64, torch.bool)


def _span(shape, stride):
    """Elements from the view's first to one past its last element (non-negative strides)."""
    if any(s == 0 for s in shape):
        return 0
    return 1 + sum((n - 1) * st for n, st in zip(shape, stride))


class _Guard:
    """The allocation behind one guarded view: ``buf`` (uint8) with the view's bytes at ``[lead, lead + nbytes)``."""

    def __init__(self, name, buf, lead, nbytes, fill, mask):
        self.name, self.buf, self.lead, self.nbytes, self.fill, self.mask = name, buf, lead, nbytes, fill, mask

    def bad(self):
        """bool tensor (one element, on the buffer's device): some guard byte differs from ``fill``."""
        diff = self.buf != self.fill
        if self.mask is not None:
            diff &= self.mask
            return diff.any()
        return diff[:self.lead].any() | diff[self.lead + self.nbytes:].any()

    def check(self):
        diff = self.buf != self.fill
        if self.mask is not None:
            diff &= self.mask
        else:
            diff[self.lead:self.lead + self.nbytes] = False
        idx = torch.nonzero(diff)
        if idx.numel():
            i = int(idx[0, 0])
            where = f"{self.lead - i} bytes before the view" if i < self.lead else \
                f"{i - self.lead - self.nbytes} bytes past the end of its element span" if i >= self.lead + self.nbytes else \
                f"at byte {i - self.lead} of its span, between the view's elements"
            raise AssertionError(f"guard of {self.name} overwritten: {idx.shape[0]} byte(s) differ from 0x{self.fill:02X}, the first "
                                 f"{where} (0x{int(self.buf[i]):02X})")


def _alloc(shape, stride, dtype, device, lead, trail, fill, body_fill, name, offset=0):
    elem = torch.empty((), dtype=dtype).element_size()
    span = _span(shape, stride)
    nbytes = span * elem
    buf = torch.empty(max(lead, 0) + ALIGN + offset + nbytes + trail, dtype=torch.uint8, device=device)
    lead = max(lead, 0) + (-(buf.data_ptr() + max(lead, 0))) % ALIGN + offset      # the view at ALIGN (+ offset) in device memory
    buf.fill_(fill)
    if body_fill is not None and body_fill != fill:
        buf[lead:lead + nbytes].fill_(body_fill)
    view = buf[lead:lead + nbytes].view(dtype).as_strided(tuple(shape), tuple(stride))
    mask = None
    if span != view.numel():                 # gaps inside the span (a cropped view): they are guard bytes too
        inside = torch.zeros(span, dtype=torch.bool, device=device)
        inside[torch.arange(span, device=device).as_strided(tuple(shape), tuple(stride)).reshape(-1)] = True
        mask = torch.ones(buf.numel(), dtype=torch.bool, device=device)
        mask[lead:lead + nbytes] = ~inside.repeat_interleave(elem)
    g = _Guard(name, buf, lead, nbytes, fill, mask)
    view.check = g.check
    view._memguard = g
    return view, g


def guarded(t, lead=4096, trail=4096, fill=NAN_FILL, name="tensor", offset=0):
    """``t``'s values, shape, dtype, strides and device in one larger allocation whose bytes outside the view are ``fill``.

    ``lead`` is raised to put the view on a 256-byte boundary (the allocator's alignment), then ``offset`` bytes are added (the alignment pass places views
    16 or 4 bytes past a boundary).  ``.check()`` on the result asserts every guard byte is still ``fill``."""
    if any(s < 0 for s in t.stride()):
        raise ValueError("guarded: negative strides are not supported")
    view, _ = _alloc(t.shape, t.stride(), t.dtype, t.device, lead, trail, fill, None, name, offset)
    with torch.no_grad():
        view.copy_(t)
    if t.requires_grad:
        view.requires_grad_(True)
    return view


def check_all(tensors):
    """Check the guards of every guarded tensor in ``tensors`` with one device synchronisation (a detailed check on the first bad one)."""
    gs = [getattr(t, "_memguard", None) if torch.is_tensor(t) else t for t in tensors]
    gs = [g for g in gs if g is not None]
    if not gs:
        return
    flags = torch.stack([g.bad().to(gs[0].buf.device) for g in gs]).cpu()
    for g, f in zip(gs, flags.tolist()):
        if f:
            g.check()


class _TorchProxy:
    """Stands in for the ``torch`` module inside the patched modules: ``empty`` / ``empty_like`` allocate guarded, poisoned views;
    everything else is the real module's attribute."""

    def __init__(self, real, fill, device_types, record):
        self._real, self._fill, self._types, self._record = real, fill, device_types, record

    def __getattr__(self, name):
        return getattr(self._real, name)

    def _make(self, shape, stride, dtype, device, requires_grad):
        caller = sys._getframe(2).f_code.co_name
        if dtype in _INT_DTYPES:
            body = 0
        elif dtype == torch.uint8:
            body = self._fill if caller in POISON_U8_BODIES else 0
        else:
            body = self._fill
        t, g = _alloc(shape, stride, dtype, device, 4096, 4096, self._fill, body,
                      f"{caller}: empty{tuple(shape)} {str(dtype).replace('torch.', '')}")
        self._record.append(g)
        if requires_grad:
            t.requires_grad_(True)
        return t

    def empty(self, *size, dtype=None, device=None, memory_format=None, requires_grad=False, **kw):
        real = self._real
        dev = real.device(device) if device is not None else real.device("cpu")
        if kw or dev.type not in self._types:
            return real.empty(*size, dtype=dtype, device=device, memory_format=memory_format, requires_grad=requires_grad, **kw)
        shape = tuple(size[0]) if len(size) == 1 and not isinstance(size[0], int) else tuple(size)
        dtype = dtype or real.get_default_dtype()
        meta = real.empty(shape, dtype=dtype, device="meta",
                          memory_format=memory_format if memory_format is not None else real.contiguous_format)
        return self._make(shape, meta.stride(), dtype, dev, requires_grad)

    def empty_like(self, t, *, dtype=None, device=None, memory_format=None, requires_grad=False, **kw):
        real = self._real
        dev = real.device(device) if device is not None else t.device
        if kw or dev.type not in self._types:
            return real.empty_like(t, dtype=dtype, device=device, memory_format=memory_format if memory_format is not None
                                   else real.preserve_format, requires_grad=requires_grad, **kw)
        meta = real.empty_like(t, dtype=dtype, device="meta",
                               memory_format=memory_format if memory_format is not None else real.preserve_format)
        return self._make(tuple(meta.shape), meta.stride(), meta.dtype, dev, requires_grad)


@contextlib.contextmanager
def poisoned_allocations(modules, fill=NAN_FILL, device_types=("cuda",)):
    """Inside the block, ``torch.empty`` / ``torch.empty_like`` called from any of ``modules`` (through the module's ``torch``
    global) return guarded views with poisoned bodies (see the module docstring for integer and uint8 allocations).  Yields the
    list of allocation guards; on a normal exit every guard is checked.  The patch is undone on every exit."""
    record = []
    proxy = _TorchProxy(torch, fill, tuple(device_types), record)
    with pytest.MonkeyPatch.context() as mp:
        for m in modules:
            mp.setattr(m, "torch", proxy)
        yield record
    check_all(record)

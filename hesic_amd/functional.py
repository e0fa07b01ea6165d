"""Host-side operators over the C ABI (``include/hesic_hip.h``) as ``torch.autograd.Function``s.

Tensors keep the reference's logical NCHW shape; wide feature maps are stored ``channels_last``
(= NHWC in memory, what the kernels want), 3-channel images keep whatever strides they have.
PyTorch is used for device memory, streams and autograd bookkeeping only -- every number on the
path is produced by a HIP kernel of ``libhesic_hip.so``.
"""
from __future__ import annotations

import ctypes as C
import os as _os

import torch

from . import _lib as L

_CL = torch.channels_last
_compute_dtype = torch.float32


def set_compute_dtype(dtype):
    """Storage type of the wide feature maps: torch.float32 (exact-fp32 MFMA, parity mode), torch.bfloat16 (bf16 MFMA, fp32
    accumulate: training and inference) or torch.float16 (IEEE half operands on the matrix cores at the same rate, 11-bit
    significand: INFERENCE -- the default of ``bench.py``).  A 16-bit choice also selects the library built for that format
    (``_lib.use_h16``); packed-weight caches are dropped when the format changes."""
    global _compute_dtype, _cache_epoch
    if dtype not in (torch.float32, torch.bfloat16, torch.float16):
        raise ValueError("compute dtype must be torch.float32, torch.bfloat16 or torch.float16")
    if dtype != torch.float32 and dtype != L.h16_dtype():
        L.use_h16(dtype)
        # A pure library switch moves the FORMAT half of the epoch only: packs whose cache key carries the 16-bit dtype (every conv weight:
        # PackedWeight) keep one entry per format and hit again when the format comes back -- Stage2Trainer alternates f16 inference with a
        # bf16 enhancer step and used to repack all frozen HSIC weights twice per step.  Caches keyed without the dtype see a
        # different tag and rebuild, as before.
        _cache_epoch = (str(dtype), _epoch_n)
    _compute_dtype = dtype


def _h16():
    """torch dtype of the active 16-bit storage format."""
    return L.h16_dtype()


def _is16():
    """True when the compute dtype is one of the 16-bit formats."""
    return _compute_dtype != torch.float32


def compute_dtype():
    return _compute_dtype


def _nhwc(x):
    return x if x.is_contiguous(memory_format=_CL) else x.contiguous(memory_format=_CL)


def _empty_nhwc(b, c, h, w, dtype, device):
    return torch.empty((b, c, h, w), dtype=dtype, device=device, memory_format=_CL)


def _is_narrow(c):
    return c <= 8


class _AllFalse:
    def __getitem__(self, i):
        return False


class _NoCtx:
    """Stand-in for the autograd context when grad mode is off: ``Function.apply`` costs ~10 us of host time per call (16+ calls
    per eval forward) to build a graph node nobody will use; ``_apply`` calls ``forward`` directly then."""
    needs_input_grad = _AllFalse()

    def save_for_backward(self, *tensors):
        pass

    def mark_non_differentiable(self, *tensors):
        pass

    def mark_dirty(self, *tensors):
        pass

    def set_materialize_grads(self, value):
        pass


_autograd_depth = 0          # > 0 while an autograd.Function of this module runs its forward on behalf of a grad-enabled call


def _apply(fn, *args):
    global _autograd_depth
    if torch.is_grad_enabled():
        if _compute_dtype == torch.float16 and any(torch.is_tensor(a) and a.requires_grad for a in args):
            raise RuntimeError("hesic_amd: float16 is an inference format here (gradients need the fp32 exponent range): train with "
                               "set_compute_dtype(torch.bfloat16) or torch.float32, or run the forward under torch.no_grad()")
        _autograd_depth += 1
        try:
            return fn.apply(*args)
        finally:
            _autograd_depth -= 1
    return fn.forward(_NoCtx(), *args)


def inference_call():
    """True when the current operator call is a plain inference call: grad mode off, NOT the forward of an autograd.Function reached from a
    grad-enabled call (grad mode is off inside ``Function.forward`` too) and not a backward pass.  The error-feedback ("shaped") weight packs are
    inference-only: a training forward outside ``Trainer.step`` must multiply the plainly rounded weights its backward differentiates."""
    return not torch.is_grad_enabled() and _autograd_depth == 0 and torch._C._current_graph_task_id() < 0


FUSE_GDN3 = True      # module switch (tests / profiling): 3-channel (I)GDN inside the 6 -> 3 cat-conv launch


def _c(t):
    """``t`` for its pointer: contiguous storage without the ~5 us ``detach()`` + ``contiguous()`` make of a new tensor object per
    launch (parameters are contiguous leaves; ``data_ptr()`` needs no detach)."""
    return t if t.is_contiguous() else t.detach().contiguous()


def _nd(t):
    return t.detach() if t.requires_grad else t


def _zeros(shape, dtype, device):
    """Zero-filled scratch for kernels that ACCUMULATE into it.  ``torch.zeros`` is a hipMemsetAsync on ROCm, and a memset
    node recorded into a HIP graph did not reliably run before the accumulating kernel on replays (see csrc/wgrad.hip:
    zero_async); ``fill_`` is an ordinary kernel and keeps its place in the stream in eager and graph mode alike."""
    return torch.empty(shape, dtype=dtype, device=device).fill_(0)


# ------------------------------------------------------------------------------ flat gradient slots
# train.FlatGroup keeps the gradients of all parameters of an optimiser group in ONE flat fp32 buffer (cleared by one
# launch per step, reduced over ranks in place, read by one Adam launch); every ``p.grad`` is a view into it.  The
# backward passes below look the parameter up here (by storage address: saved tensors come back as fresh wrappers) and, if
# it has a slot, ADD their gradient into it directly -- K-slice reduce, layout change and accumulation in the finishing
# kernel -- and hand ``None`` to autograd: no unpack kernel, no AccumulateGrad copy / add per parameter.
class GradSlot:
    __slots__ = ("grad", "writes", "on_write", "name", "param")

    def __init__(self, grad, name=""):
        self.grad, self.writes, self.on_write, self.name, self.param = grad, 0, None, name, None


_grad_slots = {}


def register_grad_slots(slots):
    """``slots``: iterable of (parameter, GradSlot).  Replaces any slot registered for the same storage address; returns the
    registered addresses (for ``clear_grad_slots``)."""
    import weakref
    keys = []
    for p, s in slots:
        s.param = weakref.ref(p)
        _grad_slots[p.data_ptr()] = s
        keys.append(p.data_ptr())
    return keys


def clear_grad_slots(keys=None):
    if keys is None:
        _grad_slots.clear()
    else:
        for k in keys:
            _grad_slots.pop(k, None)


_slots_active = False


# Deferred finishing passes of the wide weight gradients (see _wide_conv_grads): a list while train.Trainer.step collects them
_finish_queue = None
GDN_FINISH_BATCH = True      # module switch: False = one parameter finish per GDN backward (rounds 2-4)
WGRAD_FINISH_BATCH = 8     # module switch: 0 = one finishing launch per layer (rounds 2-3)
# round 5: the split-K launches of the queued layers are deferred too and share grids (hesic_conv2d_wgrad_partial_batched); 0 = each layer's
# split-K launch where its backward runs, only the finishing pass batched (A/B)
WGRAD_PARTIAL_BATCH = True


def defer_wgrad_finish(on):
    """Gate of the batched finishing pass; returns the previous state.  Turning it off flushes what is queued."""
    global _finish_queue
    prev = _finish_queue is not None
    if not on:
        flush_wgrad_finish()
        _finish_queue = None
    elif _finish_queue is None and WGRAD_FINISH_BATCH > 0:
        _finish_queue = []
        _gdn_finish_queue.clear()          # jobs a failed step left behind must not be finished into this one
    return prev


# a queued conv weight gradient: descriptor, split-K workspace, dY, gradient slots of weight / bias, the weight slot's address (two jobs on one
# gradient never share a launch), and -- when the split-K launch itself is deferred -- the conv input, the workspace size and the K-slice count
_WgJob = __import__("collections").namedtuple("_WgJob", "desc ws gy wslot bslot dwp x nws nsplit")
# a fused GDN backward whose parameter finish is pending
_GdnJob = __import__("collections").namedtuple("_GdnJob", "ws P beta gamma slot_beta slot_gamma beta_min")
_gdn_finish_queue = []


def flush_gdn_finish():
    """One ``hesic_gdn_param_finish_batched`` call for the queued GDN backwards (round 5: 15 six-microsecond launches per step before)."""
    if not _gdn_finish_queue:
        return
    q = list(_gdn_finish_queue)
    _gdn_finish_queue.clear()
    n = len(q)
    vp, i64, f32 = C.c_void_p * n, C.c_int64 * n, C.c_float * n
    L.call("hesic_gdn_param_finish_batched", n, vp(*[j.ws.data_ptr() for j in q]), i64(*[j.P for j in q]), vp(*[j.beta.data_ptr() for j in q]),
           vp(*[j.gamma.data_ptr() for j in q]), vp(*[j.slot_gamma.grad.data_ptr() for j in q]), vp(*[j.slot_beta.grad.data_ptr() for j in q]),
           f32(*[j.beta_min for j in q]), 1, L.stream())
    for j in q:
        _slot_done(j.slot_beta)
        _slot_done(j.slot_gamma)


def flush_wgrad_finish():
    """One ``hesic_conv2d_wgrad_finish_batched`` call for the queued layers, on the current stream (the stream their split-K launches
    went to); the gradient slots report afterwards, so a bucket's all-reduce is still issued behind its last finishing launch."""
    flush_gdn_finish()
    if not _finish_queue:
        return
    q = list(_finish_queue)
    _finish_queue.clear()          # first: a call that fails below must not leave its jobs for the next step
    n = len(q)
    descs = (L.ConvDesc * n)(*[j.desc for j in q])
    vp = C.c_void_p * n
    ws = vp(*[j.ws.data_ptr() for j in q])
    dy = vp(*[j.gy.data_ptr() for j in q])
    pend = [j for j in q if j.x is not None]
    if pend:          # jobs whose split-K launch was deferred: the shared grids of hesic_conv2d_wgrad_partial_batched
        m = len(pend)
        vm = C.c_void_p * m
        L.call("hesic_conv2d_wgrad_partial_batched", m, (L.ConvDesc * m)(*[j.desc for j in pend]), vm(*[j.x.data_ptr() for j in pend]),
               vm(*[j.gy.data_ptr() for j in pend]), vm(*[j.ws.data_ptr() for j in pend]), (C.c_int64 * m)(*[j.nws for j in pend]),
               (C.c_int32 * m)(*[j.nsplit for j in pend]), L.stream())
    dw = vp(*[j.wslot.grad.data_ptr() for j in q])
    db = vp(*[(j.bslot.grad.data_ptr() if j.bslot is not None else None) for j in q])
    L.call("hesic_conv2d_wgrad_finish_batched_n", n, descs, ws, dy, dw, db, 1, (C.c_int32 * n)(*[j.nsplit for j in q]), L.stream())
    for j in q:
        _slot_done(j.wslot)
        if j.bslot is not None:
            _slot_done(j.bslot)


def grad_slots_active(on):
    """Gate of the direct-write path.  Only inside ``train.Trainer.step`` (which clears the flat buffer first and reads it with
    its own optimiser) do the gradient kernels add into the slots and hand ``None`` to autograd; everywhere else -- a plain
    ``loss.backward()``, ``torch.autograd.grad``, tensor / DDP hooks on the parameters -- gradients are returned to autograd as
    usual (``p.grad`` is still the slot view, so AccumulateGrad lands in the flat buffer all the same)."""
    global _slots_active
    prev, _slots_active = _slots_active, bool(on)
    return prev


def _slot_for(t):
    if t is None or not _grad_slots or not _slots_active:
        return None
    s = _grad_slots.get(t.data_ptr())
    if s is None:
        return None
    owner = s.param() if s.param is not None else None
    if owner is None or owner.data_ptr() != t.data_ptr():       # the parameter is gone (its address may have been reused)
        _grad_slots.pop(t.data_ptr(), None)
        return None
    return s if s.grad.shape == t.shape and s.grad.device == t.device else None


def _slot_done(slot):
    slot.writes += 1
    if slot.on_write is not None:
        slot.on_write(slot)


# ------------------------------------------------------------------------------ packing cache
_epoch_n = 0
_cache_epoch = (str(L.h16_dtype()), 0)       # (active 16-bit format, invalidation count): compared for equality inside the cache tags
SHAPED_WEIGHTS = _os.environ.get("HESIC_SHAPED_WEIGHTS", "1") != "0"      # A/B switch for PackedWeight(shaped=True)


def invalidate_weight_cache():
    """Forget every packed inference weight (call after changing parameters through an API that does not bump
    the tensor version counter, e.g. a fused optimiser step issued under ``torch.no_grad()`` outside training)."""
    global _cache_epoch, _epoch_n
    _epoch_n += 1
    _cache_epoch = (_cache_epoch[0], _epoch_n)


# Training-step pack registry (used by train.Trainer): with ``train_pack_cache(True)`` the packers keep one persistent
# packed buffer per (layer, layout) also in grad mode and register it here; ``repack_all()`` then refreshes every
# registered buffer with ONE launch (hesic_pack_conv_weights_batched) right after the optimiser update, instead of ~70
# separate 7 us launches spread over the next forward/backward.  Outside that mode training re-packs on every call.
_train_pack_cache = False
_pack_registry = []            # entries: dict(weight, mask, wp, dims..., owner, key)
_pack_table = None             # (signature, device job table, n_jobs, total_blocks)
_gdn_registry = []             # PackedGdn objects holding a persistent training pack
_gdn_table = None              # (signature, device job table, n_jobs)


def train_pack_cache(on):
    global _train_pack_cache
    prev, _train_pack_cache = _train_pack_cache, bool(on)
    return prev


def _repack_gdns():
    """The registered GDN parameter packs (PackedGdn, Trainer step) refreshed in one launch."""
    global _gdn_table
    ents = [g for g in _gdn_registry if g._train is not None and g._train["beta"]() is not None and g._train["gamma"]() is not None]
    if len(ents) != len(_gdn_registry):
        _gdn_registry[:] = ents
    if not ents:
        return 0
    import numpy as np
    sig = tuple((g._train["beta"]().data_ptr(), g._train["gamma"]().data_ptr(), g._train["gp"].data_ptr()) for g in ents)
    if _gdn_table is None or _gdn_table[0] != sig:
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError("repack_all: the set of packed GDN parameters changed during HIP-graph capture; run a warm-up step first")
        jobs = np.zeros(len(ents), dtype=np.dtype([("beta", "<u8"), ("gamma", "<u8"), ("gp", "<u8"), ("bp", "<u8"), ("beta_min", "<f4"), ("pad", "<i4")]))
        for i, g in enumerate(ents):
            t = g._train
            jobs[i] = (t["beta"]().data_ptr(), t["gamma"]().data_ptr(), t["gp"].data_ptr(), t["bp"].data_ptr(), t["beta_min"], 0)
        _gdn_table = (sig, torch.from_numpy(jobs.view(np.uint8).copy()).to(ents[0]._train["gp"].device), len(ents))
    _, table, n = _gdn_table
    L.call("hesic_gdn_pack_params_batched", L.ptr(table), n, L.stream())
    for g in ents:
        t = g._train
        t["tag"] = (t["beta"]().data_ptr(), t["gamma"]().data_ptr(), t["beta"]()._version, t["gamma"]()._version, _cache_epoch)
    return n


def repack_all():
    """Refresh every registered packed weight (and GDN parameter pack) from its parameter in one launch each and mark it current."""
    global _pack_table
    _repack_gdns()
    ents = [e for e in _pack_registry if e["weight"]() is not None]
    if len(ents) != len(_pack_registry):
        _pack_registry[:] = ents
    if not ents:
        return 0
    import numpy as np
    sig = tuple((e["weight"]().data_ptr(), 0 if e["mask"] is None else e["mask"].data_ptr(), e["wp"].data_ptr()) for e in ents)
    if _pack_table is None or _pack_table[0] != sig:
        if torch.cuda.is_current_stream_capturing():
            # the job table is uploaded from host memory: never from inside a graph capture (warm-up steps build it)
            raise RuntimeError("repack_all: the set of packed weights changed during HIP-graph capture; run a warm-up step first")
        jobs = np.zeros(len(ents), dtype=np.dtype([("w", "<u8"), ("mask", "<u8"), ("wp", "<u8"), ("Cout", "<i4"), ("Cin", "<i4"), ("KH", "<i4"),
                                                      ("KW", "<i4"), ("transposed", "<i4"), ("flip", "<i4"), ("dtype", "<i4"), ("block0", "<i4")]))
        blk = 0
        for i, e in enumerate(ents):
            w = e["weight"]()
            jobs[i] = (w.data_ptr(), 0 if e["mask"] is None else e["mask"].data_ptr(), e["wp"].data_ptr(), e["cout"], e["cin"], e["kh"], e["kw"],
                       int(e["transposed"]), int(e["flip"]), L.dt(e["dtype"]), blk)
            blk += ((e["cout"] + 7) // 8) * ((e["cin"] + 31) // 32)          # one block per 8-cout x 32-cin tile
        dev = ents[0]["wp"].device
        table = torch.from_numpy(jobs.view(np.uint8).copy()).to(dev)
        _pack_table = (sig, table, len(ents), blk)
    _, table, n, blk = _pack_table
    L.call("hesic_pack_conv_weights_batched", L.ptr(table), n, blk, L.stream())
    _mark_packs_current(ents)
    return n


def _mark_packs_current(ents):
    for e in ents:
        w = e["weight"]()
        e["owner"]._cache[e["key"]] = ((w.data_ptr(), w._version, None if e["mask"] is None else e["mask"]._version, _cache_epoch), e["wp"])


def packs_replayed(params):
    """After a graph replay whose captured ``repack_all()`` refreshed them on the device: mark the registered packs of ``params`` current,
    the host half of ``repack_all()`` that a replay does not run (call it after bumping the parameters' version counters).  The packers
    then keep handing out the buffers the graph reads and writes by address -- an eager step or an eval forward between two replays
    allocates no replacement for them."""
    mine = {id(p) for p in params}
    _mark_packs_current([e for e in _pack_registry if e["weight"]() is not None and id(e["weight"]()) in mine])


class PackedWeight:
    """Device copy of a conv weight in the kernels' [tap][Cout][Cin] layout.

    Inference (grad mode off): cached, refreshed when the parameter's version counter or storage moves.
    Training (grad mode on): re-packed on every call and the inference cache is dropped -- fused optimisers
    update parameters without touching the version counter, and a 35 M-parameter repack is ~50 us.  Under
    ``train_pack_cache(True)`` (the Trainer's step) the packed buffer is persistent, registered for ``repack_all()`` and
    reused while its (storage, version, epoch) tag is current."""

    def __init__(self, shaped=False, tr_stride=0):
        self._cache = {}
        # ``shaped``: at 16-bit INFERENCE a Conv2d weight is rounded with error feedback over the taps of each (cout, cin) pair
        # (``hesic_pack_conv_weight_shaped``) -- for layers whose input is a spatially smooth feature map (g_a_conv2..4); a ConvTranspose2d
        # weight (``tr_stride`` = its stride; round 5: the synthesis stacks) inside each output phase's tap class
        self.shaped, self.tr_stride = shaped, int(tr_stride)

    def get(self, weight, mask, cout, cin, kh, kw, transposed, flip, dtype):
        # autograd.Function bodies run with grad mode off, so a training step also takes the cached branch (one repack
        # per layout and step, when the version tag moves)
        caching = not torch.is_grad_enabled()
        # an inference pack with error-feedback rounding and the plain pack of a training forward / backward are different images of one weight
        key = (transposed, flip, dtype, cout, cin, bool(self.shaped and SHAPED_WEIGHTS and inference_call() and not _train_pack_cache))
        tag = (weight.data_ptr(), weight._version, None if mask is None else mask._version, _cache_epoch)
        hit = None
        if caching:
            hit = self._cache.get(key)
            if hit is not None and hit[0] == tag:
                return hit[1]
        elif self._cache:
            self._cache.clear()
        wref = None
        if caching and _train_pack_cache:
            # the parameter behind this tensor: the tensor itself in a forward, the forward's registration in a backward
            # (saved tensors come back as fresh wrappers around the parameter's storage)
            if isinstance(weight, torch.nn.Parameter):
                wref = __import__("weakref").ref(weight)
            else:
                for e in _pack_registry:
                    w0 = e["weight"]()
                    if e["owner"] is self and w0 is not None and w0.data_ptr() == weight.data_ptr() and w0.shape == weight.shape:
                        wref = e["weight"]
                        break
        if wref is not None:
            # Trainer step: persistent buffer, registered for the batched repack that follows the optimiser update
            reuse = hit is not None and hit[1].device == weight.device and hit[1].dtype == dtype
            wp = hit[1] if reuse else torch.empty(kh * kw * cout * cin, dtype=dtype, device=weight.device)
            L.call("hesic_pack_conv_weight", L.ptr(weight.detach()), L.ptr(mask), L.ptr(wp), cout, cin, kh, kw,
                   int(transposed), int(flip), L.dt(dtype), L.stream())
            for e in _pack_registry:
                if e["owner"] is self and e["key"] == key:
                    e["wp"], e["weight"], e["mask"] = wp, wref, mask
                    break
            else:
                _pack_registry.append({"weight": wref, "mask": mask, "wp": wp, "cout": cout, "cin": cin, "kh": kh, "kw": kw,
                                       "transposed": transposed, "flip": flip, "dtype": dtype, "owner": self, "key": key})
            self._cache[key] = (tag, wp)
            return wp
        wp = torch.empty(kh * kw * cout * cin, dtype=dtype, device=weight.device)
        if (self.shaped and SHAPED_WEIGHTS and caching and inference_call() and not _train_pack_cache and dtype != torch.float32 and mask is None and not transposed
                and not flip and kh * kw > 1 and weight.dtype == torch.float32 and weight.is_contiguous()):
            L.call("hesic_pack_conv_weight_shaped", L.ptr(weight.detach()), L.ptr(wp), cout, cin, kh, kw, L.stream())
        elif (self.shaped and self.tr_stride and SHAPED_WEIGHTS and caching and inference_call() and not _train_pack_cache and dtype != torch.float32 and mask is None
                and transposed and not flip and kh * kw > 1 and weight.dtype == torch.float32 and weight.is_contiguous()):
            L.call("hesic_pack_conv_weight_shaped_tr", L.ptr(weight.detach()), L.ptr(wp), cout, cin, kh, kw, self.tr_stride, L.stream())
        else:
            L.call("hesic_pack_conv_weight", L.ptr(weight.detach()), L.ptr(mask), L.ptr(wp), cout, cin, kh, kw,
                   int(transposed), int(flip), L.dt(dtype), L.stream())
        if caching:
            self._cache[key] = (tag, wp)
        return wp


_img_cache = {}


def _weight_image(kind, weight, gp=None, gtag=None):
    """LDS weight image of an image-side MFMA kernel (``hesic_sconv_pack_weight_image``), cached per weight (+ GDN parameters)
    version: kind 0 = g_a_conv1 + GDN (64 KB, needs the packed gamma'), kind 1 = g_s_conv4 (24 KB).  The entry remembers the
    tensor OBJECT (weak reference): an address / version pair alone would also match a new tensor allocated where a dead one was."""
    import weakref
    key = (kind, weight.data_ptr())
    tag = (weight._version, gtag, _cache_epoch)
    hit = _img_cache.get(key)
    if hit is not None and hit[0] == tag and hit[2]() is weight:
        return hit[1]
    if kind == 1 and SHAPED_WEIGHTS and inference_call() and not _train_pack_cache:
        kind = 2          # inference: g_s_conv4's panel rounded with error feedback per output phase (csrc/sconv.hip, round 5)
        key = (kind, weight.data_ptr())
        hit = _img_cache.get(key)
        if hit is not None and hit[0] == tag and hit[2]() is weight:
            return hit[1]
    img = torch.empty(65536 if kind == 0 else 24576, dtype=torch.uint8, device=weight.device)
    L.call("hesic_sconv_pack_weight_image", kind, L.ptr(_c(weight)), L.ptr(gp), L.ptr(img), L.stream())
    if len(_img_cache) > 64:
        _img_cache.clear()
    try:
        _img_cache[key] = (tag, img, weakref.ref(weight))
    except TypeError:
        pass
    return img


def _wide_conv(x, wp, bias, B, H, W, Cin, Ho, Wo, Cout, k, stride, pad, transposed, act=0, in_abs=0, tap_mask=0,
               out=None, out_c_off=0, x_c_off=0, f32_out=None):
    """Launch the implicit-GEMM kernel. ``x`` NHWC (may be wider than Cin), returns / fills NHWC ``out``.
    ``f32_out`` ("only" | "both", bf16 storage): also / only store the output as fp32 from the fp32 accumulators
    (``hesic_conv2d_forward_f32out``); returns ``(out | None, out_f32)`` then."""
    dtype = x.dtype
    if out is None and f32_out != "only":
        out = _empty_nhwc(B, Cout, Ho, Wo, dtype, x.device)
    y_ps, y_co = (out.shape[1], out_c_off) if out is not None else (Cout, 0)
    d = L.ConvDesc(B, H, W, Cin, Ho, Wo, Cout, k, k, stride, pad, int(transposed), L.dt(dtype), act, in_abs,
                   x.shape[1], x_c_off, y_ps, y_co, tap_mask)
    key = (B, H, W, Cin, Ho, Wo, Cout, k, stride, pad, int(transposed), L.dt(dtype), tap_mask, bool(f32_out))
    need = _ws_bytes.get(key)
    if need is None:      # a launch with an fp32 latent output decides its K split per image: its own query
        need = _ws_bytes[key] = int((L.lib().hesic_conv2d_f32out_ws_bytes if f32_out else L.lib().hesic_conv2d_ws_bytes)(C.byref(d)))
    ws = None
    if need and SPLIT_K:      # low-resolution layer: split-K launch, fp32 partial tiles in a scratch buffer
        ws = torch.empty(need, dtype=torch.uint8, device=x.device)
    if f32_out:
        out32 = _empty_nhwc(B, Cout, Ho, Wo, torch.float32, x.device)
        L.call("hesic_conv2d_forward_f32out", C.byref(d), L.ptr(x), L.ptr(wp), L.ptr(bias), L.ptr(out), L.ptr(out32), Cout, 0,
               L.ptr(ws), need if ws is not None else 0, L.stream())
        return out, out32
    if ws is not None:
        L.call("hesic_conv2d_forward_ws", C.byref(d), L.ptr(x), L.ptr(wp), L.ptr(bias), L.ptr(out), L.ptr(ws), need, L.stream())
    else:
        L.call("hesic_conv2d_forward", C.byref(d), L.ptr(x), L.ptr(wp), L.ptr(bias), L.ptr(out), L.stream())
    return out


_ws_bytes = {}
SPLIT_K = True


class no_split_k:
    """Context manager: run the convs inside with one block per output tile (no split-K).  A split-K launch sums its K
    slices in a different order than the plain launch, so results depend (in the last bit) on which launch a SHAPE gets;
    the bit-stream codec, whose decoder re-evaluates the encoder's full-map convolutions one pixel at a time, needs
    shape-independent numbers."""

    def __enter__(self):
        global SPLIT_K
        self._prev, SPLIT_K = SPLIT_K, False

    def __exit__(self, *exc):
        global SPLIT_K
        SPLIT_K = self._prev


def _sdesc(x, y, Cin, Cout, k, stride, pad, transposed, act=0):
    B, _, H, W = x.shape
    _, _, Ho, Wo = y.shape
    xs, ys = x.stride(), y.stride()
    return L.SConvDesc(B, H, W, Cin, Ho, Wo, Cout, k, k, stride, pad, int(transposed), L.dt(x), L.dt(y), act, 0,
                       xs[0], xs[1], xs[2], xs[3], ys[0], ys[1], ys[2], ys[3])


def _out_hw(H, W, k, stride, pad, transposed):
    if transposed:
        f = lambda n: (n - 1) * stride - 2 * pad + k + stride - 1
    else:
        f = lambda n: (n + 2 * pad - k) // stride + 1
    return f(H), f(W)


def _narrow_conv_grads(x, weight, gy, cfg, dims, has_bias, need_dx, need_dw, bias=None, ydt=None):
    """dx / dw / dbias of an image-side conv (few channels on one side: strided kernels).  ``ydt``: the storage type the forward gave its
    output (``_ConvFn`` keeps it: the global compute dtype may have been restored to something else by the time the backward runs)."""
    k, stride, pad, transposed, act, in_abs, tap_mask, packer, mask = cfg
    B, H, W, Cin, Ho, Wo, Cout = dims
    dx = dw = db = None
    if ydt is None:
        ydt = torch.float32 if _is_narrow(Cout) else (_compute_dtype if _is_narrow(Cin) else x.dtype)
    gy = gy.to(ydt)
    gy = gy.contiguous() if _is_narrow(Cout) else _nhwc(gy)
    w = (weight.detach() if mask is None else weight.detach() * mask).contiguous()
    d = _sdesc(x, gy, Cin, Cout, k, stride, pad, transposed)
    if need_dx:
        dx = torch.empty_like(x)
        L.call("hesic_sconv2d_dgrad", C.byref(d), L.ptr(gy), L.ptr(w), L.ptr(dx), L.stream())
        if in_abs:
            dx = dx * torch.sign(x)
    if need_dw:
        # flat gradient slots: the kernel overwrites, so it may write the slot itself only while the (cleared) slot is untouched
        ws_, bs_ = (_slot_for(weight) if mask is None else None), _slot_for(bias) if has_bias else None
        w_direct = ws_ is not None and ws_.writes == 0 and weight.dtype == torch.float32
        b_direct = bs_ is not None and bs_.writes == 0
        dw = ws_.grad if w_direct else torch.empty_like(weight, dtype=torch.float32)
        db = (bs_.grad if b_direct else torch.empty(Cout, dtype=torch.float32, device=x.device)) if has_bias else None
        nws = L.lib().hesic_sconv2d_wgrad_ws_bytes(C.byref(d))
        ws = torch.empty(nws, dtype=torch.uint8, device=x.device) if nws else None
        L.call("hesic_sconv2d_wgrad", C.byref(d), L.ptr(x), L.ptr(gy), L.ptr(dw), L.ptr(db), L.ptr(ws), nws, L.stream())
        if mask is not None:
            dw = dw * mask
        if ws_ is not None:
            if not w_direct:
                ws_.grad.add_(dw)
            _slot_done(ws_)
            dw = None
        if bs_ is not None:
            if not b_direct:
                bs_.grad.add_(db)
            _slot_done(bs_)
            db = None
    return dx, dw, db


def _wide_conv_grads(x, weight, gy, cfg, dims, has_bias, need_dx, need_dw, bias=None):
    """dx / dw / dbias of a wide conv (implicit-GEMM kernels): shared by _ConvFn and _ConvGdnFn.  The weight gradient is one
    split-K MFMA launch + one finishing launch that reduces the K slices, writes the PyTorch layout and sums dY's columns
    for the bias (``hesic_conv2d_wgrad_direct``)."""
    k, stride, pad, transposed, act, in_abs, tap_mask, packer, mask = cfg
    B, H, W, Cin, Ho, Wo, Cout = dims
    dx = dw = db = None
    gy = _nhwc(gy.to(x.dtype))
    if need_dx:
        # data gradient = the opposite op with the same weight tensor read in the other layout
        if Cout % 32 == 0 and Cin % 8 == 0:
            wp = packer.get(weight, mask, Cin, Cout, k, k, not transposed, False, x.dtype)
            dx = _wide_conv(gy, wp, None, B, Ho, Wo, Cout, H, W, Cin, k, stride, pad, not transposed)
        else:   # odd channel counts (parity tests only): strided VALU kernel
            w = (weight.detach() if mask is None else weight.detach() * mask).contiguous()
            dx = torch.empty_like(x, memory_format=_CL)
            d = _sdesc(x, gy, Cin, Cout, k, stride, pad, transposed)
            L.call("hesic_sconv2d_dgrad", C.byref(d), L.ptr(gy), L.ptr(w), L.ptr(dx), L.stream())
        if in_abs:
            dx = dx * torch.sign(x)
    if need_dw:
        db = torch.empty(Cout, dtype=torch.float32, device=x.device) if has_bias else None
        d = L.ConvDesc(B, H, W, Cin, Ho, Wo, Cout, k, k, stride, pad, int(transposed), L.dt(x), 0, in_abs,
                       x.shape[1], 0, gy.shape[1], 0, tap_mask)
        nws = L.lib().hesic_conv2d_wgrad_ws_bytes(C.byref(d))
        ws_, bs_ = _slot_for(weight), (_slot_for(bias) if has_bias else None)
        if ws_ is not None and weight.dtype == torch.float32 and (not has_bias or bs_ is not None) and (mask is None or tap_mask):
            # flat gradient buffer: the finishing kernel adds dW (PyTorch layout) and dbias into the slots, on the stream of the backward
            # pass: the two gradients of a twice-used weight (encoder1) add into their slot in order
            nsp = 0
            if _finish_queue is not None and WGRAD_PARTIAL_BATCH:
                # the shared-grid route: its own (smaller) K-slice count, named to both batched calls; the workspace is sized for it
                nsp = L.lib().hesic_conv2d_wgrad_nsplit(C.byref(d), 1)
                nws = L.lib().hesic_conv2d_wgrad_ws_bytes_n(C.byref(d), nsp)
            ws = torch.empty(max(nws, 16), dtype=torch.uint8, device=x.device)
            if _finish_queue is not None:
                # deferred finishing pass (train.Trainer.step): only the split-K MFMA launch now; the K-slice reduce + layout change +
                # bias column sums of up to 8 layers share one launch (flush_wgrad_finish).  The job keeps ws and gy alive until then.
                dwp = ws_.grad.data_ptr()
                if len(_finish_queue) >= WGRAD_FINISH_BATCH or any(j.dwp == dwp for j in _finish_queue) or (_finish_queue and _finish_queue[0].desc.dtype != d.dtype):
                    flush_wgrad_finish()
                if WGRAD_PARTIAL_BATCH:
                    _finish_queue.append(_WgJob(d, ws, gy, ws_, bs_ if has_bias else None, dwp, x, nws, nsp))      # x stays alive until the flush
                else:
                    L.call("hesic_conv2d_wgrad_partial", C.byref(d), L.ptr(x), L.ptr(gy), L.ptr(ws), nws, L.stream())
                    _finish_queue.append(_WgJob(d, ws, gy, ws_, bs_ if has_bias else None, dwp, None, nws, 0))
                return dx, None, None
            L.call("hesic_conv2d_wgrad_direct", C.byref(d), L.ptr(x), L.ptr(gy), L.ptr(ws_.grad), L.ptr(bs_.grad if has_bias else None), 1,
                   L.ptr(ws), nws, L.stream())
            _slot_done(ws_)
            if has_bias:
                _slot_done(bs_)
            return dx, None, None
        ws = torch.empty(max(nws, 16), dtype=torch.uint8, device=x.device)
        dw = torch.empty(weight.shape, dtype=torch.float32, device=x.device)      # dead taps of a masked conv are zero-filled by the call
        L.call("hesic_conv2d_wgrad_direct", C.byref(d), L.ptr(x), L.ptr(gy), L.ptr(dw), L.ptr(db), 0, L.ptr(ws), nws, L.stream())
        if mask is not None and not tap_mask:
            dw = dw * mask
    return dx, dw, db


_det_conv_grads = False


class deterministic_conv_grads:
    """``with deterministic_conv_grads():`` -- convs whose FORWARD runs inside the block take the order-fixed bias gradient
    (``hesic_bias_grad``) and, for a 3x3 conv with two input channels, the order-fixed weight gradient (``hesic_narrow_in_wgrad``) in their
    backward, wherever that runs: the usual kernels end those two sums in float atomics, whose last bits change from run to run.
    ``homography.Net`` uses it with grad mode on (bit-identical steps and resumes); nothing else does, and outside it every conv launches
    what it always did."""

    def __enter__(self):
        global _det_conv_grads
        self._prev, _det_conv_grads = _det_conv_grads, True

    def __exit__(self, *exc):
        global _det_conv_grads
        _det_conv_grads = self._prev


def _det_target(param, shape, device):
    """(buffer, slot, accumulate) of an order-fixed gradient under the flat-slot protocol: the slot's buffer (added to once it has been
    written) or a fresh tensor."""
    slot = _slot_for(param)
    if slot is not None:
        return slot.grad, slot, int(slot.writes > 0)
    return torch.empty(shape, dtype=torch.float32, device=device), None, 0


def _det_conv_param_grads(ctx, x, weight, gy):
    """The order-fixed part of a conv's parameter gradients: (dw or None, db or None, dw_done, db_done).  ``gy``: NHWC, after the activation's
    backward."""
    k, stride, pad, transposed, act, in_abs, tap_mask, packer, mask = ctx.cfg
    B, H, W, Cin, Ho, Wo, Cout = ctx.dims
    dw = db = None
    dw_done = db_done = False
    if _is_narrow(Cout) or 256 % Cout or not gy.is_contiguous(memory_format=_CL):
        return dw, db, dw_done, db_done
    if ctx.has_bias and ctx.needs_input_grad[2]:
        db, slot, acc = _det_target(ctx.bias, (Cout,), gy.device)
        ws = torch.empty(L.DET_MAX_BLOCKS * Cout, dtype=torch.float32, device=gy.device)
        L.call("hesic_bias_grad", L.ptr(gy), L.ptr(db), L.ptr(ws), B * Ho * Wo, Cout, acc, L.dt(gy), L.stream())
        if slot is not None:
            _slot_done(slot)
            db = None
        db_done = True
    if (ctx.narrow and ctx.needs_input_grad[1] and Cin == 2 and k == 3 and stride == 1 and pad == 1 and not transposed and mask is None and not in_abs
            and x.dtype == torch.float32 and x.is_contiguous() and weight.dtype == torch.float32):
        dw, slot, acc = _det_target(weight, weight.shape, gy.device)
        ws = torch.empty(L.DET_MAX_BLOCKS * Cout * Cin * 9, dtype=torch.float32, device=gy.device)
        L.call("hesic_narrow_in_wgrad", L.ptr(x), L.ptr(gy), L.ptr(dw), L.ptr(ws), B, Cin, H, W, Cout, acc, L.dt(gy), L.stream())
        if slot is not None:
            _slot_done(slot)
            dw = None
        dw_done = True
    return dw, db, dw_done, db_done


class _ConvFn(torch.autograd.Function):
    """conv()/deconv() of compressai/models/utils.py:104-118 (+ MaskedConv2d, layers.py:21-45)."""

    @staticmethod
    def forward(ctx, x, weight, bias, cfg):
        L.require_cuda(x, weight)
        k, stride, pad, transposed, act, in_abs, tap_mask, packer, mask = cfg
        if transposed:
            Cin, Cout = weight.shape[0], weight.shape[1]
        else:
            Cout, Cin = weight.shape[0], weight.shape[1]
        B, Cx, H, W = x.shape
        if Cx != Cin:
            raise RuntimeError(f"conv: expected {Cin} input channels, got {Cx}")
        Ho, Wo = _out_hw(H, W, k, stride, pad, transposed)
        narrow = _is_narrow(Cin) or _is_narrow(Cout) or Cin % 32 or Cout % 8 or (transposed and (Ho != H * stride))
        ctx.cfg, ctx.narrow, ctx.dims = cfg, narrow, (B, H, W, Cin, Ho, Wo, Cout)
        if narrow:
            ydt = ctx.ydt = torch.float32 if _is_narrow(Cout) else (_compute_dtype if _is_narrow(Cin) else x.dtype)
            if not _is_narrow(Cin):
                x = _nhwc(x)
            y = _empty_nhwc(B, Cout, Ho, Wo, ydt, x.device) if not _is_narrow(Cout) else \
                torch.empty((B, Cout, Ho, Wo), dtype=ydt, device=x.device)
            w = weight.detach() if mask is None else (weight.detach() * mask)
            d = _sdesc(x, y, Cin, Cout, k, stride, pad, transposed, act)
            if transposed and Cin == 128 and Cout == 3 and k == 5 and stride == 2 and mask is None and x.dtype == _h16() and weight.dtype == torch.float32:
                # g_s_conv4: the kernel's LDS weight panel is pre-packed once per weight update
                L.call("hesic_sconv2d_forward_prepacked", C.byref(d), L.ptr(x), L.ptr(w.contiguous()), L.ptr(_weight_image(1, weight)), L.ptr(bias),
                       L.ptr(y), L.stream())
            else:
                L.call("hesic_sconv2d_forward", C.byref(d), L.ptr(x), L.ptr(w.contiguous()), L.ptr(bias), L.ptr(y), L.stream())
        else:
            x = _nhwc(x)
            wp = packer.get(weight, mask, Cout, Cin, k, k, transposed, False, x.dtype)
            y = _wide_conv(x, wp, bias, B, H, W, Cin, Ho, Wo, Cout, k, stride, pad, transposed, act, in_abs, tap_mask)
        ctx.save_for_backward(x, weight, y if act else None)
        ctx.has_bias, ctx.bias, ctx.det = bias is not None, bias, _det_conv_grads
        return y

    @staticmethod
    def backward(ctx, gy):
        x, weight, y_act = ctx.saved_tensors
        k, stride, pad, transposed, act, in_abs, tap_mask, packer, mask = ctx.cfg
        B, H, W, Cin, Ho, Wo, Cout = ctx.dims
        if act:
            g2 = torch.empty_like(y_act)
            gyc = gy.to(y_act.dtype)
            gyc = _nhwc(gyc) if y_act.is_contiguous(memory_format=_CL) and y_act.dim() == 4 and not _is_narrow(Cout) else gyc.contiguous()
            L.call("hesic_act_backward", L.ptr(y_act), L.ptr(gyc), L.ptr(g2), y_act.numel(), act, L.dt(y_act), L.stream())
            gy = g2
        dx = dw = db = None
        if ctx.det:
            # order-fixed bias (and first-layer weight) gradients; the usual kernels compute what is left
            ddw, ddb, dw_done, db_done = _det_conv_param_grads(ctx, x, weight, _nhwc(gy) if gy.dim() == 4 and not _is_narrow(Cout) else gy)
            has_bias, need_dw = ctx.has_bias and not db_done, ctx.needs_input_grad[1] and not dw_done
            if ctx.narrow:
                dx, dw, db = _narrow_conv_grads(x, weight, gy, ctx.cfg, ctx.dims, has_bias, ctx.needs_input_grad[0], need_dw, ctx.bias, ydt=ctx.ydt)
            else:
                dx, dw, db = _wide_conv_grads(x, weight, gy, ctx.cfg, ctx.dims, has_bias, ctx.needs_input_grad[0], need_dw, ctx.bias)
            dw, db = (ddw if dw_done else dw), (ddb if db_done else db)
        elif ctx.narrow:
            dx, dw, db = _narrow_conv_grads(x, weight, gy, ctx.cfg, ctx.dims, ctx.has_bias, ctx.needs_input_grad[0], ctx.needs_input_grad[1], ctx.bias,
                                            ydt=ctx.ydt)
        else:
            dx, dw, db = _wide_conv_grads(x, weight, gy, ctx.cfg, ctx.dims, ctx.has_bias, ctx.needs_input_grad[0], ctx.needs_input_grad[1], ctx.bias)
        if not ctx.has_bias:
            db = None
        return dx, dw, db, None


import os as _os
FUSE_CONV_GDN = True      # module switch for profiling


class PackedGdn:
    """gamma' (bf16, LDS-image + MFMA-fragment copies) / beta' (fp32) for the fused conv+GDN epilogue; inference-only cache."""

    def __init__(self):
        self._hit = None
        self._train = None

    def get(self, beta, gamma, beta_min):
        tag = (beta.data_ptr(), gamma.data_ptr(), beta._version, gamma._version, _cache_epoch)
        if self._hit is not None and self._hit[0] == tag and not torch.is_grad_enabled():
            return self._hit[1], self._hit[2]
        # (grad mode is OFF inside an autograd.Function.forward -- where the fused conv + GDN stages call this: rounds 3-4 therefore re-packed 12
        # of the 15 GDNs one by one every step on top of the batched launch; the Trainer's step flag alone decides)
        if (_train_pack_cache and isinstance(beta, torch.nn.Parameter) and isinstance(gamma, torch.nn.Parameter)
                and gamma.dtype == torch.float32 and gamma.is_contiguous() and beta.is_contiguous()):
            # Trainer step: a persistent pack, refreshed with every other GDN's by ONE launch behind the optimiser update (repack_all) --
            # 15 pack launches a step otherwise
            t = self._train
            if t is not None and t["tag"] == tag and t["gp"].dtype == _h16() and t["gp"].device == gamma.device:
                return t["gp"], t["bp"]
            import weakref
            gp = torch.empty(2 * 128 * 128, dtype=_h16(), device=gamma.device)
            bp = torch.empty(128, dtype=torch.float32, device=gamma.device)
            L.call("hesic_gdn_pack_params", L.ptr(beta), L.ptr(gamma), float(beta_min), L.ptr(gp), L.ptr(bp), 128, L.stream())
            self._train = {"tag": tag, "gp": gp, "bp": bp, "beta": weakref.ref(beta), "gamma": weakref.ref(gamma), "beta_min": float(beta_min)}
            if self not in _gdn_registry:
                _gdn_registry.append(self)
            return gp, bp
        gp = torch.empty(2 * 128 * 128, dtype=_h16(), device=gamma.device)
        bp = torch.empty(128, dtype=torch.float32, device=gamma.device)
        L.call("hesic_gdn_pack_params", L.ptr(_c(beta)), L.ptr(_c(gamma)), float(beta_min), L.ptr(gp),
               L.ptr(bp), 128, L.stream())
        self._hit = (tag, gp, bp)
        return gp, bp


FUSE_CONV_GDN_TRAIN = True      # module switch for profiling


def conv2d_gdn_fusable(x, weight, gdn_channels, transposed):
    """The fused epilogue exists for bf16 storage, 128 output channels and a wide input; with autograd on, the wide
    stages keep the fusion through ``_ConvGdnFn`` (the kernel then also stores the conv output for GDN's backward), the
    same goes for the image-side 3 -> 128 stage (``_SConvGdnFn``)."""
    cout = weight.shape[1] if transposed else weight.shape[0]
    cin = weight.shape[0] if transposed else weight.shape[1]
    if not x.is_cuda or cout != 128 or gdn_channels != 128 or not FUSE_CONV_GDN:
        return False
    if cin == 3:      # g_a_conv1 + g_a_gdn1: image in (any float dtype), bf16 storage out
        if torch.is_grad_enabled() and not FUSE_CONV_GDN_TRAIN:
            return False
        return (not transposed and _is16() and weight.shape[-1] == 5
                and x.dtype in (torch.float32, _h16()))
    if torch.is_grad_enabled() and not FUSE_CONV_GDN_TRAIN:
        return False
    return x.dtype == _h16() and cin % 32 == 0


def _gdn_backward(v, gy, beta, gamma, inverse, beta_min):
    """GDN.backward on (input v, dy): returns (dv, dbeta, dgamma); with flat gradient slots the parameter gradients are
    added in place and come back as None."""
    B, Cc, H, W = v.shape
    P = B * H * W
    gv = torch.empty_like(v, memory_format=_CL)
    sb, sg = _slot_for(beta), _slot_for(gamma)
    direct = sb is not None and sg is not None
    dbeta = sb.grad if direct else torch.empty_like(beta, dtype=torch.float32)
    dgamma = sg.grad if direct else torch.empty_like(gamma, dtype=torch.float32)
    ws = torch.empty(max(1, L.lib().hesic_gdn_backward_ws_bytes(P, Cc)), dtype=torch.uint8, device=v.device)
    if (direct and _finish_queue is not None and GDN_FINISH_BATCH and beta.is_contiguous() and gamma.is_contiguous()
            and L.lib().hesic_gdn_backward_partial_ok(P, Cc, L.dt(v))):
        # Trainer step: dx now, the parameter-gradient finish with the other GDNs' in one launch (flush_gdn_finish); a module used twice in a
        # step (encoder1) must not have two jobs in one launch
        if any(j.slot_gamma is sg for j in _gdn_finish_queue) or len(_gdn_finish_queue) >= 16:
            flush_gdn_finish()
        L.call("hesic_gdn_backward_partial", L.ptr(v), L.ptr(gy), L.ptr(beta), L.ptr(gamma), L.ptr(gv), L.ptr(ws), P, Cc, int(inverse),
               float(beta_min), L.dt(v), L.stream())
        _gdn_finish_queue.append(_GdnJob(ws, P, beta, gamma, sb, sg, float(beta_min)))
        return gv, None, None
    L.call("hesic_gdn_backward_acc", L.ptr(v), L.ptr(gy), L.ptr(_c(beta)), L.ptr(_c(gamma)), L.ptr(gv), L.ptr(dbeta),
           L.ptr(dgamma), int(direct), L.ptr(ws), P, Cc, int(inverse), float(beta_min), L.dt(v), L.stream())
    if direct:
        _slot_done(sb)
        _slot_done(sg)
        return gv, None, None
    return gv, dbeta, dgamma


def _n2w_image(weight, beta, gamma, gp, x):
    """LDS image of g_a_conv1's weights + the K-permuted gamma' for the fused 3 -> 128 kernel's fast form (fp32 planar image,
    5x5 stride 2); None -> the kernel gathers in its prologue (other layouts)."""
    if tuple(weight.shape) != (128, 3, 5, 5) or weight.dtype != torch.float32 or x.dtype != torch.float32:
        return None
    return _weight_image(0, weight, gp, (gamma.data_ptr(), gamma._version, beta._version, gp.data_ptr()))


class _SConvGdnFn(torch.autograd.Function):
    """g_a_gdn1(g_a_conv1(image)) fused under autograd (the 3 -> 128 stage): v = conv output is stored next to y."""

    @staticmethod
    def forward(ctx, x, weight, bias, beta, gamma, cfg):
        k, stride, pad, inverse, beta_min, gdn_packer = cfg
        B, Cin, H, W = x.shape
        Cout = weight.shape[0]
        Ho, Wo = _out_hw(H, W, k, stride, pad, False)
        gp, bp = gdn_packer.get(beta, gamma, beta_min)
        y = _empty_nhwc(B, Cout, Ho, Wo, _h16(), x.device)
        v = _empty_nhwc(B, Cout, Ho, Wo, _h16(), x.device)
        d = _sdesc(x, y, Cin, Cout, k, stride, pad, False)
        L.call("hesic_sconv2d_gdn_forward_prepacked", C.byref(d), L.ptr(x), L.ptr(_c(weight)),
               L.ptr(_n2w_image(weight, beta, gamma, gp, x)), L.ptr(bias), L.ptr(gp), L.ptr(bp), int(inverse), L.ptr(y), L.ptr(v), L.stream())
        ctx.save_for_backward(x, weight, v, beta, gamma)
        ctx.cfg, ctx.dims, ctx.has_bias, ctx.bias = cfg, (B, H, W, Cin, Ho, Wo, Cout), bias is not None, bias
        return y

    @staticmethod
    def backward(ctx, gy):
        x, weight, v, beta, gamma = ctx.saved_tensors
        k, stride, pad, inverse, beta_min, _ = ctx.cfg
        gv, dbeta, dgamma = _gdn_backward(v, _nhwc(gy.to(v.dtype)), beta, gamma, inverse, beta_min)
        ccfg = (k, stride, pad, False, 0, 0, 0, None, None)
        dx, dw, db = _narrow_conv_grads(x, weight, gv, ccfg, ctx.dims, ctx.has_bias, ctx.needs_input_grad[0], ctx.needs_input_grad[1], ctx.bias)
        return dx, dw, (db if ctx.has_bias else None), dbeta, dgamma, None


class _ConvGdnFn(torch.autograd.Function):
    """(I)GDN(conv(x)) with the fused forward kernel kept under autograd: the kernel stores the conv output v next to y,
    the backward is GDN's backward on (v, gy) followed by the conv's data / weight gradients."""

    @staticmethod
    def forward(ctx, x, weight, bias, beta, gamma, cfg):
        k, stride, pad, transposed, inverse, beta_min, packer, gdn_packer = cfg
        Cin, Cout = (weight.shape[0], weight.shape[1]) if transposed else (weight.shape[1], weight.shape[0])
        B, _, H, W = x.shape
        Ho, Wo = _out_hw(H, W, k, stride, pad, transposed)
        x = _nhwc(x)
        wp = packer.get(weight, None, Cout, Cin, k, k, transposed, False, x.dtype)
        gp, bp = gdn_packer.get(beta, gamma, beta_min)
        y = _empty_nhwc(B, Cout, Ho, Wo, x.dtype, x.device)
        v = _empty_nhwc(B, Cout, Ho, Wo, x.dtype, x.device)
        d = L.ConvDesc(B, H, W, Cin, Ho, Wo, Cout, k, k, stride, pad, int(transposed), L.dt(x), 0, 0, Cin, 0, Cout, 0, 0)
        L.call("hesic_conv2d_gdn_forward_train", C.byref(d), L.ptr(x), L.ptr(wp), L.ptr(bias), L.ptr(gp), L.ptr(bp), int(inverse),
               L.ptr(y), L.ptr(v), L.stream())
        ctx.save_for_backward(x, weight, v, beta, gamma)
        ctx.cfg, ctx.dims, ctx.has_bias, ctx.bias = cfg, (B, H, W, Cin, Ho, Wo, Cout), bias is not None, bias
        return y

    @staticmethod
    def backward(ctx, gy):
        x, weight, v, beta, gamma = ctx.saved_tensors
        k, stride, pad, transposed, inverse, beta_min, packer, _ = ctx.cfg
        gv, dbeta, dgamma = _gdn_backward(v, _nhwc(gy.to(v.dtype)), beta, gamma, inverse, beta_min)
        ccfg = (k, stride, pad, transposed, 0, 0, 0, packer, None)
        dx, dw, db = _wide_conv_grads(x, weight, gv, ccfg, ctx.dims, ctx.has_bias, ctx.needs_input_grad[0], ctx.needs_input_grad[1], ctx.bias)
        return dx, dw, (db if ctx.has_bias else None), dbeta, dgamma, None


def conv2d_gdn(x, weight, bias, beta, gamma, *, kernel_size, stride, padding, transposed, inverse, beta_min, packer, gdn_packer):
    """(I)GDN(conv(x)) in ONE kernel (inference only; training keeps the two autograd ops)."""
    L.require_cuda(x, weight)
    k = kernel_size
    Cin, Cout = (weight.shape[0], weight.shape[1]) if transposed else (weight.shape[1], weight.shape[0])
    B, _, H, W = x.shape
    Ho, Wo = _out_hw(H, W, k, stride, padding, transposed)
    if Cin == 3 and torch.is_grad_enabled():
        return _apply(_SConvGdnFn, x, weight, bias, beta, gamma, (k, stride, padding, inverse, beta_min, gdn_packer))
    if Cin == 3:      # image-side stage: strided fp32/bf16 image in, bf16 NHWC out
        gp, bp = gdn_packer.get(beta, gamma, beta_min)
        out = _empty_nhwc(B, Cout, Ho, Wo, _h16(), x.device)
        d = _sdesc(x, out, Cin, Cout, k, stride, padding, False)
        L.call("hesic_sconv2d_gdn_forward_prepacked", C.byref(d), L.ptr(x), L.ptr(_c(weight)),
               L.ptr(_n2w_image(weight, beta, gamma, gp, x)), L.ptr(bias), L.ptr(gp), L.ptr(bp), int(inverse), L.ptr(out), None, L.stream())
        return out
    if torch.is_grad_enabled():
        return _apply(_ConvGdnFn, x, weight, bias, beta, gamma, (k, stride, padding, transposed, inverse, beta_min, packer, gdn_packer))
    x = _nhwc(x)
    wp = packer.get(weight, None, Cout, Cin, k, k, transposed, False, x.dtype)
    gp, bp = gdn_packer.get(beta, gamma, beta_min)
    out = _empty_nhwc(B, Cout, Ho, Wo, x.dtype, x.device)
    d = L.ConvDesc(B, H, W, Cin, Ho, Wo, Cout, k, k, stride, padding, int(transposed), L.dt(x), 0, 0, Cin, 0, Cout, 0, 0)
    L.call("hesic_conv2d_gdn_forward", C.byref(d), L.ptr(x), L.ptr(wp), L.ptr(bias), L.ptr(gp), L.ptr(bp), int(inverse),
           L.ptr(out), L.stream())
    return out


def conv2d(x, weight, bias, *, kernel_size, stride, padding, transposed=False, act=L.ACT_NONE, in_abs=False,
           tap_mask=0, packer=None, mask=None):
    packer = packer if packer is not None else PackedWeight()
    return _apply(_ConvFn, x, weight, bias, (kernel_size, stride, padding, transposed, act, int(in_abs), tap_mask, packer, mask))


FP32_LATENTS = _os.environ.get("HESIC_BF16_LATENTS") is None      # A/B switch: set to store latents / sigma / mu as bf16 again


def fp32_latents():
    """True when the inference forward keeps what feeds round() and the likelihoods in fp32 although the feature maps are
    bf16: the latents y, z and the sigma / mu maps are written from the convs' fp32 accumulators (round 1 stored them as
    bf16: one ulp = 1/16 at |y| ~ 10, so latents near .5 flipped and bpp / PSNR sat just outside the 1e-3 target)."""
    return FP32_LATENTS and _is16() and not torch.is_grad_enabled()


def conv2d_latent(x, weight, bias, *, kernel_size, stride, padding, transposed=False, act=L.ACT_NONE, in_abs=False,
                  tap_mask=0, packer=None, mask=None, want_lo=True):
    """A conv whose output feeds an entropy model: returns ``(lo, hi)`` -- ``lo`` in the storage dtype for the next conv
    (None unless ``want_lo``), ``hi`` for round() / the likelihood.  bf16 inference: ``hi`` is fp32 straight from the
    accumulators; otherwise both are the ordinary output."""
    k = kernel_size
    Cin, Cout = (weight.shape[0], weight.shape[1]) if transposed else (weight.shape[1], weight.shape[0])
    ok = (fp32_latents() and x.is_cuda and x.dtype == _h16() and not _is_narrow(Cin) and not _is_narrow(Cout)
          and Cin % 32 == 0 and Cout % 8 == 0)
    if not ok:
        y = conv2d(x, weight, bias, kernel_size=k, stride=stride, padding=padding, transposed=transposed, act=act, in_abs=in_abs,
                   tap_mask=tap_mask, packer=packer, mask=mask)
        return (y if want_lo else None), y
    L.require_cuda(x, weight)
    packer = packer if packer is not None else PackedWeight()
    B, _, H, W = x.shape
    Ho, Wo = _out_hw(H, W, k, stride, padding, transposed)
    x = _nhwc(x)
    wp = packer.get(weight, mask, Cout, Cin, k, k, transposed, False, x.dtype)
    return _wide_conv(x, wp, bias, B, H, W, Cin, Ho, Wo, Cout, k, stride, padding, transposed, act, int(in_abs), tap_mask,
                      f32_out="both" if want_lo else "only")


# ------------------------------------------------------------------------------ bf16x3 ("hi/lo") analysis path
# The reference computes g_a in fp32 and round()s its output; single-bf16 operands move y by ~3e-3 relative and flip ~1 % of
# the latents.  In the "bf16x3" analysis mode every value on the way to y is a PAIR of bf16 (hi = bf16(v), lo = bf16(v - hi)):
# activations [hi(C) | lo(C)] per pixel, weights [w_hi | w_lo] along Cin, three MFMA products per staged operand pair
# (x_hi w_hi + x_lo w_hi + x_hi w_lo; x_lo w_lo, 2^-18, is dropped) -- bf16 arithmetic on the matrix cores at ~2^-17 relative per operand.  Inference only.
# Modes (16-bit inference; the 16-bit format itself -- bfloat16 or float16 -- is the compute dtype):
#   "x3"    every analysis layer and the hyper-analysis on pairs, three products per MAC;
#   "x3c2"  as "x3", but g_a_conv2 (128 -> 128 5x5 s2 on the largest map: 70 % of g_a's MACs) multiplies SINGLE operands -- one product per
#           MAC; its input leaves the conv1 + GDN kernel as one 16-bit value per channel, its GDN epilogue runs on pairs and hands pairs on.
#           Meant for float16 (11-bit significand: ~6e-4 of the latents flip against the fp32 reference; with bfloat16 it is ~5e-3);
#   "x2"    pairs everywhere, TWO products per MAC: x pairs x single error-feedback weights (no w_lo term; round 5, measured and not the default);
#   "x1"    single operands everywhere (round 2's path; float16: ~1.3e-3 flips, bfloat16: ~1e-2).
# "bf16x3" / "bf16" are the round-3 names of "x3" / "x1".
ANALYSIS_MODES = ("x1", "x3", "x3c2", "x2")
_ANALYSIS_ALIASES = {"bf16": "x1", "bf16x3": "x3"}


def _canon_analysis(mode):
    mode = _ANALYSIS_ALIASES.get(mode, mode)
    if mode != "auto" and mode not in ANALYSIS_MODES:
        raise ValueError(f"analysis precision must be 'auto' or one of {ANALYSIS_MODES} (or {tuple(_ANALYSIS_ALIASES)})")
    return mode


_analysis_mode = _canon_analysis(_os.environ.get("HESIC_ANALYSIS", "auto"))


def set_analysis_precision(mode):
    """Operand precision of the analysis transforms + hyper-analysis of a 16-bit inference forward: "x3", "x3c2", "x2", "x1" (see above) or
    "auto" (the default) = "x3" for both 16-bit formats.  Round 4's default for float16 maps was "x3c2" (1.25x the speed of "x3"); round 5
    measured it at TRAINED operating points (piecewise-smooth pairs, 30 - 33 dB, ``profiles/scripts/parity_smooth.py``): 2.6 - 8e-4 of the
    latents flip there and every flip moves the reconstruction -- |dPSNR| 2 - 6e-3 dB, outside north_star's 1e-3 -- where "x3" stays at
    <= 5e-6 flips / 1.6 - 3.6e-4 dB.  "x3c2" (and "x2" = pairs x single error-feedback weights, 1.5 - 2.1e-4 flips, 1.3 - 1.5e-3 dB) stay
    available as explicit fast modes.  Returns the previous setting."""
    global _analysis_mode
    prev, _analysis_mode = _analysis_mode, _canon_analysis(mode)
    return prev


def analysis_precision():
    """The mode in effect for the current compute dtype ("auto" resolved)."""
    if _analysis_mode == "auto":
        return "x3"
    return _analysis_mode


def analysis_hilo(x):
    """True when the analysis stack should take the hi/lo route for input ``x``: 16-bit inference on the GPU."""
    return (analysis_precision() != "x1" and _is16() and not torch.is_grad_enabled() and x.is_cuda)


def analysis_conv2_single():
    """True in the "x3c2" mode: g_a_conv2 on single operands between the pair layers."""
    return analysis_precision() == "x3c2"


PAIR_WEIGHT_SCALING = True      # part of the pair arithmetic since round 5 (no run-time switch: it changes the last bit of y)


def _pair_weight_shift(w):
    """Power-of-two exponent s for packing a weight as the pair (w 2^s)_hi | (w 2^s)_lo.  binary16 only: the lo half of an unscaled weight of
    0.02 is 5e-6 -- a SUBNORMAL half (step 6e-8), so the pair carries 2^-20 instead of 2^-22 and a 128 -> 128 5x5 layer's output is
    ~1e-6 relative off, the largest single term of the pair mode's flipped latents (profiles/scripts/gdn_pair_precision.py).  With the
    largest |w| brought to [2^13, 2^14) every weight down to 2^-17 of it keeps a normal lo half; the kernel multiplies its accumulators by
    2^-s once (exact).  bfloat16 has fp32's range: s = 0.  One device -> host sync per repack (inference packs are cached)."""
    if not PAIR_WEIGHT_SCALING or _h16() != torch.float16 or not w.is_cuda:
        return 0
    m = float(w.abs().max())
    if not (m > 0.0) or m != m or m == float("inf"):
        return 0
    import math
    return max(0, min(24, 13 - math.frexp(m)[1] + 1))


class PackedWeightHiLo:
    """[w_hi | w_lo] (bf16, the kernels' [tap][Cout][2 Cin] layout) of a conv weight; inference cache keyed like ``PackedWeight``.
    ``as_1x1``: flatten (Cout, Cin, k, k) to a 1x1 weight over the im2col columns, zero-padded to ``kp`` columns."""

    def __init__(self):
        self._hit = None

    def get(self, weight, as_1x1=False, kp=0, single=False):
        """``single``: the rows of the two-product form (``hesic_conv2d_forward_hilo_w1``): [w rounded with error feedback over the taps | 0]."""
        tag = (weight.data_ptr(), weight._version, _cache_epoch, as_1x1, kp, single)
        if self._hit is not None and self._hit[0] == tag:
            return self._hit[1]
        if single:
            cout, cin, kh, kw = weight.shape
            tmp = torch.empty(kh * kw * cout * cin, dtype=_h16(), device=weight.device)
            L.call("hesic_pack_conv_weight_shaped", L.ptr(_c(weight.detach())), L.ptr(tmp), cout, cin, kh, kw, L.stream())
            wp = torch.empty((kh * kw, cout, 2, cin), dtype=_h16(), device=weight.device).fill_(0)
            wp[:, :, 0] = tmp.view(kh * kw, cout, cin)
            wp = wp.reshape(-1)
            self._hit = (tag, wp)
            return wp
        w = weight.detach().float()
        if as_1x1:
            cout = w.shape[0]
            flat = w.reshape(cout, -1)
            w = torch.cat([flat, flat.new_zeros(cout, kp - flat.shape[1])], 1).reshape(cout, kp, 1, 1)
        sh = _pair_weight_shift(w)
        if sh:
            w = w * float(2 ** sh)
        hi = w.to(_h16()).float()
        lo = (w - hi).to(_h16()).float()
        w2 = torch.cat([hi, lo], 1).contiguous()
        cout, cin2, kh, kw = w2.shape
        wp = torch.empty(kh * kw * cout * cin2, dtype=_h16(), device=w2.device)
        L.call("hesic_pack_conv_weight", L.ptr(w2), None, L.ptr(wp), cout, cin2, kh, kw, 0, 0, L.H16, L.stream())
        wp.hesic_acc_scale = float(2.0 ** -sh)          # conv2d_hilo hands it to the launch (hesic_conv2d_hilo_set_acc_scale)
        self._hit = (tag, wp)
        return wp


class PackedGdnLo:
    """Fragment-order lo half of gamma' for the hi/lo GDN epilogue (``hesic_gdn_pack_params_lo``); inference cache."""

    def __init__(self):
        self._hit = None

    def get(self, gamma):
        tag = (gamma.data_ptr(), gamma._version, _cache_epoch)
        if self._hit is not None and self._hit[0] == tag:
            return self._hit[1]
        glo = torch.empty(128 * 128, dtype=_h16(), device=gamma.device)
        L.call("hesic_gdn_pack_params_lo", L.ptr(_c(gamma)), L.ptr(glo), 128, L.stream())
        self._hit = (tag, glo)
        return glo


class PackedN2wHiLo:
    """LDS images [w_hi | w_lo | gamma'_hi | gamma'_lo] (128 KB) of the fused hi/lo g_a_conv1 + GDN kernel; inference cache."""

    def __init__(self):
        self._hit = {}

    def get(self, weight, gamma, out1=False, inverse=False):
        """``out1``: the image of the kernel's single-output form (w rounded with error feedback over the taps, lo halves unused).
        ``inverse``: the image for an IGDN launch -- never scaled: GDN's quotient is invariant under the binary16 weight scaling, IGDN's
        product v sqrt(n) is not (it would come out times 4^s)."""
        tag = (weight.data_ptr(), weight._version, gamma.data_ptr(), gamma._version, _cache_epoch)
        inverse = bool(inverse) and not out1
        hit = self._hit.get((out1, inverse))
        if hit is not None and hit[0] == tag:
            return hit[1]
        img = torch.empty(128 * 1024, dtype=torch.uint8, device=weight.device)
        sh = 0 if (out1 or inverse) else _pair_weight_shift(weight.detach().float())
        if sh:
            # pair form, binary16: weights times 2^s in the image (normal lo halves); sconv_gdn_hilo then passes bias 2^s and beta' 4^s
            L.call("hesic_sconv_pack_weight_image_hilo_scaled", L.ptr(_c(weight)), L.ptr(_c(gamma)), float(2 ** sh), L.ptr(img), L.stream())
        else:
            L.call("hesic_sconv_pack_weight_image_hilo_out1" if out1 else "hesic_sconv_pack_weight_image_hilo", L.ptr(_c(weight)), L.ptr(_c(gamma)),
                   L.ptr(img), L.stream())
        img.hesic_wscale = float(2 ** sh)
        img.hesic_scaled = {}                              # (tensor address, version) -> the scaled copy of bias / beta'
        self._hit[(out1, inverse)] = (tag, img)
        return img


def sconv_gdn_hilo_ok(x, weight):
    """The fused hi/lo 3 -> 128 kernel takes an fp32 image with unit pixel stride and an even width."""
    return (x.dtype == torch.float32 and x.dim() == 4 and x.stride(3) == 1 and x.shape[3] % 2 == 0 and tuple(weight.shape) == (128, 3, 5, 5)
            and weight.dtype == torch.float32 and min(x.stride()) >= 0)


def sconv_gdn_hilo(x, image, bias, beta_packed, inverse, out1=False):
    """GDN(conv(x)) of the 3 -> 128 5x5 stride-2 stage on hi/lo pairs in one kernel: (B, 256, H/2, W/2) [hi | lo] 16-bit NHWC;
    ``out1``: the same arithmetic, but the output is ONE 16-bit value per channel, (B, 128, H/2, W/2)."""
    L.require_cuda(x)
    wsc = getattr(image, "hesic_wscale", 1.0)
    if wsc != 1.0 and inverse:
        raise ValueError("sconv_gdn_hilo: an IGDN launch needs the unscaled weight image (PackedN2wHiLo.get(..., inverse=True))")
    if wsc != 1.0:
        def scaled(t, f):
            if t is None:
                return None
            key = (t.data_ptr(), t._version, f)
            hit = image.hesic_scaled.get(key)
            if hit is None:
                if len(image.hesic_scaled) > 8:
                    image.hesic_scaled.clear()
                hit = image.hesic_scaled[key] = (t.detach().float() * f).contiguous()
            return hit
        bias, beta_packed = scaled(bias, wsc), scaled(beta_packed, wsc * wsc)
    B, Cc, H, W = x.shape
    Ho, Wo = _out_hw(H, W, 5, 2, 2, False)
    y = _empty_nhwc(B, 128 if out1 else 256, Ho, Wo, _h16(), x.device)
    d = _sdesc(x, y, 3, 128, 5, 2, 2, False)
    L.call("hesic_sconv2d_gdn_forward_hilo_out1" if out1 else "hesic_sconv2d_gdn_forward_hilo", C.byref(d), L.ptr(x), L.ptr(image), L.ptr(bias),
           L.ptr(beta_packed), int(inverse), L.ptr(y), L.stream())
    return y


def conv2d_gdn_hilo_out(x, wp, bias, cin, *, kernel_size, stride, padding, gdn):
    """(I)GDN(conv(x)) with SINGLE 16-bit operands in the conv (one product per MAC), the GDN on pairs from the fp32 accumulators and a
    hi/lo output map (B, 256, Ho, Wo) -- ``hesic_conv2d_gdn_forward_hilo_out``; ``gdn`` = (gamma_packed, gamma_lo_packed, beta_packed, inverse)."""
    L.require_cuda(x)
    k = kernel_size
    B, cx, H, W = x.shape
    Ho, Wo = _out_hw(H, W, k, stride, padding, False)
    x = _nhwc(x)
    gp, glo, bp, inverse = gdn
    y = _empty_nhwc(B, 256, Ho, Wo, _h16(), x.device)
    d = L.ConvDesc(B, H, W, cin, Ho, Wo, 128, k, k, stride, padding, 0, L.H16, 0, 0, cx, 0, 256, 0, 0)
    L.call("hesic_conv2d_gdn_forward_hilo_out", C.byref(d), L.ptr(x), L.ptr(wp), L.ptr(bias), L.ptr(gp), L.ptr(glo), L.ptr(bp), int(inverse),
           L.ptr(y), L.stream())
    return y


def im2col_hilo(x, k, stride, padding, kp):
    """Column matrix of a few-channel fp32 image as hi/lo bf16: (B, 2*kp, Ho, Wo) NHWC (``hesic_im2col_hilo``)."""
    L.require_cuda(x)
    if x.dtype != torch.float32:
        x = x.float()
    B, Cc, H, W = x.shape
    Ho, Wo = _out_hw(H, W, k, stride, padding, False)
    cols = _empty_nhwc(B, 2 * kp, Ho, Wo, _h16(), x.device)
    st = (C.c_int64 * 4)(*x.stride())
    L.call("hesic_im2col_hilo", L.ptr(x), st, B, Cc, H, W, k, k, stride, padding, Ho, Wo, kp, L.ptr(cols), L.stream())
    return cols


class HiLo(tuple):
    """A feature map stored as [hi(C) | lo(C)] bf16 pairs per pixel: ``HiLo((tensor (B, 2C, H, W) NHWC bf16, C))``.  A tuple, so the
    stream bookkeeping of the inference schedule (``models._tensors``) sees the tensor inside."""
    __slots__ = ()
    t = property(lambda self: self[0])
    c = property(lambda self: self[1])


def conv2d_hilo(x_hilo, wp3, bias, cin, cout, *, kernel_size, stride, padding, gdn=None, act=L.ACT_NONE, out="f32", out_abs=False, products=3):
    """Implicit GEMM on hi/lo operands (``hesic_conv2d_forward_hilo``).  ``gdn`` = (gamma_packed, gamma_lo_packed, beta_packed,
    inverse): fused hi/lo (I)GDN, returns the (B, 2*cout, Ho, Wo) hi/lo map.  Otherwise ``out``: "f32" -> act(conv + bias) as fp32
    (B, cout, Ho, Wo); "hilo" -> the hi/lo map (of |.| with ``out_abs``); "both" -> (hilo, f32)."""
    L.require_cuda(x_hilo)
    k = kernel_size
    B, c2, H, W = x_hilo.shape
    Ho, Wo = _out_hw(H, W, k, stride, padding, False)
    x_hilo = _nhwc(x_hilo)
    entry = "hesic_conv2d_forward_hilo_w1" if products == 2 else "hesic_conv2d_forward_hilo"      # ``products`` = 2: ``wp3`` from PackedWeightHiLo.get(single=True)
    acc_scale = getattr(wp3, "hesic_acc_scale", 1.0)            # weights packed times 2^s (PackedWeightHiLo): the launch unscales its sums
    if gdn is not None:
        gp, glo, bp, inverse = gdn
        y = _empty_nhwc(B, 2 * cout, Ho, Wo, _h16(), x_hilo.device)
        d = L.ConvDesc(B, H, W, cin, Ho, Wo, cout, k, k, stride, padding, 0, L.H16, 0, 0, c2, 0, 2 * cout, 0, 0)
        if acc_scale != 1.0:
            L.call("hesic_conv2d_hilo_set_acc_scale", acc_scale)
        L.call(entry, C.byref(d), L.ptr(x_hilo), L.ptr(wp3), L.ptr(bias), L.ptr(gp), L.ptr(glo), L.ptr(bp), int(inverse),
               L.ptr(y), 0, None, 0, 0, None, 0, L.stream())
        return y
    y = _empty_nhwc(B, 2 * cout, Ho, Wo, _h16(), x_hilo.device) if out in ("hilo", "both") else None
    y32 = _empty_nhwc(B, cout, Ho, Wo, torch.float32, x_hilo.device) if out in ("f32", "both") else None
    d = L.ConvDesc(B, H, W, cin, Ho, Wo, cout, k, k, stride, padding, 0, L.H16, act, 0, c2, 0, 2 * cout if y is not None else cout, 0, 0)
    key = ("hilo", B, H, W, cin, cout, k, stride, padding)
    need = _ws_bytes.get(key)
    if need is None:
        need = _ws_bytes[key] = int(L.lib().hesic_conv2d_hilo_ws_bytes(C.byref(d)))
    ws = torch.empty(need, dtype=torch.uint8, device=x_hilo.device) if (need and SPLIT_K) else None
    if acc_scale != 1.0:
        L.call("hesic_conv2d_hilo_set_acc_scale", acc_scale)
    L.call(entry, C.byref(d), L.ptr(x_hilo), L.ptr(wp3), L.ptr(bias), None, None, None, 0, L.ptr(y), int(out_abs),
           L.ptr(y32), cout, 0, L.ptr(ws), need if ws is not None else 0, L.stream())
    return (y, y32) if out == "both" else (y if out == "hilo" else y32)


class PackedGroup:
    """Packed bf16 weights (+ concatenated fp32 bias) of several same-geometry convs side by side along Cout, for
    ``conv2d_grouped``; inference cache with the tag policy of ``PackedWeight``."""

    def __init__(self):
        self._hit = None

    def get(self, weights, biases, k, transposed):
        """Returns (packed weights, bias, per-branch cout offsets, padded total): every branch starts on a multiple of 128 couts (the
        cout tile of the kernel; pad rows are zero weights / zero bias -- 960 -> 1024 for the mixture-parameter layers)."""
        tag = tuple((w.data_ptr(), w._version) for w in weights) + tuple((b.data_ptr(), b._version) for b in biases if b is not None) + (_cache_epoch,)
        if self._hit is not None and self._hit[0] == tag:
            return self._hit[1:]
        couts = [(w.shape[1] if transposed else w.shape[0]) for w in weights]
        cin = weights[0].shape[0] if transposed else weights[0].shape[1]
        offs, total = [], 0
        for co in couts:
            offs.append(total)
            total += -(-co // 128) * 128
        dev = weights[0].device
        wp = torch.empty(k * k * total * cin, dtype=_h16(), device=dev).fill_(0)
        bias = torch.empty(total, dtype=torch.float32, device=dev).fill_(0)
        for w, b, co, off in zip(weights, biases, couts, offs):
            L.call("hesic_pack_conv_weight_slice", L.ptr(w.detach().contiguous()), L.ptr(wp), co, cin, k, k, int(transposed), total, off, L.stream())
            if b is not None:
                bias[off:off + co].copy_(b.detach())
        self._hit = (tag, wp, bias, offs, total)
        return wp, bias, offs, total


def grouped_ok(x):
    """The grouped hyper-synthesis launches exist for bf16 inference."""
    return GROUP_HYPER and not torch.is_grad_enabled() and x.is_cuda and x.dtype == _h16()


GROUP_HYPER = _os.environ.get("HESIC_NO_GROUP_HYPER") is None      # A/B switch


def conv2d_grouped(x, weights, biases, packer, *, kernel_size, stride, padding, transposed=False, shared_input=True, x_c_off=0,
                   x_group_step=None, acts=None, f32_out=None):
    """Several convs of one geometry as ONE implicit-GEMM launch (``hesic_conv2d_forward_grouped``): ``weights`` / ``biases`` are the
    branches' tensors; with ``shared_input`` every branch reads channels [x_c_off, x_c_off + Cin) of ``x``, otherwise branch g reads
    [x_c_off + g * x_group_step, ...) (default step: Cin).  ``acts``: one activation per branch (at most two distinct values,
    switching once).  Returns ``(out, offsets)``: the concatenated output (B, padded sum of Cout, Ho, Wo) -- bf16, or with
    ``f32_out="only"`` fp32 from the accumulators -- and each branch's first channel in it (branches start on multiples of 128)."""
    L.require_cuda(x, *weights)
    k = kernel_size
    couts = [(w.shape[1] if transposed else w.shape[0]) for w in weights]
    cin = weights[0].shape[0] if transposed else weights[0].shape[1]
    G = len(weights)
    if not shared_input and len(set(couts)) != 1:
        raise ValueError("conv2d_grouped: branches with their own input slices need equal Cout")
    wp, bias, offs, total = packer.get(weights, biases, k, transposed)
    acts = list(acts) if acts is not None else [L.ACT_NONE] * G
    act, act2, split = acts[0], acts[0], 0
    for g in range(1, G):
        if acts[g] != acts[g - 1]:
            if split:
                raise ValueError("conv2d_grouped: the activation may switch once along the branches")
            act2, split = acts[g], offs[g]
    B, _, H, W = x.shape
    Ho, Wo = _out_hw(H, W, k, stride, padding, transposed)
    x = _nhwc(x)
    out = None if f32_out == "only" else _empty_nhwc(B, total, Ho, Wo, _h16(), x.device)
    out32 = _empty_nhwc(B, total, Ho, Wo, torch.float32, x.device) if f32_out else None
    groups = 1 if shared_input else G
    step = 0 if shared_input else (cin if x_group_step is None else int(x_group_step))
    d = L.ConvDesc(B, H, W, cin, Ho, Wo, total, k, k, stride, padding, int(transposed), L.H16, act, 0, x.shape[1], x_c_off, total, 0, 0)
    L.call("hesic_conv2d_forward_grouped", C.byref(d), groups, step, act2, split, L.ptr(x), L.ptr(wp), L.ptr(bias),
           L.ptr(out), L.ptr(out32), total, 0, L.stream())
    return (out32 if f32_out == "only" else (out if not f32_out else (out, out32))), offs


def conv2d_slice(x, x_c_off, weight, bias, *, kernel_size, stride, padding, transposed=False, act=L.ACT_NONE, packer=None):
    """Inference conv on the channel slice [x_c_off, x_c_off + Cin) of a wider NHWC tensor, read in place (no slice copy)."""
    L.require_cuda(x, weight)
    if torch.is_grad_enabled() and (x.requires_grad or weight.requires_grad):
        raise RuntimeError("conv2d_slice is an inference form")
    k = kernel_size
    Cin, Cout = (weight.shape[0], weight.shape[1]) if transposed else (weight.shape[1], weight.shape[0])
    B, _, H, W = x.shape
    Ho, Wo = _out_hw(H, W, k, stride, padding, transposed)
    x = _nhwc(x)
    packer = packer if packer is not None else PackedWeight()
    wp = packer.get(weight, None, Cout, Cin, k, k, transposed, False, x.dtype)
    return _wide_conv(x, wp, bias, B, H, W, Cin, Ho, Wo, Cout, k, stride, padding, transposed, act, 0, 0, x_c_off=x_c_off)


def conv2d_into(x, weight, bias, out, out_c_off, *, kernel_size, stride, padding, transposed=False, act=L.ACT_NONE, packer=None,
                mask=None, tap_mask=0):
    """Inference conv whose output lands in channels [out_c_off, out_c_off + Cout) of the wider NHWC tensor ``out`` (the kernels
    write a channel slice in place): what a ``torch.cat`` of conv outputs would otherwise copy together."""
    L.require_cuda(x, weight, out)
    if torch.is_grad_enabled() and (x.requires_grad or weight.requires_grad):
        raise RuntimeError("conv2d_into is an inference form")
    k = kernel_size
    Cin, Cout = (weight.shape[0], weight.shape[1]) if transposed else (weight.shape[1], weight.shape[0])
    B, _, H, W = x.shape
    Ho, Wo = _out_hw(H, W, k, stride, padding, transposed)
    if out.shape[0] != B or tuple(out.shape[2:]) != (Ho, Wo) or out_c_off + Cout > out.shape[1] or not out.is_contiguous(memory_format=_CL) \
            or out.dtype != x.dtype:
        raise ValueError("conv2d_into: `out` must be an NHWC tensor of the conv's dtype and output size with room for the channel slice")
    x = _nhwc(x)
    packer = packer if packer is not None else PackedWeight()
    wp = packer.get(weight, mask, Cout, Cin, k, k, transposed, False, x.dtype)
    _wide_conv(x, wp, bias, B, H, W, Cin, Ho, Wo, Cout, k, stride, padding, transposed, act, 0, tap_mask, out=out, out_c_off=out_c_off)
    return out


def copy_into(x, out, out_c_off):
    """``out[:, out_c_off:out_c_off + C] = x`` for NHWC tensors of one dtype (``hesic_copy_channels``)."""
    L.require_cuda(x, out)
    B, Cx, H, W = x.shape
    x = _nhwc(x)
    L.call("hesic_copy_channels", L.ptr(x), L.ptr(out), B * H * W, Cx, Cx, 0, out.shape[1], out_c_off, L.dt(x), L.stream())
    return out


def round_to(x, dtype):
    """round-half-even(x) stored as ``dtype``: ``_quantize(x, "dequantize")`` without means on an fp32 latent."""
    L.require_cuda(x)
    x = x.detach()
    if not (x.is_contiguous() or x.is_contiguous(memory_format=_CL)):
        x = x.contiguous(memory_format=_CL)
    y = torch.empty_like(x, dtype=dtype)
    L.call("hesic_round", L.ptr(x), L.dt(x), L.ptr(y), L.dt(dtype), x.numel(), L.stream())
    return y


# ------------------------------------------------------------------------------------ GDN
def conv3x3_c32_ok(x, weight):
    """Inference-only fast path of the enhancement net's 32-channel 3x3 convs (``hesic_conv3x3_c32_forward``)."""
    return (not torch.is_grad_enabled() and x.is_cuda and x.dim() == 4 and x.shape[1] == 32 and x.dtype == _h16()
            and weight.shape[1] == 32 and tuple(weight.shape[2:]) == (3, 3) and (weight.shape[0] == 32 or weight.shape[0] <= 4)
            and weight.dtype == torch.float32 and _is16())


def pack_images_c32(xa, xb):
    """cat((xa, xb), 1) of two (B,3,H,W) images as channels 0..5 of a zero-padded (B,32,H,W) bf16 NHWC tensor."""
    L.require_cuda(xa, xb)
    B, _, H, W = xa.shape
    out = _empty_nhwc(B, 32, H, W, _h16(), xa.device)
    L.call("hesic_pack_images_c32", L.ptr(xa.float().contiguous()), L.ptr(xb.float().contiguous()), L.ptr(out), B, H, W, L.stream())
    return out


def conv3x3_c32_img6(xa, xb, weight, bias, act=L.ACT_NONE):
    """act(conv3x3(cat((xa, xb), 1)) + bias) of the enhancement net's input layer (newnet1.py:300-301) in ONE launch (round 6,
    ``hesic_conv3x3_c32_forward_img6``): the two fp32 planar (B,3,H,W) images are read as they are, (B,32,H,W) 16-bit NHWC out; bit-identical to
    ``pack_images_c32`` + ``conv3x3_c32`` with the weight zero-padded along Cin."""
    L.require_cuda(xa, xb, weight)
    B, _, H, W = xa.shape
    y = _empty_nhwc(B, 32, H, W, _h16(), xa.device)
    L.call("hesic_conv3x3_c32_forward_img6", L.ptr(xa.float().contiguous()), L.ptr(xb.float().contiguous()), L.ptr(weight.detach().float().contiguous()),
           L.ptr(None if bias is None else bias.detach().float()), int(act), L.ptr(y), B, H, W, L.stream())
    return y


def conv3x3_c32(x, weight, bias, act=L.ACT_NONE, res1=None, res2=None):
    """act(conv3x3(x) + bias) + res1 + res2 in one launch: x (B,32,H,W) bf16 (any layout, made NHWC); 32 couts -> bf16 NHWC
    with bf16 residuals, <= 4 couts -> fp32 planar with one fp32 planar residual (the 32 -> 3 output conv + the image)."""
    L.require_cuda(x, weight)
    B, _, H, W = x.shape
    cout = weight.shape[0]
    x = _nhwc(x)
    w = weight.detach().contiguous()
    if cout == 32:
        y = _empty_nhwc(B, 32, H, W, _h16(), x.device)
        r1 = None if res1 is None else _nhwc(res1.to(_h16()))
        r2 = None if res2 is None else _nhwc(res2.to(_h16()))
    else:
        y = torch.empty((B, cout, H, W), dtype=torch.float32, device=x.device)
        r1 = None if res1 is None else res1.to(torch.float32).contiguous()
        r2 = None
        if res2 is not None:
            raise RuntimeError("conv3x3_c32: the planar form takes one residual")
    L.call("hesic_conv3x3_c32_forward", L.ptr(x), L.ptr(w), L.ptr(None if bias is None else bias.detach().float()), cout, int(act),
           L.ptr(r1), L.ptr(r2), L.ptr(y), B, H, W, L.stream())
    return y


RESBLOCK_FUSED = True      # module switch: a ResidualBlock is ONE launch at inference


def resblock_c32(x, w1, b1, w2, b2, act=L.ACT_LEAKY, res2=None):
    """act(conv3x3(act(conv3x3(x, w1) + b1), w2) + b2) + x + res2 in one launch (``hesic_resblock_c32_forward``): the ResidualBlock of
    the enhancement stage at inference (layers.py:125-147), x (B,32,H,W) in the 16-bit format; round 6: agrees with two ``conv3x3_c32`` calls to the last bits, not bit for bit (another summation order:
    include/hesic_hip.h)."""
    L.require_cuda(x, w1, w2)
    B, _, H, W = x.shape
    x = _nhwc(x)
    y = _empty_nhwc(B, 32, H, W, _h16(), x.device)
    r2 = None if res2 is None else _nhwc(res2.to(_h16()))
    f32 = lambda t: None if t is None else t.detach().float().contiguous()
    L.call("hesic_resblock_c32_forward", L.ptr(x), L.ptr(f32(w1)), L.ptr(f32(b1)), L.ptr(f32(w2)), L.ptr(f32(b2)), int(act), L.ptr(r2), L.ptr(y),
           B, H, W, L.stream())
    return y


EN_TRAIN_FAST = True      # module switch


def conv3x3_c32_train_ok(x, weight):
    """Training form of the 32 -> 32 fast path: autograd on, bf16 storage (stage 2 trains the enhancement net with HSIC frozen,
    newnet1.py:272-311, newtrain6_real.py)."""
    return (EN_TRAIN_FAST and torch.is_grad_enabled() and x.is_cuda and x.dim() == 4 and x.shape[1] == 32 and x.dtype == _h16()
            and weight.shape[0] == 32 and weight.shape[1] <= 32 and tuple(weight.shape[2:]) == (3, 3) and weight.dtype == torch.float32
            and _is16())


def conv3x3_c32_wgrad(x, g, weight, bias):
    """(dw, dbias) of a 3x3 conv over 32-channel NHWC bf16 maps (``hesic_conv3x3_c32_wgrad``): ``x`` the layer input, ``g`` the gradient
    w.r.t. conv + bias; ``weight`` (Cout <= 32, Cin <= 32, 3, 3) and ``bias`` only give shapes / flat gradient slots (with slots the
    gradients are added in place and come back as None)."""
    B, _, H, W = x.shape
    cout, cin = weight.shape[0], weight.shape[1]
    nws = int(L.lib().hesic_conv3x3_c32_wgrad_ws_bytes())
    ws = torch.empty(nws, dtype=torch.uint8, device=x.device)
    sw, sb = _slot_for(weight), (_slot_for(bias) if bias is not None else None)
    if sw is not None and (bias is None or sb is not None):
        L.call("hesic_conv3x3_c32_wgrad", L.ptr(x), L.ptr(g), L.ptr(sw.grad), L.ptr(None if bias is None else sb.grad), cout, cin, 1,
               L.ptr(ws), nws, B, H, W, L.stream())
        _slot_done(sw)
        if bias is not None:
            _slot_done(sb)
        return None, None
    dw = torch.empty((cout, cin, 3, 3), dtype=torch.float32, device=x.device)
    db = torch.empty(cout, dtype=torch.float32, device=x.device) if bias is not None else None
    L.call("hesic_conv3x3_c32_wgrad", L.ptr(x), L.ptr(g), L.ptr(dw), L.ptr(db), cout, cin, 0, L.ptr(ws), nws, B, H, W, L.stream())
    return dw, db


def _mirror_t(weight, pad_to=None):
    """(Cout, Cin, 3, 3) -> the weight of the data-gradient conv: (Cin, Cout, 3, 3) with the taps mirrored, Cout zero-padded to ``pad_to``."""
    wt = weight.detach().flip(2, 3).transpose(0, 1)
    if pad_to is not None and wt.shape[1] < pad_to:
        wt = torch.nn.functional.pad(wt, (0, 0, 0, 0, 0, pad_to - wt.shape[1]))
    return wt.contiguous()


# ------------------------------------------------------------------------------ mirrored data-gradient weights
# train.EnhancerTrainer keeps the data-gradient weight of every 3x3 conv of the enhancement net in ONE flat fp32 buffer that a single launch per
# step refreshes (``c32_mirror_weights``).  The registry follows the gradient slots': a weight is looked up by storage address, and only while the
# gate is on (inside that trainer's step, after its refresh) does a backward pass take the view; everywhere else ``_mirror_t`` runs as before.
_mirror_views = {}
_mirror_active = False


def register_mirror_views(pairs):
    """``pairs``: iterable of (weight parameter, its view of the mirrored flat buffer, shaped like ``_mirror_t(weight, 32)``).  Replaces any view
    registered for the same storage address; returns the registered addresses (for ``clear_mirror_views``)."""
    import weakref
    keys = []
    for p, view in pairs:
        _mirror_views[p.data_ptr()] = (weakref.ref(p), view)
        keys.append(p.data_ptr())
    return keys


def clear_mirror_views(keys=None):
    if keys is None:
        _mirror_views.clear()
    else:
        for k in keys:
            _mirror_views.pop(k, None)


def mirror_views_active(on):
    """Gate of the registry; returns the previous state.  The caller has refreshed the flat buffer on this stream before it turns the gate on."""
    global _mirror_active
    prev, _mirror_active = _mirror_active, bool(on)
    return prev


def _dgrad_weight(weight, pad_to=32):
    """The weight of ``weight``'s data-gradient conv: the registered view while the registry is active, ``_mirror_t`` otherwise."""
    if _mirror_active and _mirror_views:
        hit = _mirror_views.get(weight.data_ptr())
        if hit is not None:
            owner = hit[0]()
            if owner is None or owner.data_ptr() != weight.data_ptr():      # the parameter is gone (its address may have been reused)
                _mirror_views.pop(weight.data_ptr(), None)
            elif hit[1].shape == (weight.shape[1], max(weight.shape[0], pad_to or 0), 3, 3) and hit[1].device == weight.device:
                return hit[1]
    return _mirror_t(weight, pad_to)


def c32_mirror_weights(src, dst, table, n_layers):
    """``hesic_c32_mirror_weights``: the data-gradient weights of ``n_layers`` convs of the flat fp32 buffer ``src`` into the flat fp32 buffer
    ``dst``, one launch; ``table``: a device uint8 tensor holding ``_lib.MirrorEntry`` records."""
    L.require_cuda(src, dst, table)
    L.call("hesic_c32_mirror_weights", L.ptr(src), src.numel(), L.ptr(dst), dst.numel(), L.ptr(table), int(n_layers),
           table.numel() // C.sizeof(L.MirrorEntry), L.stream())
    return dst


def mirror_table(entries, device):
    """A device table for ``c32_mirror_weights`` from ``(src offset, dst offset, cout, cin, cout_pad)`` tuples (offsets in floats)."""
    arr = (L.MirrorEntry * len(entries))(*[L.MirrorEntry(int(s), int(d), int(co), int(ci), int(cp), 0) for s, d, co, ci, cp in entries])
    return torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8).to(device)


def _check_en_images(who, *ts):
    for t in ts:
        if t.dim() != 4 or t.shape[1] != 3 or t.shape != ts[0].shape or t.dtype != torch.float32 or not t.is_contiguous():
            raise ValueError(f"{who}: four dense fp32 (B,3,H,W) tensors of one shape")


def en_loss(a1, b1, a2, b2, lambda_255sq, out=None, ws=None):
    """``hesic_en_loss``: fp64 ``[sse1, sse2, mse_loss, loss]`` of two (enhanced image, target) pairs, dense fp32 planar (B,3,H,W); two launches,
    no atomics.  ``out`` (4 fp64) and ``ws`` (uint8, ``hesic_en_loss_ws_bytes``) are allocated when not given."""
    L.require_cuda(a1, b1, a2, b2, out, ws)
    _check_en_images("en_loss", a1, b1, a2, b2)
    B, _, H, W = a1.shape
    nws = int(L.lib().hesic_en_loss_ws_bytes(B, H, W))
    if nws < 0:
        raise RuntimeError(f"hesic_en_loss_ws_bytes failed: {L.lib().hesic_last_error().decode()}")
    if ws is None:
        ws = torch.empty(nws, dtype=torch.uint8, device=a1.device)
    if out is None:
        out = torch.empty(4, dtype=torch.float64, device=a1.device)
    L.call("hesic_en_loss", L.ptr(a1), L.ptr(b1), L.ptr(a2), L.ptr(b2), B, H, W, float(lambda_255sq), L.ptr(out), L.ptr(ws), ws.numel(), L.stream())
    return out


def en_loss_grad(a1, b1, a2, b2, lambda_255sq, seed=None, out=None):
    """``hesic_en_loss_grad``: the gradient of ``en_loss``'s loss w.r.t. ``a1`` and ``a2`` as two (B,32,H,W) NHWC maps in the 16-bit format (channels
    0..2, the rest zero), one launch; ``seed``: an fp32 device scalar that multiplies the scale, or None; ``out``: the two maps, or None."""
    L.require_cuda(a1, b1, a2, b2, seed)
    _check_en_images("en_loss_grad", a1, b1, a2, b2)
    B, _, H, W = a1.shape
    g1, g2 = out if out is not None else (_empty_nhwc(B, 32, H, W, _h16(), a1.device), _empty_nhwc(B, 32, H, W, _h16(), a1.device))
    L.call("hesic_en_loss_grad", L.ptr(a1), L.ptr(b1), L.ptr(a2), L.ptr(b2), B, H, W, float(lambda_255sq), L.ptr(seed), L.ptr(g1), L.ptr(g2),
           L.stream())
    return g1, g2


def _dense_f32(t):
    return t.detach().to(torch.float32).contiguous()


class _EnCriterionFn(torch.autograd.Function):
    """Both views' 32 -> 3 output convs (+ the images they refine) and the stage-2 criterion as ONE autograd node: forward = two
    ``hesic_conv3x3_c32_forward`` launches and ``hesic_en_loss``; backward = ``hesic_en_loss_grad`` (the gradient lands in the 32-channel map
    directly: no fp32 gradient image, no zero image, no pack) and per view the 32-channel data-gradient conv and ``conv3x3_c32_wgrad`` (flat
    slots honoured).  Outputs: loss, mse_loss (fp64 device scalars), the two enhanced images; only ``loss`` carries a gradient."""

    @staticmethod
    def forward(ctx, t1, w1, b1, img1, x1, t2, w2, b2, img2, x2, lmbda):
        t1, t2 = _nhwc(t1), _nhwc(t2)
        x1, x2 = _dense_f32(x1), _dense_f32(x2)
        y1 = conv3x3_c32(t1, w1, b1, res1=img1)
        y2 = conv3x3_c32(t2, w2, b2, res1=img2)
        ctx.scale = float(lmbda) * 255 ** 2
        out = en_loss(y1, x1, y2, x2, ctx.scale)
        ctx.save_for_backward(t1, w1, t2, w2, y1, x1, y2, x2)
        ctx.biases = (b1, b2)
        loss, mse = out[3], out[2]
        ctx.mark_non_differentiable(mse, y1, y2)
        ctx.set_materialize_grads(False)          # no zero images for the outputs that carry no gradient
        return loss, mse, y1, y2

    @staticmethod
    def backward(ctx, g_loss, *unused):
        t1, w1, t2, w2, y1, x1, y2, x2 = ctx.saved_tensors
        # as in _RdLossFn: g_loss stays on the device and is applied (inside the kernel) only when SCALED_LOSS is on
        seed = g_loss.detach().reshape(1).to(torch.float32) if SCALED_LOSS else None
        g1, g2 = en_loss_grad(y1, x1, y2, x2, ctx.scale, seed)
        grads = []
        for i, (t, w, g, bias) in enumerate(((t1, w1, g1, ctx.biases[0]), (t2, w2, g2, ctx.biases[1]))):
            dt = dw = db = None
            if ctx.needs_input_grad[5 * i]:
                dt = conv3x3_c32(g, _dgrad_weight(w, 32), None)
            if ctx.needs_input_grad[5 * i + 1]:
                dw, db = conv3x3_c32_wgrad(t, g, w, bias)
            grads += [dt, dw, db, None, None]
        return (*grads, None)


def en_criterion_ok(t, weight):
    """The fused stage-2 criterion node applies: a ROCm device, autograd on, the 16-bit training format, a (3,32,3,3) output layer."""
    return (EN_TRAIN_FAST and torch.is_grad_enabled() and t.is_cuda and t.dim() == 4 and t.shape[1] == 32 and t.dtype == _h16() and _is16()
            and tuple(weight.shape) == (3, 32, 3, 3) and weight.dtype == torch.float32)


def en_criterion(t1, w1, b1, img1, x1, t2, w2, b2, img2, x2, lmbda):
    """``loss = lmbda * 255^2 * (MSE(y1, x1) + MSE(y2, x2))`` with ``y_v = conv3x3(t_v, w_v) + b_v + img_v`` (newtrain6_real.py:82-88 on
    ``Enhancement``'s output layer): returns ``(loss, mse_loss, y1, y2)``, fp64 device scalars and the detached fp32 enhanced images."""
    return _EnCriterionFn.apply(t1, w1, b1, img1.float(), x1, t2, w2, b2, img2.float(), x2, lmbda)


class _Conv3x3C32Fn(torch.autograd.Function):
    """act(conv3x3(x) + bias) of the 32-channel enhancement layers under autograd, forward, data gradient AND weight gradient on kernels
    built for the shape: dx = conv3x3(act'(y) * dy, W^T with the taps mirrored) is ``hesic_conv3x3_c32_forward`` on another weight tensor,
    dW / dbias come from ``hesic_conv3x3_c32_wgrad`` (flat slots included).  ``weight`` may have fewer than 32 input channels (the
    6 -> 32 input layer on the zero-padded image map: the kernel then sees the zero-padded weight).  Residual adds stay outside (the
    activation's derivative needs the sign of the un-added output)."""

    @staticmethod
    def forward(ctx, x, weight, bias, act):
        x = _nhwc(x)
        w = weight.detach()
        if w.shape[1] < 32:
            w = torch.nn.functional.pad(w, (0, 0, 0, 0, 0, 32 - w.shape[1]))
        y = conv3x3_c32(x, w, bias, act=act)
        ctx.save_for_backward(x, weight, y if act else None)
        ctx.act, ctx.bias = act, bias
        return y

    @staticmethod
    def backward(ctx, gy):
        x, weight, y_act = ctx.saved_tensors
        gy = _nhwc(gy.to(_h16()))
        if ctx.act:
            g = torch.empty_like(y_act)
            L.call("hesic_act_backward", L.ptr(y_act), L.ptr(gy), L.ptr(g), y_act.numel(), ctx.act, L.dt(y_act), L.stream())
        else:
            g = gy
        dx = dw = db = None
        if ctx.needs_input_grad[0]:
            dx = conv3x3_c32(g, _dgrad_weight(weight, 32), None)      # (a narrower conv's extra input channels get zero gradient)
        if ctx.needs_input_grad[1]:
            dw, db = conv3x3_c32_wgrad(x, g, weight, ctx.bias)
        return dx, dw, db, None


class _Conv3x3C32OutFn(torch.autograd.Function):
    """The 32 -> 3 output conv of ``Enhancement`` plus the image it refines (fp32 planar out) under autograd: the incoming gradient
    goes into channels 0..2 of a zero-padded 32-channel map, after which data and weight gradient are the 32-channel kernels'."""

    @staticmethod
    def forward(ctx, t, weight, bias, image):
        t = _nhwc(t)
        y = conv3x3_c32(t, weight, bias, res1=image)
        ctx.save_for_backward(t, weight)
        ctx.bias = bias
        return y

    @staticmethod
    def backward(ctx, gy):
        t, weight = ctx.saved_tensors
        gy = gy.float().contiguous()
        g32 = pack_images_c32(gy, torch.zeros_like(gy))
        if weight.shape[0] != 3:
            raise NotImplementedError("conv3x3_c32 output layer: 3 output channels")
        dt = dw = db = None
        if ctx.needs_input_grad[0]:
            dt = conv3x3_c32(g32, _mirror_t(weight, 32), None)
        if ctx.needs_input_grad[1]:
            dw, db = conv3x3_c32_wgrad(t, g32, weight, ctx.bias)
        return dt, dw, db, (gy if ctx.needs_input_grad[3] else None)


def conv3x3_c32_train(x, weight, bias, act=L.ACT_NONE, packer=None):
    return _Conv3x3C32Fn.apply(x, weight, bias, act)


def conv3x3_c32_out_train(t, weight, bias, image):
    return _Conv3x3C32OutFn.apply(t, weight, bias, image)


def conv2d_cat(xa, xb, weight, bias, *, kernel_size, stride, padding, transposed=False, packer=None, gdn=None, gdn_on_input=False):
    """conv(torch.cat((xa, xb), 1)) (newnet1.py:643,686).  At inference the 6 -> 3 image-side stages read their two
    3-channel halves straight from the two tensors (``hesic_sconv2d_forward_cat``: no concatenated copy); otherwise the
    ordinary cat + conv2d (autograd) path runs.  ``gdn``: the 3-channel GDN module next to the conv -- applied to the conv's
    output (pre_conv -> GDN, :643-644) or, with ``gdn_on_input``, to ``xa`` before the cat (IGDN -> cat -> after_conv, :684-686);
    fused into the same launch on the fast path."""
    cin = weight.shape[0] if transposed else weight.shape[1]
    cout = weight.shape[1] if transposed else weight.shape[0]
    ok = (not torch.is_grad_enabled() and xa.is_cuda and xb.is_cuda and cin == 6 and cout == 3 and kernel_size == 5 and stride == 1
          and padding == 2 and xa.shape[1] + xb.shape[1] == 6 and xa.shape[-1] >= 128 and xa.shape[0] == xb.shape[0]
          and xa.shape[2:] == xb.shape[2:] and xa.dtype in (torch.float32, _h16()) and xb.dtype in (torch.float32, _h16()))
    fuse = ok and gdn is not None and FUSE_GDN3 and (not gdn_on_input or xa.shape[1] == 3)
    if not ok or (gdn is not None and not fuse):
        gdn_now = None if gdn is None else (lambda t: _gdn_op(t, gdn.beta, gdn.gamma, gdn.inverse, gdn.beta_min))      # the operator, not the module's (deferring) __call__
        if gdn is not None and gdn_on_input:
            xa = gdn_now(xa)
        if ok:
            y = conv2d_cat(xa, xb, weight, bias, kernel_size=kernel_size, stride=stride, padding=padding, transposed=transposed, packer=packer)
        else:
            y = conv2d(torch.cat((xa.float(), xb.float()), 1), weight, bias, kernel_size=kernel_size, stride=stride,
                       padding=padding, transposed=transposed, packer=packer)
        return gdn_now(y) if (gdn is not None and not gdn_on_input) else y
    B, _, H, W = xa.shape
    y = torch.empty((B, cout, H, W), dtype=torch.float32, device=xa.device)
    d = _sdesc(xa, y, cin, cout, kernel_size, stride, padding, transposed)
    xbs = (C.c_int64 * 4)(*xb.stride())
    if fuse:
        L.call("hesic_sconv2d_forward_cat_gdn", C.byref(d), L.ptr(xa), L.ptr(xb), xbs, L.dt(xb), int(xa.shape[1]), L.ptr(_c(weight)),
               L.ptr(bias), L.ptr(_c(gdn.beta)), L.ptr(_c(gdn.gamma)), float(gdn.beta_min), int(bool(gdn.inverse)), int(bool(gdn_on_input)),
               L.ptr(y), L.stream())
    else:
        L.call("hesic_sconv2d_forward_cat", C.byref(d), L.ptr(xa), L.ptr(xb), xbs, L.dt(xb), int(xa.shape[1]),
               L.ptr(_c(weight)), L.ptr(bias), L.ptr(y), L.stream())
    return y


class _GdnFn(torch.autograd.Function):
    """GDN.forward (compressai/layers/gdn.py:55-70), reparametrisation included."""

    @staticmethod
    def forward(ctx, x, beta, gamma, inverse, beta_min):
        L.require_cuda(x, beta, gamma)
        B, Cc, H, W = x.shape
        x = _nhwc(x)
        y = torch.empty_like(x, memory_format=_CL)
        L.call("hesic_gdn_forward", L.ptr(x), L.ptr(_c(beta)), L.ptr(_c(gamma)), L.ptr(y),
               B * H * W, Cc, int(inverse), float(beta_min), L.dt(x), L.stream())
        ctx.save_for_backward(x, beta, gamma)
        ctx.inverse, ctx.beta_min = inverse, beta_min
        return y

    @staticmethod
    def backward(ctx, gy):
        x, beta, gamma = ctx.saved_tensors
        dx, dbeta, dgamma = _gdn_backward(x, _nhwc(gy.to(x.dtype)), beta, gamma, ctx.inverse, ctx.beta_min)
        return dx, dbeta, dgamma, None, None


class _Gdn3PlanarFn(torch.autograd.Function):
    """The 3-channel image-side GDN / IGDN (pre_gdn / after_gdn, newnet1.py:630,669) on a planar tensor under autograd: forward
    ``hesic_gdn_forward_planar``, backward one fused pass (``hesic_gdn_backward_planar_acc``) -- no NHWC copies, planar in and out."""

    @staticmethod
    def forward(ctx, x, beta, gamma, inverse, beta_min):
        L.require_cuda(x, beta, gamma)
        B, Cc, H, W = x.shape
        y = torch.empty_like(x)
        L.call("hesic_gdn_forward_planar", L.ptr(x), L.ptr(_c(beta)), L.ptr(_c(gamma)), L.ptr(y), B, Cc, H * W,
               int(inverse), float(beta_min), L.dt(x), L.stream())
        ctx.save_for_backward(x, beta, gamma)
        ctx.inverse, ctx.beta_min = inverse, beta_min
        return y

    @staticmethod
    def backward(ctx, gy):
        x, beta, gamma = ctx.saved_tensors
        B, Cc, H, W = x.shape
        gy = gy.to(x.dtype).contiguous()
        dx = torch.empty_like(x)
        sb, sg = _slot_for(beta), _slot_for(gamma)
        direct = sb is not None and sg is not None
        dbeta = sb.grad if direct else torch.empty_like(beta, dtype=torch.float32)
        dgamma = sg.grad if direct else torch.empty_like(gamma, dtype=torch.float32)
        ws = torch.empty(64, dtype=torch.uint8, device=x.device)
        L.call("hesic_gdn_backward_planar_acc", L.ptr(x), L.ptr(gy), L.ptr(_c(beta)), L.ptr(_c(gamma)), L.ptr(dx), L.ptr(dbeta),
               L.ptr(dgamma), int(direct), L.ptr(ws), B, H * W, Cc, int(ctx.inverse), float(ctx.beta_min), L.dt(x), L.stream())
        if direct:
            _slot_done(sb)
            _slot_done(sg)
            return dx, None, None, None, None
        return dx, dbeta, dgamma, None, None


GDN3_PLANAR_TRAIN = True      # module switch: False = the NHWC route of rounds 1-3 under autograd


def gdn(x, beta, gamma, inverse=False, beta_min=1e-6):
    if x.shape[1] == 3 and x.is_cuda and x.is_contiguous() and not torch.is_grad_enabled() and x.dtype in (torch.float32, _h16()):
        # image-side GDN on a planar tensor at inference: no NHWC round trip
        B, Cc, H, W = x.shape
        y = torch.empty_like(x)
        L.call("hesic_gdn_forward_planar", L.ptr(x), L.ptr(_c(beta)), L.ptr(_c(gamma)), L.ptr(y), B, Cc, H * W,
               int(inverse), float(beta_min), L.dt(x), L.stream())
        return y
    if (GDN3_PLANAR_TRAIN and x.shape[1] == 3 and x.is_cuda and x.is_contiguous() and x.dtype in (torch.float32, _h16())
            and beta.dtype == torch.float32 and gamma.dtype == torch.float32):
        return _apply(_Gdn3PlanarFn, x, beta, gamma, inverse, beta_min)
    return _apply(_GdnFn, x, beta, gamma, inverse, beta_min)


_gdn_op = gdn          # conv2d_cat's parameter ``gdn`` is the MODULE


# ----------------------------------------------------------------------------------- warp
class _WarpFn(torch.autograd.Function):
    """kornia.warp_perspective(src, M, dsize) (third party; call sites newnet1.py:746,753,767)."""

    @staticmethod
    def forward(ctx, src, M, dsize, align_corners, inverse_map=False):
        L.require_cuda(src, M)
        B, Cc, H, W = src.shape
        Ho, Wo = int(dsize[0]), int(dsize[1])
        if src.dtype not in (torch.float32, _h16()):
            raise TypeError("warp_perspective: float32 or the active 16-bit format only")
        Mf = M.detach().to(torch.float32).contiguous()
        dst = torch.empty((B, Cc, Ho, Wo), dtype=src.dtype, device=src.device)
        ss, ds = src.stride(), dst.stride()
        d = L.WarpDesc(B, Cc, H, W, Ho, Wo, int(align_corners), L.dt(src), L.dt(dst), int(inverse_map), ss[0], ss[1], ss[2], ss[3],
                       ds[0], ds[1], ds[2], ds[3])
        L.call("hesic_warp_perspective_forward", C.byref(d), L.ptr(src), L.ptr(Mf), L.ptr(dst), L.stream())
        ctx.save_for_backward(Mf)
        ctx.meta = (src.shape, src.dtype, Ho, Wo, int(align_corners), int(inverse_map))
        return dst

    @staticmethod
    def backward(ctx, g):
        (Mf,) = ctx.saved_tensors
        shape, sdt, Ho, Wo, ac, inv = ctx.meta
        B, Cc, H, W = shape
        g = g.contiguous()
        dsrc = _zeros(shape, torch.float32, g.device)
        ss, ds = dsrc.stride(), g.stride()
        d = L.WarpDesc(B, Cc, H, W, Ho, Wo, ac, L.F32, L.dt(g), inv, ss[0], ss[1], ss[2], ss[3], ds[0], ds[1], ds[2], ds[3])
        L.call("hesic_warp_perspective_backward", C.byref(d), L.ptr(g), L.ptr(Mf), L.ptr(dsrc), L.stream())
        return dsrc.to(sdt), None, None, None, None


class _WarpMFn(torch.autograd.Function):
    """``_WarpFn`` for a matrix that requires grad: the same forward and source gradient (``_WarpFn``'s own code, which a warp by a constant
    matrix keeps using untouched), plus ``hesic_warp_perspective_backward_m`` on the source kept for it."""

    class _Saved:
        """The part of an autograd context ``_WarpFn`` uses."""

        def save_for_backward(self, *tensors):
            self.saved_tensors = tensors

    @staticmethod
    def forward(ctx, src, M, dsize, align_corners, inverse_map=False):
        inner = _WarpMFn._Saved()
        dst = _WarpFn.forward(inner, src, M, dsize, align_corners, inverse_map)
        ctx.save_for_backward(inner.saved_tensors[0], src.detach())
        ctx.meta, ctx.m_dtype = inner.meta, M.dtype
        return dst

    @staticmethod
    def backward(ctx, g):
        inner = _WarpMFn._Saved()
        Mf, src = ctx.saved_tensors
        inner.saved_tensors, inner.meta = (Mf,), ctx.meta
        dsrc = _WarpFn.backward(inner, g)[0]
        (B, Cc, H, W), _, Ho, Wo, ac, inv = ctx.meta
        g = g.contiguous()
        ss, ds = src.stride(), g.stride()
        d = L.WarpDesc(B, Cc, H, W, Ho, Wo, ac, L.dt(src), L.dt(g), inv, ss[0], ss[1], ss[2], ss[3], ds[0], ds[1], ds[2], ds[3])
        dM = torch.empty((B, 3, 3), dtype=torch.float32, device=g.device)
        L.call("hesic_warp_perspective_backward_m", C.byref(d), L.ptr(src), L.ptr(g), L.ptr(Mf), L.ptr(_htrain_partials(B, g.device)),
               L.ptr(dM), L.stream())
        return dsrc, dM.to(ctx.m_dtype), None, None, None


def _htrain_partials(B, device):
    """The fp64 per-block partials of the image-sized entry points of include/hesic_homography_train.h (written before they are read)."""
    return torch.empty(B * L.HTRAIN_MAX_BLOCKS * L.HTRAIN_PARTIAL_WIDTH, dtype=torch.float64, device=device)


class _PhotometricFn(torch.autograd.Function):
    """mean |bilinear(img_a, h p) - patch_b| with h = DLT(corners - corners[:,0] -> corners + delta); autograd to ``delta`` only."""

    @staticmethod
    def forward(ctx, delta, img_a, patch_b, corners, align_corners):
        L.require_cuda(delta, img_a, patch_b, corners)
        B, Cc, H, W = img_a.shape
        Ho, Wo = patch_b.shape[-2:]
        ss, ds = img_a.stride(), patch_b.stride()
        d = L.WarpDesc(B, Cc, H, W, Ho, Wo, int(align_corners), L.F32, L.F32, 1, ss[0], ss[1], ss[2], ss[3], ds[0], ds[1], ds[2], ds[3])
        dl, cn = delta.detach().contiguous(), corners.contiguous()
        h = torch.empty((B, 9), dtype=torch.float64, device=img_a.device)
        loss = torch.empty((1,), dtype=torch.float32, device=img_a.device)
        L.call("hesic_photometric_forward", C.byref(d), L.ptr(img_a), L.ptr(patch_b), L.ptr(cn), L.ptr(dl), L.ptr(h),
               L.ptr(_htrain_partials(B, img_a.device)), L.ptr(loss), L.stream())
        ctx.save_for_backward(dl, img_a, patch_b, cn, h)
        ctx.desc = d
        return loss.view(())

    @staticmethod
    def backward(ctx, g):
        dl, img_a, patch_b, cn, h = ctx.saved_tensors
        g = g.to(torch.float32).contiguous()
        d_delta = torch.empty_like(dl)
        L.call("hesic_photometric_backward", C.byref(ctx.desc), L.ptr(img_a), L.ptr(patch_b), L.ptr(cn), L.ptr(dl), L.ptr(h), L.ptr(g),
               L.ptr(_htrain_partials(dl.shape[0], dl.device)), L.ptr(d_delta), L.stream())
        return d_delta, None, None, None, None


def photometric_loss(delta, img_a, patch_b, corners, align_corners=True):
    return _apply(_PhotometricFn, delta, img_a, patch_b, corners, align_corners)


class _PerspectiveTransformFn(torch.autograd.Function):
    """kornia.get_perspective_transform (4-point DLT) with the adjoint kernel as its backward."""

    @staticmethod
    def forward(ctx, src, dst):
        L.require_cuda(src, dst)
        H = torch.empty((src.shape[0], 3, 3), dtype=torch.float32, device=src.device)
        L.call("hesic_perspective_transform", L.ptr(src), L.ptr(dst), L.ptr(H), src.shape[0], L.stream())
        ctx.save_for_backward(src, dst)
        return H

    @staticmethod
    def backward(ctx, g):
        src, dst = ctx.saved_tensors
        g = g.to(torch.float32).contiguous()
        d_src = torch.empty_like(src) if ctx.needs_input_grad[0] else None
        d_dst = torch.empty_like(dst) if ctx.needs_input_grad[1] else None
        L.call("hesic_perspective_transform_backward", L.ptr(src), L.ptr(dst), L.ptr(g), L.ptr(d_src), L.ptr(d_dst), src.shape[0], L.stream())
        return d_src, d_dst


def perspective_transform(src, dst):
    """``src``, ``dst``: (B,4,2) fp32 contiguous."""
    return _apply(_PerspectiveTransformFn, src, dst)


class _HFromDeltaFn(torch.autograd.Function):
    """hesic_h_from_delta (DLT, 3x3 inverse, h_adjust) with its adjoint with respect to ``delta``."""

    @staticmethod
    def forward(ctx, corners, delta, ratio_a, ratio_b, subtract_origin):
        L.require_cuda(corners, delta)
        H = torch.empty((corners.shape[0], 3, 3), dtype=torch.float32, device=corners.device)
        L.call("hesic_h_from_delta", L.ptr(corners), L.ptr(delta), ratio_a, ratio_b, subtract_origin, L.ptr(H), corners.shape[0], L.stream())
        ctx.save_for_backward(corners, delta)
        ctx.meta = (ratio_a, ratio_b, subtract_origin)
        return H

    @staticmethod
    def backward(ctx, g):
        corners, delta = ctx.saved_tensors
        if ctx.needs_input_grad[0]:
            raise NotImplementedError("h_matrix_from_delta: the gradient goes to delta only")
        g = g.to(torch.float32).contiguous()
        d_delta = torch.empty_like(delta)
        L.call("hesic_h_from_delta_backward", L.ptr(corners), L.ptr(delta), *ctx.meta, L.ptr(g), L.ptr(d_delta), corners.shape[0], L.stream())
        return None, d_delta, None, None, None


def h_from_delta(corners, delta, ratio_a, ratio_b, subtract_origin):
    """``corners``, ``delta``: (B,4,2) fp32 contiguous."""
    return _apply(_HFromDeltaFn, corners, delta, float(ratio_a), float(ratio_b), int(subtract_origin))


# include/hesic_homography_refine.h: photometric refinement of a pair's homography (homography.refine_h_matrix checks the arguments)
def homography_refine_levels(H, W, levels):
    """Pyramid levels a ``levels``-level refinement of H x W images actually uses (0: the image is below 16 pixels on a side)."""
    n = L.lib().hesic_hrefine_levels(int(H), int(W), int(levels))
    if n < 0:
        raise ValueError(f"homography_refine: levels must lie in [1, {L.HREFINE_MAX_LEVELS}], got {levels}")
    return n


def _strides4(t):
    return (C.c_int64 * 4)(*t.stride())


def homography_refine_pyramid(x1, x2, levels):
    """The grey pyramid of both views in one launch: x1, x2 fp32 (B,C,H,W) of one shape, C in {1,3}, any non-negative strides.  Returns the
    flat fp32 buffer and its levels as views ``[(2, B, H_l, W_l)]`` (view 0: x1)."""
    L.require_cuda(x1, x2)
    B, Cc, H, W = x1.shape
    n = homography_refine_levels(H, W, levels)
    pyr = torch.empty(L.lib().hesic_hrefine_pyramid_elems(B, H, W, n), dtype=torch.float32, device=x1.device)
    L.call("hesic_hrefine_pyramid", L.ptr(x1), _strides4(x1), L.ptr(x2), _strides4(x2), B, Cc, H, W, n, L.ptr(pyr), L.stream())
    views, off = [], 0
    for _ in range(n):
        views.append(pyr[off:off + 2 * B * H * W].view(2, B, H, W))
        off += 2 * B * H * W
        H, W = H // 2, W // 2
    return pyr, views


def homography_refine_normal_eq(pyr, shape, levels, level, A, huber=None):
    """The per-block sums of one candidate per pair on ``level`` of a pyramid built for ``shape`` = (B, H, W) with ``levels`` used levels:
    ``A`` (B,3,3) fp64 in that level's coordinates -> (B, nblk, 46) fp64 (see the header for the 46 sums)."""
    L.require_cuda(pyr, A)
    B, H, W = shape
    A = A.contiguous()
    nblk = L.lib().hesic_hrefine_blocks(H >> level, W >> level)
    partials = torch.empty((B, nblk, L.HREFINE_SUMS), dtype=torch.float64, device=pyr.device)
    L.call("hesic_hrefine_normal_eq", L.ptr(pyr), B, H, W, int(levels), int(level), L.ptr(A), 9, float(huber or 0.0), L.ptr(partials), L.stream())
    return partials


def homography_refine(x1, x2, h, levels=3, iters=10, huber=None, min_overlap=0.25):
    """x1, x2 fp32 (B,C,H,W), ``h`` (B,3,3) fp32 contiguous -> (h_refined (B,3,3) fp32, info (B,8) fp64: cost_before, cost_after, accepted,
    rejected, valid_share, levels_used, refined, 0).  Nothing is read back; the call can be captured into a graph."""
    L.require_cuda(x1, x2, h)
    B, Cc, H, W = x1.shape
    nbytes = L.lib().hesic_homography_refine_ws_bytes(B, H, W, int(levels))
    if nbytes < 0:
        raise ValueError(f"homography_refine: levels must lie in [1, {L.HREFINE_MAX_LEVELS}], got {levels}")
    ws = torch.empty(nbytes // 8, dtype=torch.float64, device=x1.device)
    h_out = torch.empty((B, 3, 3), dtype=torch.float32, device=x1.device)
    info = torch.empty((B, L.HREFINE_INFO), dtype=torch.float64, device=x1.device)
    L.call("hesic_homography_refine", L.ptr(x1), _strides4(x1), L.ptr(x2), _strides4(x2), B, Cc, H, W, L.ptr(h), int(levels), int(iters),
           float(huber or 0.0), float(min_overlap), L.ptr(ws), nbytes, L.ptr(h_out), L.ptr(info), L.stream())
    return h_out, info


# The host path the descriptor-batch entries share (homonet_prepare_items, homonet_synth, both pair gathers): the items as a structured array,
# the per-item checks, a device, the outputs, the upload; each wrapper below is these plus its own launch line.
def _items_array(name, dtype_name, dtype, items):
    """``items`` -- a 1-d structured array of ``dtype`` (the list called ``dtype_name``) or its bytes as a (B, itemsize) uint8 CPU tensor --
    as the contiguous structured array."""
    import numpy as np
    dtype = np.dtype(dtype)
    if torch.is_tensor(items):
        if items.is_cuda or items.dtype != torch.uint8 or items.dim() != 2 or items.shape[1] != dtype.itemsize or not items.is_contiguous():
            raise ValueError(f"{name}: items as a tensor must be a contiguous (B, {dtype.itemsize}) uint8 CPU tensor")
        items = items.numpy().view(dtype).reshape(-1)
    items = np.ascontiguousarray(items)
    if items.dtype != dtype or items.ndim != 1:
        raise ValueError(f"{name}: items must be a 1-d array of {dtype_name}")
    return items


def _item_fields(items):
    """Every item's fields as a dict of Python integers (a sub-array field such as ``delta`` stays an array): one conversion for the whole
    array, a third of the time of a read per field."""
    return [dict(zip(items.dtype.names, row)) for row in items.tolist()]


def _check_stored_crop(name, b, it, cw, ch):
    """The stored-image, crop, column and row conditions of item ``b`` (``it``: its integer fields; ``cw``, ``ch``: the crop read from it)."""
    if it["pitch_px"] < 1 or it["rows"] < 1:
        raise ValueError(f"{name}: item {b} stored image {it['rows']} x {it['pitch_px']}")
    if cw < 1 or ch < 1:
        raise ValueError(f"{name}: item {b} crop {ch} x {cw} (at least one pixel each way)")
    if not (0 <= it["x0"] and it["x0"] + cw <= it["pitch_px"]):
        raise ValueError(f"{name}: item {b} columns [{it['x0']}, {it['x0'] + cw}) outside the stored image's {it['pitch_px']}")
    if not (0 <= it["y0"] and it["y0"] + ch <= it["rows"]):
        raise ValueError(f"{name}: item {b} rows [{it['y0']}, {it['y0'] + ch}) outside the stored image's {it['rows']}")


def _launch_device(*given):
    """The device a descriptor batch goes to: that of the first tensor of ``given`` that is not ``None``, else the current one.  Called after
    the host checks and before anything is allocated."""
    if not torch.cuda.is_available():
        raise RuntimeError("hesic_amd: the HIP path needs a ROCm device (no CPU fallback)")
    for t in given:
        if t is not None:
            return t.device
    return torch.device("cuda", torch.cuda.current_device())


def _outputs(name, out, shapes, device, dtypes=None, what="fp32 tensors"):
    """``out`` validated against ``shapes`` / ``dtypes`` (default: all fp32), or dense tensors of them allocated on ``device``."""
    dtypes = dtypes or [torch.float32] * len(shapes)
    if out is None:
        return [torch.empty(s, dtype=d, device=device) for s, d in zip(shapes, dtypes)]
    L.require_cuda(*out)
    if len(out) != len(shapes) or any(tuple(t.shape) != s or t.dtype != d or not t.is_contiguous() for t, s, d in zip(out, shapes, dtypes)):
        raise ValueError(f"{name}: out must be dense {what} of shapes {shapes}")
    return out


def _upload_items(items, device):
    """The descriptors' bytes on ``device``, through a pinned copy: the caller may reuse ``items`` at once."""
    import numpy as np
    host = torch.from_numpy(items.view(np.uint8).reshape(len(items), items.dtype.itemsize)).pin_memory()
    return host.to(device, non_blocking=True)


def homonet_prepare(x1, x2, xy, pic_size, patch_size, mean, std, out=None):
    """``hesic_homonet_prepare`` (include/hesic_homography_prep.h): ``x1``, ``x2`` (B,3,H,W) uint8 or float32 in [0, 1] with any non-negative
    strides, ``xy`` (B,2) int32 window origins on the device (the CALLER checks 0 <= x, y <= pic_size - patch_size) ->
    ``(grey1, grey2, patch1, patch2, corners)``, fp32, one launch.  ``out``: five preallocated dense fp32 tensors of those shapes."""
    L.require_cuda(x1, x2, xy)
    if x1.dim() != 4 or x1.shape[1] != 3 or x1.shape != x2.shape:
        raise ValueError(f"homonet_prepare: expected two (B,3,H,W) tensors of one shape, got {tuple(x1.shape)}, {tuple(x2.shape)}")
    if x1.dtype != x2.dtype:
        raise TypeError(f"homonet_prepare: the two views differ in dtype ({x1.dtype} vs {x2.dtype})")
    if x1.dtype not in (torch.uint8, torch.float32):
        raise TypeError(f"homonet_prepare: uint8 or float32 images, got {x1.dtype}")
    B, _, H, W = x1.shape
    S, P = int(pic_size), int(patch_size)
    if xy.dtype != torch.int32 or tuple(xy.shape) != (B, 2) or not xy.is_contiguous():
        raise ValueError(f"homonet_prepare: xy must be a contiguous int32 (B,2) tensor, got {xy.dtype} {tuple(xy.shape)}")
    out = _outputs("homonet_prepare", out, [(B, 1, S, S), (B, 1, S, S), (B, 1, P, P), (B, 1, P, P), (B, 4, 2)], x1.device)
    L.call("hesic_homonet_prepare", L.ptr(x1), (C.c_int64 * 4)(*x1.stride()), L.ptr(x2), (C.c_int64 * 4)(*x2.stride()), L.ptr(xy), B, H, W, S, P,
           float(mean), float(std), L.PREP_F32 if x1.dtype == torch.float32 else L.PREP_U8, *[L.ptr(t) for t in out], L.stream())
    return tuple(out)


HOMONET_ITEM_DTYPE = [("left", "<u8"), ("right", "<u8"), ("pitch_px", "<i4"), ("rows", "<i4"), ("x0", "<i4"), ("y0", "<i4"), ("cw", "<i4"),
                      ("ch", "<i4"), ("wx", "<i4"), ("wy", "<i4")]       # hesic_homonet_item as a numpy structured dtype (48 bytes)


def homonet_items(batch):
    """A zeroed host array of ``batch`` ``hesic_homonet_item`` descriptors (numpy structured, fields as in include/hesic_homonet_items.h;
    ``left`` / ``right`` are device addresses as integers)."""
    import numpy as np
    return np.zeros(int(batch), dtype=np.dtype(HOMONET_ITEM_DTYPE))


def _check_homonet_geometry(name, b, it, S, P):
    """The stored-image, crop and window conditions of item ``b`` that the item entries share (``it``: its integer fields)."""
    _check_stored_crop(name, b, it, it["cw"], it["ch"])
    if not (0 <= it["wx"] <= S - P and 0 <= it["wy"] <= S - P):
        raise ValueError(f"{name}: item {b} window origin ({it['wx']}, {it['wy']}) outside [0, {S - P}]")


def check_homonet_items(items, S, P):
    """The per-item conditions ``hesic_homonet_prepare_items`` leaves to its caller, on the host: ValueError names the first item that breaks one."""
    S, P = int(S), int(P)
    for b, it in enumerate(_item_fields(items)):
        if it["left"] == 0 or it["right"] == 0:
            raise ValueError(f"homonet_prepare_items: item {b} has a null view pointer")
        _check_homonet_geometry("homonet_prepare_items", b, it, S, P)


def homonet_prepare_items(items, pic_size, patch_size, mean, std, out=None):
    """``hesic_homonet_prepare_items`` (include/hesic_homonet_items.h): ``items`` the HOST description of the batch -- a numpy array of
    ``HOMONET_ITEM_DTYPE`` (``homonet_items(B)``) or its bytes as a (B, 48) uint8 CPU tensor --, whose ``left`` / ``right`` are addresses of
    uint8 HWC images on the current device.  Every item is checked here, on the host (the C entry cannot read them); the descriptors are
    then uploaded and one launch writes ``(grey1, grey2, patch1, patch2, corners)``, fp32, the outputs of ``homonet_prepare`` on each
    item's crop.  ``out``: five preallocated dense fp32 tensors of those shapes."""
    items = _items_array("homonet_prepare_items", "HOMONET_ITEM_DTYPE", HOMONET_ITEM_DTYPE, items)
    B, S, P = len(items), int(pic_size), int(patch_size)
    if not (1 <= B <= 65535 and 1 <= P <= S <= 16384):
        raise ValueError(f"homonet_prepare_items: need 1 <= B <= 65535 and 1 <= P <= S <= 16384, got B={B} S={S} P={P}")
    check_homonet_items(items, S, P)
    dev = _launch_device(*(out or ())[:1])
    out = _outputs("homonet_prepare_items", out, [(B, 1, S, S), (B, 1, S, S), (B, 1, P, P), (B, 1, P, P), (B, 4, 2)], dev)
    items_dev = _upload_items(items, dev)
    L.call("hesic_homonet_prepare_items", L.ptr(items_dev), B, S, P, float(mean), float(std), *[L.ptr(t) for t in out], L.stream())
    return tuple(out)


HOMONET_SYNTH_ITEM_DTYPE = [("view", "<u8"), ("pitch_px", "<i4"), ("rows", "<i4"), ("x0", "<i4"), ("y0", "<i4"), ("cw", "<i4"), ("ch", "<i4"),
                            ("wx", "<i4"), ("wy", "<i4"), ("delta", "<i4", (8,))]    # hesic_homonet_synth_item as a numpy structured dtype (72 bytes)


def homonet_synth_items(batch):
    """A zeroed host array of ``batch`` ``hesic_homonet_synth_item`` descriptors (numpy structured, fields as in
    include/hesic_homonet_synth.h; ``view`` is a device address as an integer)."""
    import numpy as np
    return np.zeros(int(batch), dtype=np.dtype(HOMONET_SYNTH_ITEM_DTYPE))


def perturbed_quad_is_convex(wx, wy, P, delta):
    """Whether the window's corners [[wx, wy], [wx+P, wy], [wx+P, wy+P], [wx, wy+P]] moved by the eight integers ``delta`` (x, y per corner)
    form a STRICTLY convex quadrilateral: the four cross products of consecutive edges are non-zero and of one sign.  Exact (Python ints)."""
    wx, wy, P = int(wx), int(wy), int(P)
    d = [int(v) for v in delta]
    q = [(wx + d[0], wy + d[1]), (wx + P + d[2], wy + d[3]), (wx + P + d[4], wy + P + d[5]), (wx + d[6], wy + P + d[7])]
    cross = []
    for k in range(4):
        (ax, ay), (bx, by), (cx, cy) = q[k], q[(k + 1) % 4], q[(k + 2) % 4]
        cross.append((bx - ax) * (cy - by) - (by - ay) * (cx - bx))
    return all(c > 0 for c in cross) or all(c < 0 for c in cross)


def check_homonet_synth_items(items, S, P):
    """The per-item conditions ``hesic_homonet_synth_items`` leaves to its caller, on the host: those of ``check_homonet_items`` for the one
    view, and the strict convexity of the perturbed quadrilateral.  ValueError names the first item that breaks one."""
    S, P = int(S), int(P)
    for b, it in enumerate(_item_fields(items)):
        if it["view"] == 0:
            raise ValueError(f"homonet_synth: item {b} has a null view pointer")
        _check_homonet_geometry("homonet_synth", b, it, S, P)
        delta = [int(v) for v in it["delta"]]
        if not perturbed_quad_is_convex(it["wx"], it["wy"], P, delta):
            raise ValueError(f"homonet_synth: item {b} corners + delta {delta} is not a strictly convex quadrilateral")


def homonet_synth(items, pic_size, patch_size, mean, std, align_corners, out=None):
    """``hesic_homonet_synth_items`` (include/hesic_homonet_synth.h): ``items`` the HOST description of the batch -- a numpy array of
    ``HOMONET_SYNTH_ITEM_DTYPE`` (``homonet_synth_items(B)``) or its bytes as a (B, 72) uint8 CPU tensor --, whose ``view`` is the address
    of a uint8 HWC image on the current device.  Every item is checked here, on the host; the descriptors are then uploaded and the entry
    writes ``(grey_a, patch_a, corners, delta, h, grey_b, patch_b)``: fp32 but for ``h`` (B, 9) fp64.  ``out``: seven preallocated dense
    tensors of those shapes and types."""
    items = _items_array("homonet_synth", "HOMONET_SYNTH_ITEM_DTYPE", HOMONET_SYNTH_ITEM_DTYPE, items)
    B, S, P = len(items), int(pic_size), int(patch_size)
    if not (1 <= B <= 65535 and 1 <= P <= S <= 16384):
        raise ValueError(f"homonet_synth: need 1 <= B <= 65535 and 1 <= P <= S <= 16384, got B={B} S={S} P={P}")
    check_homonet_synth_items(items, S, P)
    dev = _launch_device(*(out or ())[:1])
    out = _outputs("homonet_synth", out, [(B, 1, S, S), (B, 1, P, P), (B, 4, 2), (B, 4, 2), (B, 9), (B, 1, S, S), (B, 1, P, P)], dev,
                   [torch.float32] * 4 + [torch.float64] + [torch.float32] * 2, "fp32 tensors (h: fp64)")
    items_dev = _upload_items(items, dev)
    L.call("hesic_homonet_synth_items", L.ptr(items_dev), B, S, P, float(mean), float(std), int(bool(align_corners)),
           *[L.ptr(t) for t in out], L.stream())
    return tuple(out)


PAIR_ITEM_DTYPE = [("left", "<u8"), ("right", "<u8"), ("pitch_px", "<i4"), ("rows", "<i4"), ("x0", "<i4"), ("y0", "<i4"), ("hx", "<i4"),
                   ("hy", "<i4"), ("h_index", "<i4"), ("reserved", "<i4")]       # hesic_pair_item as a numpy structured dtype (48 bytes)


def pair_items(batch):
    """A zeroed host array of ``batch`` ``hesic_pair_item`` descriptors (numpy structured, fields as in include/hesic_pair_batch.h;
    ``left`` / ``right`` are device addresses as integers)."""
    import numpy as np
    return np.zeros(int(batch), dtype=np.dtype(PAIR_ITEM_DTYPE))


PAIR_HFLIP, PAIR_VFLIP, PAIR_SWAP = L.PAIR_HFLIP, L.PAIR_VFLIP, L.PAIR_SWAP       # the bits ``hesic_pair_batch_gather_aug`` reads in ``reserved``
PAIR_FLAG_MASK = PAIR_HFLIP | PAIR_VFLIP | PAIR_SWAP


def check_pair_items(items, n_table, ph, pw, flag_mask=0, name="pair_batch_gather"):
    """The per-item conditions ``hesic_pair_batch_gather`` leaves to its caller, on the host: ValueError names the first item that breaks one.
    ``flag_mask``: the bits ``reserved`` may hold (none for the plain entry, ``PAIR_FLAG_MASK`` for ``hesic_pair_batch_gather_aug``)."""
    for b, it in enumerate(_item_fields(items)):
        if it["left"] == 0 or it["right"] == 0:
            raise ValueError(f"{name}: item {b} has a null view pointer")
        _check_stored_crop(name, b, it, pw, ph)
        if not -1 <= it["h_index"] < n_table:
            raise ValueError(f"{name}: item {b} h_index {it['h_index']} outside [-1, {n_table})")
        if it["reserved"] & ~flag_mask:
            raise ValueError(f"{name}: item {b} reserved field must be 0" if not flag_mask else
                             f"{name}: item {b} reserved field {it['reserved']} holds bits other than HFLIP = 1, VFLIP = 2, SWAP = 4")


def _pair_batch_gather(name, flag_mask, items, h_table, ph, pw, out):
    """Both gather entries: the host checks, the upload of the descriptors, one launch of ``hesic_<name>``."""
    items = _items_array(name, "PAIR_ITEM_DTYPE", PAIR_ITEM_DTYPE, items)
    B, ph, pw = len(items), int(ph), int(pw)
    if B < 1 or ph < 1 or pw < 1:
        raise ValueError(f"{name}: bad shape B={B} ph={ph} pw={pw}")
    n_table = 0
    if h_table is not None:
        L.require_cuda(h_table)
        if h_table.dtype != torch.float64 or h_table.dim() != 2 or h_table.shape[1] != 9 or not h_table.is_contiguous():
            raise ValueError(f"{name}: h_table must be a dense fp64 (N, 9) tensor, got {h_table.dtype} {tuple(h_table.shape)}")
        n_table = h_table.shape[0]
    check_pair_items(items, n_table, ph, pw, flag_mask, name)
    dev = _launch_device(h_table, *(out or ())[:1])
    out = _outputs(name, out, [(B, 3, ph, pw), (B, 3, ph, pw), (B, 3, 3)], dev)
    items_dev = _upload_items(items, dev)
    L.call("hesic_" + name, L.ptr(items_dev), L.ptr(h_table), B, ph, pw, *[L.ptr(t) for t in out], L.stream())
    return tuple(out)


def pair_batch_gather(items, h_table, ph, pw, out=None):
    """``hesic_pair_batch_gather`` (include/hesic_pair_batch.h): ``items`` the HOST description of the batch -- a numpy array of
    ``PAIR_ITEM_DTYPE`` (``pair_items(B)``) or its bytes as a (B, 48) uint8 CPU tensor --, whose ``left`` / ``right`` are addresses of uint8
    HWC images on the current device; ``h_table`` a dense fp64 (N, 9) device tensor or ``None``.  Every item is checked here, on the host
    (the C entry cannot read them); the descriptors are then uploaded and one launch writes ``(x1, x2, h)``: (B,3,ph,pw), (B,3,ph,pw),
    (B,3,3), fp32.  ``out``: three preallocated dense fp32 tensors of those shapes."""
    return _pair_batch_gather("pair_batch_gather", 0, items, h_table, ph, pw, out)


def pair_batch_gather_aug(items, h_table, ph, pw, out=None):
    """``hesic_pair_batch_gather_aug`` (include/hesic_pair_augment.h): ``pair_batch_gather`` -- the same arguments, host checks and outputs --
    with each item's ``reserved`` read as any combination of ``PAIR_HFLIP`` = 1 (both views mirrored left-right), ``PAIR_VFLIP`` = 2 (top-bottom)
    and ``PAIR_SWAP`` = 4 (``x1`` from the right view, ``x2`` from the left), the homography following the pixels (``F H F``, the inverse).  Any
    other bit raises ValueError naming the item, here on the host before any launch: the C entry cannot read the descriptors and ignores it."""
    return _pair_batch_gather("pair_batch_gather_aug", PAIR_FLAG_MASK, items, h_table, ph, pw, out)


# ------------------------------------------------------------------------------ HomographyNet in training mode
# include/hesic_homography_net.h: the pieces of ywz/mywork/model.py:73-101 that are not convolutions, with their gradients.
class _MaxPool2Fn(torch.autograd.Function):
    """nn.MaxPool2d(2, 2) on a channels_last map.  The backward recomputes the argmax from the input (saved anyway: it is the ``y_act`` of the
    conv in front) -- first maximum in the scan order (0,0), (0,1), (1,0), (1,1), torch's rule -- and writes every element of the gradient."""

    @staticmethod
    def forward(ctx, x):
        L.require_cuda(x)
        x = _nhwc(x)
        B, Cc, H, W = x.shape
        y = _empty_nhwc(B, Cc, H // 2, W // 2, x.dtype, x.device)
        L.call("hesic_maxpool2_forward", L.ptr(x), L.ptr(y), B, H, W, Cc, L.dt(x), L.stream())
        ctx.save_for_backward(x)
        return y

    @staticmethod
    def backward(ctx, gy):
        (x,) = ctx.saved_tensors
        B, Cc, H, W = x.shape
        gy = _nhwc(gy.to(x.dtype))
        gx = _empty_nhwc(B, Cc, H, W, x.dtype, x.device)
        L.call("hesic_maxpool2_backward", L.ptr(x), L.ptr(gy), L.ptr(gx), B, H, W, Cc, L.dt(x), L.stream())
        return gx


def max_pool2(x):
    return _apply(_MaxPool2Fn, x)


def dropout_args(p, seed=0, step=0, site=0):
    """The by-value arguments of ``hesic_flatten_dropout_*`` for drop probability ``p``: (thr, scale, seed, step, site) with
    thr = round-half-even(p * 2^32) clamped to [0, 2^32 - 1] and scale = 1.0f / (1.0f - (float)p) as an fp32 value."""
    import numpy as np
    p = float(p)
    if not (0.0 <= p and np.float32(p) < np.float32(1.0)):
        raise ValueError(f"dropout: p must be in [0, 1) as an fp32 value, got {p}")
    thr = min(max(int(round(p * 4294967296.0)), 0), 4294967295)
    scale = float(np.float32(1.0) / (np.float32(1.0) - np.float32(p)))
    return thr, scale, int(seed) & 0xFFFFFFFFFFFFFFFF, int(step) & 0xFFFFFFFF, int(site) & 0xFFFFFFFF


def dropout_state_args(p, taken, site=0):
    """The arguments of ``hesic_flatten_dropout_*_state`` for drop probability ``p``: ``dropout_args``' (thr, scale, ., ., site) with
    ``(seed, step)`` replaced by ``taken``, the 16-byte device tensor ``dropout_state_take`` wrote."""
    if not (isinstance(taken, torch.Tensor) and taken.is_cuda and taken.is_contiguous() and taken.numel() * taken.element_size() == 16):
        raise ValueError("dropout: taken must be a contiguous 16-byte device tensor (what dropout_state_take returns)")
    thr, scale, _, _, site = dropout_args(p, 0, 0, site)
    return thr, scale, taken, site


def dropout_state(seed, step, device):
    """The dropout state in device memory: int32 words {seed lo, seed hi, step, reserved = 0} (``include/hesic_dropout_state.h``)."""
    return torch.from_numpy(_dropout_words(seed, step)).to(device)


def _dropout_words(seed, step):
    import numpy as np
    seed, step = int(seed) & 0xFFFFFFFFFFFFFFFF, int(step) & 0xFFFFFFFF
    return np.array([seed & 0xFFFFFFFF, seed >> 32, step, 0], dtype=np.uint32).view(np.int32)


def dropout_state_take(state):
    """One launch: a fresh 16-byte tensor with the four words of ``state``, whose step is then incremented on the device."""
    L.require_cuda(state)
    taken = torch.empty_like(state)
    L.call("hesic_dropout_state_take", L.ptr(state), L.ptr(taken), L.stream())
    return taken


class _FlattenDropoutFn(torch.autograd.Function):
    """``x.reshape(B, -1)`` of the reference (NCHW flatten order) of a channels_last map -- or a (B, F) matrix as it is -- with inverted
    dropout on the way; the mask is a Philox4x32-10 stream of (seed, step, site, logical index) that the backward regenerates.  ``cfg`` is
    ``dropout_args``' by-value tuple or ``dropout_state_args``' (the ``_state`` entries: seed and step read from ``taken`` on the device,
    by the backward too)."""

    @staticmethod
    def _call(which, src, dst, B, HW, Cc, cfg, dt):
        if len(cfg) == 4:
            thr, scale, taken, site = cfg
            L.call(f"hesic_flatten_dropout_{which}_state", L.ptr(src), L.ptr(dst), B, HW, Cc, thr, scale, L.ptr(taken), site, dt, L.stream())
        else:
            L.call(f"hesic_flatten_dropout_{which}", L.ptr(src), L.ptr(dst), B, HW, Cc, *cfg, dt, L.stream())

    @staticmethod
    def forward(ctx, x, cfg):
        L.require_cuda(x)
        if x.dim() == 4:
            x = _nhwc(x)
            B, Cc, HW = x.shape[0], x.shape[1], x.shape[2] * x.shape[3]
        else:
            x = x.contiguous()
            (B, Cc), HW = x.shape, 1
        y = torch.empty((B, Cc * HW), dtype=x.dtype, device=x.device)
        _FlattenDropoutFn._call("forward", x, y, B, HW, Cc, cfg, L.dt(x))
        ctx.cfg, ctx.shape, ctx.dtype = cfg, tuple(x.shape), x.dtype
        return y

    @staticmethod
    def backward(ctx, gy):
        shape = ctx.shape
        gy = gy.to(ctx.dtype).contiguous()
        if len(shape) == 4:
            gx = _empty_nhwc(*shape, ctx.dtype, gy.device)
            B, Cc, HW = shape[0], shape[1], shape[2] * shape[3]
        else:
            gx = torch.empty(shape, dtype=ctx.dtype, device=gy.device)
            (B, Cc), HW = shape, 1
        _FlattenDropoutFn._call("backward", gy, gx, B, HW, Cc, ctx.cfg, L.dt(ctx.dtype))
        return gx, None


def flatten_dropout(x, cfg):
    """``cfg`` = ``dropout_args(p, seed, step, site)`` or ``dropout_state_args(p, taken, site)``; p = 0 is the plain flatten."""
    return _apply(_FlattenDropoutFn, x, cfg)


class _LinearFn(torch.autograd.Function):
    """act(x W^T + b) for up to ``_lib.LINEAR_MAX_ROWS`` rows over the fp32 master weight in nn.Linear's layout (no packed copy): the
    weight is streamed once by the forward, once by the data gradient, and its gradient written once, into the flat slot when it has one."""

    @staticmethod
    def forward(ctx, x, weight, bias, act):
        L.require_cuda(x, weight)
        if x.dim() != 2 or weight.dim() != 2 or x.shape[1] != weight.shape[1]:
            raise RuntimeError(f"linear: expected x (B, In) and weight (Out, In), got {tuple(x.shape)}, {tuple(weight.shape)}")
        if weight.dtype != torch.float32 or (bias is not None and bias.dtype != torch.float32):
            raise TypeError("linear: fp32 weight and bias")
        x = x.contiguous()
        B, In = x.shape
        Out = weight.shape[0]
        nws = int(L.lib().hesic_linear_forward_ws_bytes(B, In, Out))
        ws = torch.empty(max(nws, 16), dtype=torch.uint8, device=x.device)
        y = torch.empty((B, Out), dtype=x.dtype, device=x.device)
        L.call("hesic_linear_forward", L.ptr(x), L.ptr(_c(weight)), L.ptr(bias), L.ptr(y), B, In, Out, act, L.dt(x), L.ptr(ws), nws, L.stream())
        ctx.save_for_backward(x, weight, y if act else None)
        ctx.act, ctx.has_bias, ctx.bias = act, bias is not None, bias
        return y

    @staticmethod
    def backward(ctx, gy):
        x, weight, y_act = ctx.saved_tensors
        B, In = x.shape
        Out = weight.shape[0]
        gy = gy.to(x.dtype).contiguous()
        if ctx.act:
            g2 = torch.empty_like(y_act)
            L.call("hesic_act_backward", L.ptr(y_act), L.ptr(gy), L.ptr(g2), y_act.numel(), ctx.act, L.dt(y_act), L.stream())
            gy = g2
        dx = dw = db = None
        if ctx.needs_input_grad[0]:
            dx = torch.empty_like(x)
            L.call("hesic_linear_dgrad", L.ptr(gy), L.ptr(_c(weight)), L.ptr(dx), B, In, Out, L.dt(x), L.stream())
        if ctx.needs_input_grad[1] or (ctx.has_bias and ctx.needs_input_grad[2]):
            # flat gradient slots: an untouched (cleared) slot is written directly, a slot that already holds a gradient is added to.  One
            # flag serves both outputs: adding into a cleared slot is the same as writing it, and a plain output is zero-filled first.
            ws_ = _slot_for(weight) if weight.is_contiguous() else None
            bs_ = _slot_for(ctx.bias) if ctx.has_bias else None
            accumulate = int((ws_ is not None and ws_.writes > 0) or (bs_ is not None and bs_.writes > 0))
            fresh = _zeros if accumulate else torch.empty
            dw = ws_.grad if ws_ is not None else fresh(weight.shape, dtype=torch.float32, device=x.device)
            db = (bs_.grad if bs_ is not None else fresh((Out,), dtype=torch.float32, device=x.device)) if ctx.has_bias else None
            L.call("hesic_linear_wgrad", L.ptr(x), L.ptr(gy), L.ptr(dw), L.ptr(db), B, In, Out, accumulate, L.dt(x), L.stream())
            if ws_ is not None:
                _slot_done(ws_)
                dw = None
            if bs_ is not None:
                _slot_done(bs_)
                db = None
        return dx, dw, db, None


def linear(x, weight, bias, act=L.ACT_NONE, packer=None):
    """``F.linear`` (+ fused ReLU) on the HIP path.  Up to ``_lib.LINEAR_MAX_ROWS`` rows: the small-batch kernels over the fp32 master weight;
    more rows: the 1x1 implicit-GEMM conv route (``conv2d`` with its packed weight copies), so that large batches still train."""
    if x.shape[0] > L.LINEAR_MAX_ROWS:
        B, In = x.shape
        y = conv2d(x.reshape(B, In, 1, 1).contiguous(memory_format=_CL), weight.view(weight.shape[0], In, 1, 1), bias, kernel_size=1, stride=1,
                   padding=0, act=act, packer=packer)
        return y.reshape(B, -1)
    return _apply(_LinearFn, x, weight, bias, act)


def warp_perspective(src, M, dsize, align_corners=True, inverse_map=False):
    """``inverse_map``: ``M`` already maps destination pixels to source pixels, i.e. this is the warp by ``M^-1``
    (Independent_EN warps view 2 by ``torch.inverse(h_matrix)``, newnet1.py:1290-1291: no 3x3 inversion launches)."""
    if torch.is_grad_enabled() and M.requires_grad:
        return _apply(_WarpMFn, src, M, dsize, align_corners, inverse_map)
    return _apply(_WarpFn, src, M, dsize, align_corners, inverse_map)


# ---------------------------------------------------------------------- entropy bottleneck
EB_BOUND_SLOT = 60


def eb_pack_params(matrices, biases, factors, quantiles, lik_bound=1e-9):
    """[C][64] fp32 table read by hesic_eb_forward/backward (layout in csrc/entropy.hip); slot 60 = likelihood lower bound."""
    Cc = quantiles.shape[0]
    cols = [m.reshape(Cc, -1) for m in matrices] + [b.reshape(Cc, -1) for b in biases] + \
           [f.reshape(Cc, -1) for f in factors] + [quantiles[:, 0, 1:2]]
    t = torch.cat(cols, 1).to(torch.float32)
    assert t.shape[1] == 59, "EntropyBottleneck kernels are specialised for filters=(3,3,3,3)"
    t = torch.nn.functional.pad(t, (0, L.EB_PARAM_STRIDE - 59)).contiguous()
    t[:, EB_BOUND_SLOT] = float(lik_bound)
    return t


def eb_unpack_grads(dparams, matrices, biases, factors, quantiles):
    out, o = [], 0
    for group in (matrices, biases, factors):
        for p in group:
            n = p[0].numel()
            out.append(dparams[:, o:o + n].reshape(p.shape).to(p.dtype))
            o += n
    dq = _zeros(quantiles.shape, quantiles.dtype, quantiles.device)
    dq[:, 0, 1] = dparams[:, 58]
    return out, dq


def _eb_layout(matrices, biases, factors, quantiles, lik_bound=0.0, grads=False):
    """``EbLayout`` of a bottleneck's 14 parameter tensors (or, ``grads``: of their flat gradient slots; None if any has no
    slot).  Table columns: matrices, then biases, then factors, each (C, rows, cols) flattened per channel; column 58 = the
    median = quantiles[:, 0, 1]."""
    lay = L.EbLayout()
    col, j = 0, 0
    for group in (matrices, biases, factors):
        for p in group:
            t = p
            if grads:
                sl = _slot_for(p)
                if sl is None:
                    return None
                t = sl.grad
            n = p[0].numel()
            lay.ptr[j], lay.width[j], lay.stride[j], lay.first[j], lay.col[j] = t.data_ptr(), n, n, 0, col
            col += n
            j += 1
    if col != 58:
        raise NotImplementedError("EntropyBottleneck kernels are specialised for filters=(3,3,3,3)")
    t = quantiles
    if grads:
        sl = _slot_for(quantiles)
        if sl is None:
            return None
        t = sl.grad
    lay.ptr[j], lay.width[j], lay.stride[j], lay.first[j], lay.col[j] = t.data_ptr(), 1, 3, 1, 58
    lay.n, lay.lik_bound = j + 1, float(lik_bound)
    return lay


def _eb_table(matrices, biases, factors, quantiles, lik_bound):
    """The raw [C][64] parameter table in one launch (``hesic_eb_pack_table``)."""
    ps = (*matrices, *biases, *factors, quantiles)
    if not all(p.is_cuda and p.dtype == torch.float32 and p.is_contiguous() for p in ps):
        return eb_pack_params([m.detach() for m in matrices], [b.detach() for b in biases], [f.detach() for f in factors],
                              quantiles.detach(), lik_bound)
    Cc = quantiles.shape[0]
    table = torch.empty((Cc, L.EB_PARAM_STRIDE), dtype=torch.float32, device=quantiles.device)
    lay = _eb_layout(matrices, biases, factors, quantiles, lik_bound)
    L.call("hesic_eb_pack_table", C.byref(lay), L.ptr(table), Cc, L.stream())
    return table


class _EbFn(torch.autograd.Function):
    """EntropyBottleneck.forward (entropy_models.py:384-411): returns (z_hat, likelihood)."""

    @staticmethod
    def forward(ctx, z, noise, quantiles, n_mat, lik_bound, *params):
        L.require_cuda(z)
        matrices, biases, factors = params[:n_mat], params[n_mat:2 * n_mat], params[2 * n_mat:]
        B, Cc, H, W = z.shape
        z = _nhwc(z)
        table = _eb_table(matrices, biases, factors, quantiles, lik_bound)
        zh = torch.empty_like(z, memory_format=_CL)
        lik = _empty_nhwc(B, Cc, H, W, torch.float32, z.device)
        nz = None if noise is None else _nhwc(noise.to(z.dtype))
        L.call("hesic_eb_forward", L.ptr(z), L.ptr(table), L.ptr(nz), L.ptr(zh), L.ptr(lik), None, B * H * W, Cc,
               L.dt(z), L.stream())
        ctx.save_for_backward(z, table, nz, quantiles, *params)
        ctx.n_mat = n_mat
        return zh, lik

    @staticmethod
    def backward(ctx, g_zh, g_lik):
        z, table, nz, quantiles, *params = ctx.saved_tensors
        n_mat = ctx.n_mat
        B, Cc, H, W = z.shape
        dz = torch.empty_like(z, memory_format=_CL)
        dpar = _zeros(table.shape, table.dtype, table.device)
        g_lik = _nhwc(g_lik.to(torch.float32))
        g_zh = None if g_zh is None else _nhwc(g_zh.to(z.dtype))
        L.call("hesic_eb_backward", L.ptr(z), L.ptr(table), L.ptr(nz), L.ptr(g_lik), L.ptr(g_zh), L.ptr(dz), L.ptr(dpar),
               B * H * W, Cc, L.dt(z), L.stream())
        glay = _eb_layout(params[:n_mat], params[n_mat:2 * n_mat], params[2 * n_mat:], quantiles, grads=True)
        if glay is not None:          # flat gradient slots: one scatter-add launch instead of 14 slice copies + AccumulateGrad
            L.call("hesic_eb_scatter_grads", C.byref(glay), L.ptr(dpar), Cc, 1, L.stream())
            for p in (*params, quantiles):
                _slot_done(_slot_for(p))
            return (dz, None, None, None, None, *([None] * len(params)))
        grads, dq = eb_unpack_grads(dpar, params[:n_mat], params[n_mat:2 * n_mat], params[2 * n_mat:], quantiles)
        return (dz, None, dq, None, None, *grads)


class PackedEb:
    """The [C][64] parameter table of an EntropyBottleneck; inference-only cache (same policy as PackedWeight)."""

    def __init__(self):
        self._hit = None

    def get(self, matrices, biases, factors, quantiles, lik_bound=1e-9):
        ps = (*matrices, *biases, *factors, quantiles)
        tag = tuple((p.data_ptr(), p._version) for p in ps) + (_cache_epoch, float(lik_bound))
        if self._hit is None or self._hit[0] != tag:
            raw = _eb_table(matrices, biases, factors, quantiles, lik_bound)
            ready = torch.empty_like(raw)           # softplus / tanh applied once here, not per thread and launch
            L.call("hesic_eb_prepare_params", L.ptr(raw), L.ptr(ready), raw.shape[0], L.stream())
            self._hit = (tag, ready)
        return self._hit[1]


def entropy_bottleneck(z, matrices, biases, factors, quantiles, noise=None, packer=None, out_dtype=None, lik_bound=1e-9):
    """``out_dtype`` (inference, fp32 ``z`` only): storage of z_hat when it differs from z's (bf16 mode with fp32 latents)."""
    if packer is not None and noise is None and not torch.is_grad_enabled():
        # inference: cached parameter table, no autograd bookkeeping -- one launch
        L.require_cuda(z)
        B, Cc, H, W = z.shape
        z = _nhwc(z)
        table = packer.get(matrices, biases, factors, quantiles, lik_bound)
        if out_dtype is not None and out_dtype != z.dtype and z.dtype == torch.float32:
            zh = _empty_nhwc(B, Cc, H, W, out_dtype, z.device)
            lik = _empty_nhwc(B, Cc, H, W, torch.float32, z.device)
            L.call("hesic_eb_forward_f32in", L.ptr(z), L.ptr(table), L.ptr(zh), L.dt(out_dtype), L.ptr(lik), None, B * H * W, Cc, L.stream())
            return zh, lik
        zh = torch.empty_like(z, memory_format=_CL)
        lik = _empty_nhwc(B, Cc, H, W, torch.float32, z.device)
        L.call("hesic_eb_forward", L.ptr(z), L.ptr(table), None, L.ptr(zh), L.ptr(lik), None, B * H * W, Cc, L.dt(z), L.stream())
        return zh, lik
    return _apply(_EbFn, z, noise, quantiles, len(matrices), float(lik_bound), *matrices, *biases, *factors)


class _EbAuxFn(torch.autograd.Function):
    """EntropyBottleneck.loss (entropy_models.py:345-348): sum |c(quantiles) - target| with the cumulative's parameters
    detached -- forward AND the quantile gradient in one launch (the tensor-op form is ~35 launches per bottleneck)."""

    @staticmethod
    def forward(ctx, quantiles, tail_mass, n_mat, *params):
        L.require_cuda(quantiles)
        matrices, biases, factors = params[:n_mat], params[n_mat:2 * n_mat], params[2 * n_mat:]
        Cc = quantiles.shape[0]
        table = _eb_table(matrices, biases, factors, quantiles, 0.0)
        loss = _zeros(1, torch.float32, quantiles.device)
        dq = torch.empty_like(quantiles, dtype=torch.float32)
        L.call("hesic_eb_aux_loss", L.ptr(table), L.ptr(_c(quantiles)), float(tail_mass), L.ptr(loss), L.ptr(dq), Cc, 0, L.stream())
        ctx.save_for_backward(dq)
        ctx.n_params = len(params)
        return loss.reshape(())

    @staticmethod
    def backward(ctx, g):
        (dq,) = ctx.saved_tensors
        return (dq * g, None, None, *([None] * ctx.n_params))


def eb_aux_loss(matrices, biases, factors, quantiles, tail_mass=1e-9):
    return _EbAuxFn.apply(quantiles, float(tail_mass), len(matrices), *matrices, *biases, *factors)


# ------------------------------------------------------------ Gaussian (mixture) conditional
class _GmmFn(torch.autograd.Function):
    """GaussianMixtureConditional.forward (entropy_models.py:661-702) for K>1 with weights, and
    GaussianConditional.forward (:546-554) for K==1 (means optional, used in the quantiser)."""

    @staticmethod
    def forward(ctx, y, scales, means, weights, noise, K, use_means_in_quant, scale_bound, lik_bound):
        L.require_cuda(y, scales, means)
        B, M, H, W = y.shape
        y = _nhwc(y)
        if means is None:
            means = _zeros(scales.shape, scales.dtype, scales.device).contiguous(memory_format=_CL) if scales.dim() == 4 else _zeros(scales.shape, scales.dtype, scales.device)
        # scales / means may be channel slices of one tensor (chunk(2,1)): read in place
        ps, sptr, mptr, _keep = _sm_pointers(_nd(scales), _nd(means), y, B, K, M)
        if ps == K * M:
            scales, means = _keep
        wts = None if weights is None else weights.detach().reshape(B, K * M).to(torch.float32).contiguous()
        yh = torch.empty_like(y, memory_format=_CL)
        lik = _empty_nhwc(B, M, H, W, torch.float32, y.device)
        nz = None if noise is None else _nhwc(noise.to(y.dtype))
        d = L.GmmDesc(B, H * W, M, K, L.dt(y), int(use_means_in_quant), ps, 0, 0, float(scale_bound), float(lik_bound))
        L.call("hesic_gmm_forward", C.byref(d), L.ptr(y), sptr, mptr, L.ptr(wts), L.ptr(nz), L.ptr(yh), L.ptr(lik), None,
               L.stream())
        ctx.save_for_backward(y, scales, means, wts, nz)
        ctx.meta = (K, int(use_means_in_quant), float(scale_bound), float(lik_bound), weights is not None)
        return yh, lik

    @staticmethod
    def backward(ctx, g_yh, g_lik):
        y, scales, means, wts, nz = ctx.saved_tensors
        K, umq, sb, lb, has_w = ctx.meta
        B, M, H, W = y.shape
        scales, means = _nhwc(scales.to(y.dtype)), _nhwc(means.to(y.dtype))
        dy = torch.empty_like(y, memory_format=_CL)
        dsc = torch.empty_like(scales, memory_format=_CL)
        dmu = torch.empty_like(means, memory_format=_CL)
        dw = _zeros((B, K * M), torch.float32, y.device) if has_w else None
        g_lik = _nhwc(g_lik.to(torch.float32))
        g_yh = None if g_yh is None else _nhwc(g_yh.to(y.dtype))
        d = L.GmmDesc(B, H * W, M, K, L.dt(y), umq, K * M, 0, 0, sb, lb)
        L.call("hesic_gmm_backward", C.byref(d), L.ptr(y), L.ptr(scales), L.ptr(means), L.ptr(wts), L.ptr(nz), L.ptr(g_lik),
               L.ptr(g_yh), L.ptr(dy), L.ptr(dsc), L.ptr(dmu), L.ptr(dw), L.stream())
        if dw is not None:
            dw = dw.reshape(B, K * M, 1, 1)
        return dy, dsc, dmu, dw, None, None, None, None, None


def _sm_pointers(scales, means, y, B, K, M):
    """(pixel stride, scales ptr, means ptr, keep-alive) of the two parameter maps in ``y``'s dtype.  Channel slices of wider
    channels_last tensors (``chunk(2, 1)`` of HESIC+'s entropy parameters, the sigma | means halves of the grouped hyper-synthesis
    output) are read in place: all the kernels need is NHWC with one common pixel stride."""
    def nhwc_stride(t):
        if t.dim() != 4 or t.dtype != y.dtype or t.shape[0] != B or t.shape[2:] != y.shape[2:]:
            return None
        sb, sc, sh, sw = t.stride()
        H, W = t.shape[2], t.shape[3]
        ok = sc == 1 and sw >= t.shape[1] and (W == 1 or sh == W * sw) and (B == 1 or sb == H * W * sw) and (H == 1 or sh == W * sw)
        return sw if ok else None
    ps_s, ps_m = nhwc_stride(scales), nhwc_stride(means)
    if ps_s is not None and ps_s == ps_m and scales.shape[1] == K * M and means.shape[1] == K * M:
        return ps_s, L.ptr(scales), L.ptr(means), (scales, means)
    scales, means = _nhwc(scales.to(y.dtype)), _nhwc(means.to(y.dtype))
    return K * M, L.ptr(scales), L.ptr(means), (scales, means)


def _gmm_f32in(y, scales, means, weights, K, use_means_in_quant, scale_bound, lik_bound, out_dtype):
    """Inference with fp32 latents / parameters and y_hat stored as ``out_dtype`` (``hesic_gmm_forward_f32in``)."""
    L.require_cuda(y, scales, means)
    B, M, H, W = y.shape
    y = _nhwc(y.detach())
    ps, sptr, mptr, keep = _sm_pointers(scales.detach(), means.detach(), y, B, K, M)
    wts = None if weights is None else weights.detach().reshape(B, K * M).to(torch.float32).contiguous()
    yh = _empty_nhwc(B, M, H, W, out_dtype, y.device)
    lik = _empty_nhwc(B, M, H, W, torch.float32, y.device)
    d = L.GmmDesc(B, H * W, M, K, L.F32, int(use_means_in_quant), ps, 0, 0, float(scale_bound), float(lik_bound))
    L.call("hesic_gmm_forward_f32in", C.byref(d), L.ptr(y), sptr, mptr, L.ptr(wts), L.ptr(yh), L.dt(out_dtype), L.ptr(lik), None, L.stream())
    del keep
    return yh, lik


def _use_f32in(y, noise, out_dtype, K, M):
    return (out_dtype is not None and out_dtype != y.dtype and y.dtype == torch.float32 and noise is None and not torch.is_grad_enabled()
            and K in (1, 5) and M % 2 == 0 and y.is_cuda)


def gaussian_mixture(y, scales, means, weights, K, noise=None, scale_bound=0.11, lik_bound=1e-9, out_dtype=None):
    if _use_f32in(y, noise, out_dtype, K, y.shape[1]):
        return _gmm_f32in(y, scales, means, weights, K, False, scale_bound, lik_bound, out_dtype)
    return _apply(_GmmFn, y, scales, means, weights, noise, K, False, scale_bound, lik_bound)


def gaussian_conditional(y, scales, means=None, noise=None, scale_bound=0.11, lik_bound=1e-9, out_dtype=None):
    if means is not None and _use_f32in(y, noise, out_dtype, 1, y.shape[1]):
        return _gmm_f32in(y, scales, means, None, 1, True, scale_bound, lik_bound, out_dtype)
    return _apply(_GmmFn, y, scales, means, None, noise, 1, means is not None, scale_bound, lik_bound)


def gmm_cdf_tables(scales, means, weights, channels, minmax, K, b=0, scale_bound=0.11):
    """Per-element cumulative-frequency tables of the real bit-stream (HSIC.compress / decompress,
    ywz/mywork/newnet1.py:925-978): returns an int32 tensor (len(channels), H, W, 2*minmax+2) on the device whose rows
    are the uint32 tables [0, cumsum(round(clip(pmf)/sum*65536))] of image ``b``."""
    L.require_cuda(scales, means)
    B, KM, H, W = scales.shape
    M = KM // K
    dt = scales.dtype
    scales, means = _nhwc(scales), _nhwc(means.to(dt))
    wts = None if weights is None else weights.detach().reshape(B, K * M).to(torch.float32).contiguous()
    ch = torch.as_tensor(channels, dtype=torch.int32, device=scales.device).contiguous()
    out = torch.empty((ch.numel(), H, W, 2 * int(minmax) + 2), dtype=torch.int32, device=scales.device)
    d = L.GmmDesc(B, H * W, M, K, L.dt(scales), 0, K * M, 0, 0, float(scale_bound), 0.0)
    L.call("hesic_gmm_cdf", C.byref(d), int(b), L.ptr(scales), L.ptr(means), L.ptr(wts), L.ptr(ch), ch.numel(), int(minmax),
           L.ptr(out), L.stream())
    return out


# ------------------------------------------------------------------------------------ device-resident range coder
# include/hesic_codec.h (csrc/codec.hip): the bit-stream of HSIC.compress_batch / decompress_batch.  Of one VIEW of a batch, image b has
# its own alphabet (``minmax[b]``) and its own list of coded channels (``channels[b]``, ascending); stream (b, s) carries
# ``channels_per_stream`` consecutive coded channels.  Tables and symbols stay on the device.
def rc_check(minmax, channels, M):
    """Host-side refusal of what the coder's kernels cannot take (nothing is launched): alphabets beyond their LDS row, malformed channel
    lists.  Returns the normalised (minmax, channels) lists."""
    if len(minmax) != len(channels) or len(minmax) == 0:
        raise ValueError("device range coder: one minmax and one channel list per image")
    mms, chs = [], []
    for mm, ch in zip(minmax, channels):
        mm, ch = int(mm), [int(c) for c in ch]
        if mm < 1 or 2 * mm + 1 > L.CODEC_MAX_ALPHABET:
            raise ValueError(f"device range coder: an alphabet of 2 * {mm} + 1 symbols is outside its limit of {L.CODEC_MAX_ALPHABET} (one table "
                             "row per wave in LDS); code this pair with the per-pair HSIC.compress / decompress (HESIC+: HSICJoint.compress / "
                             "decompress), which have no such limit")
        if len(ch) > M or any(c < 0 or c >= M for c in ch) or any(a >= b for a, b in zip(ch, ch[1:])):
            raise ValueError(f"device range coder: the coded channels must be ascending indices in [0, {M})")
        mms.append(mm)
        chs.append(ch)
    return mms, chs


def rc_meta(minmax, channels, M, device):
    """The per-image header of one view as the kernels read it: int32 (B, M + 2) rows [n_coded, minmax, channel_0, ...], checked by
    ``rc_check`` first."""
    mms, chs = rc_check(minmax, channels, M)
    return torch.tensor([[len(ch), mm] + ch + [0] * (M - len(ch)) for mm, ch in zip(mms, chs)], dtype=torch.int32, device=device)


def _rc_args(scales, means, weights, K, scale_bound):
    L.require_cuda(scales, means)
    B, KM, H, W = scales.shape
    M = KM // K
    ps, sptr, mptr, keep = _sm_pointers(scales.detach(), means.detach(), scales, B, K, M)
    wts = None if weights is None else weights.detach().reshape(B, K * M).to(torch.float32).contiguous()
    d = L.GmmDesc(B, H * W, M, K, L.dt(scales), 0, ps, 0, 0, float(scale_bound), 0.0)
    return d, sptr, mptr, wts, keep, (B, M, H, W)


def _rc_streams(M, channels_per_stream):
    cps = int(channels_per_stream)
    if cps < 1 or cps > M:
        raise ValueError(f"channels_per_stream must be in [1, {M}], got {channels_per_stream}")
    return cps, (M + cps - 1) // cps


def gmm_rc_ranges(scales, means, weights, y_hat, minmax, channels, K, scale_bound=0.11, meta=None):
    """The coding interval of every coded latent: int32 (B, M, H, W, 3) with [j] = (c[s], c[s+1] - c[s], c[A]) of the symbol
    s = y_hat + minmax[b] of image b's j-th coded channel in the row ``gmm_cdf_tables`` forms for that element (bit for bit); rows
    j >= len(channels[b]) are not written."""
    d, sptr, mptr, wts, keep, (B, M, H, W) = _rc_args(scales, means, weights, K, scale_bound)
    L.require_cuda(y_hat)
    if y_hat.shape != (B, M, H, W):
        raise ValueError(f"gmm_rc_ranges: y_hat must be {(B, M, H, W)}, got {tuple(y_hat.shape)}")
    if meta is None:
        meta = rc_meta(minmax, channels, M, scales.device)
    y_hat = _nhwc(y_hat.detach())
    out = torch.empty((B, M, H, W, 3), dtype=torch.int32, device=scales.device)
    L.call("hesic_gmm_rc_ranges", C.byref(d), sptr, mptr, L.ptr(wts), L.ptr(y_hat), L.dt(y_hat), L.ptr(meta), L.ptr(out), L.stream())
    del keep
    return out


def gmm_rc_encode(scales, means, weights, y_hat, minmax, channels, K, channels_per_stream=1, scale_bound=0.11, order=None):
    """One view of a batch -> (bytes, counts): ``counts`` int32 (B, S), S = ceil(M / channels_per_stream), the byte length of every stream
    (0 beyond an image's coded channels), ``bytes`` uint8 the streams back to back in (b, s) order -- both on the device; what crosses
    to the host is the payload and the counts.  Raises if a stream overflowed its slot or a symbol had no frequency.
    ``order``: int32 (H * W) on the device, the raster index of the i-th pixel in coding order -- the HESIC+ stream (pixel-major, walked
    through that permutation; include/hesic_codec.h) instead of the channel-major HESIC stream."""
    B, KM, H, W = scales.shape
    M = KM // K
    cps, S = _rc_streams(M, channels_per_stream)
    meta = rc_meta(minmax, channels, M, scales.device)
    triples = gmm_rc_ranges(scales, means, weights, y_hat, minmax, channels, K, scale_bound, meta=meta)
    dev = scales.device
    cap = 4 * cps * H * W + 16
    slots = torch.empty((B * S, cap), dtype=torch.uint8, device=dev)
    counts = torch.empty((B, S), dtype=torch.int32, device=dev)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    if order is None:
        L.call("hesic_rc_encode_streams", L.ptr(triples), L.ptr(meta), B, M, H * W, cps, L.ptr(slots), cap, L.ptr(counts), L.ptr(status), L.stream())
    else:
        L.require_cuda(order)
        if order.dtype != torch.int32 or order.numel() != H * W or not order.is_contiguous():
            raise ValueError(f"gmm_rc_encode: order must be a contiguous int32 tensor of {H * W} pixels")
        L.call("hesic_rc_encode_streams_ordered", L.ptr(triples), L.ptr(meta), B, M, H * W, cps, L.ptr(order), L.ptr(slots), cap, L.ptr(counts),
               L.ptr(status), L.stream())
    offsets = torch.cumsum(counts.reshape(-1), 0, dtype=torch.int64)
    st, total = (int(v) for v in torch.stack([status[0].to(torch.int64), offsets[-1]]).cpu())
    if st:
        what = ["a stream overflowed its slot of 4 bytes per symbol + 16"] if st & L.CODEC_OVERFLOW else []
        what += ["a latent lies outside its image's alphabet (zero frequency)"] if st & L.CODEC_BAD_SYMBOL else []
        raise RuntimeError("gmm_rc_encode: " + " and ".join(what))
    offsets = offsets - counts.reshape(-1)
    out = torch.empty((total,), dtype=torch.uint8, device=dev)
    if total:
        L.call("hesic_rc_compact_streams", L.ptr(slots), cap, L.ptr(counts), L.ptr(offsets), B * S, L.ptr(out), total, L.stream())
    return out, counts


def gmm_rc_decode(scales, means, weights, minmax, channels, K, data, counts, out_dtype=None, channels_per_stream=1, scale_bound=0.11):
    """Inverse of ``gmm_rc_encode`` for one view: ``data`` uint8 (device) the streams back to back, ``counts`` (B, S) their lengths ->
    y_hat (B, M, H, W) channels-last in ``out_dtype`` (default: the compute dtype), unflagged channels zero.  Streams written by the host
    range coder over ``gmm_cdf_tables`` rows (8-byte termination) decode too."""
    d, sptr, mptr, wts, keep, (B, M, H, W) = _rc_args(scales, means, weights, K, scale_bound)
    cps, S = _rc_streams(M, channels_per_stream)
    dev = scales.device
    meta = rc_meta(minmax, channels, M, dev)
    L.require_cuda(data)
    if data.dtype != torch.uint8 or data.dim() != 1 or not data.is_contiguous():
        raise ValueError("gmm_rc_decode: data must be a contiguous 1-d uint8 tensor")
    counts = torch.as_tensor(counts, dtype=torch.int32, device=dev).contiguous()
    if counts.numel() != B * S:
        raise ValueError(f"gmm_rc_decode: {B * S} stream lengths expected, got {counts.numel()}")
    offsets = torch.cumsum(counts.reshape(-1), 0, dtype=torch.int64) - counts.reshape(-1)
    out_dtype = out_dtype or _compute_dtype
    y_hat = _empty_nhwc(B, M, H, W, out_dtype, dev)
    y_hat.zero_()                                   # the unflagged channels: one memset
    L.call("hesic_gmm_rc_decode", C.byref(d), sptr, mptr, L.ptr(wts), L.ptr(meta), cps, L.ptr(data), data.numel(), L.ptr(offsets), L.ptr(counts),
           L.ptr(y_hat), L.dt(out_dtype), L.stream())
    del keep
    return y_hat


def joint_gather_batch(y_rows, Wp, centre, rows, group_offset, P, crops, par, ext, e_off, feat):
    """One wavefront group of a batch of HESIC+ latent maps (``hesic_joint_gather_batch``): ``y_rows`` (B, rows, M) the padded maps,
    ``centre`` / ``rows`` int32 (HW) the padded and raster row of every pixel in coding order, ``par`` (B, HW, c_par), ``ext``
    (B, HW, M) or None -> ``crops`` (>= B * P, 25, M) and ``feat`` (>= B * P, c_feat), rows b * P + p."""
    B, n_rows, M = y_rows.shape
    L.require_cuda(y_rows, centre, rows, crops, par, ext, feat)
    HW = centre.numel()
    # the entry point sees pointers only: every size it relies on is checked here
    if (crops.shape[0] < B * P or crops.shape[1:] != (5, 5, M) or feat.dim() != 2 or feat.shape[0] < B * P or par.dim() != 3 or par.shape[:2] != (B, HW)
            or rows.numel() != HW or centre.dtype != torch.int32 or rows.dtype != torch.int32 or (ext is not None and ext.shape != (B, HW, M))):
        raise ValueError("joint_gather_batch: crops (>= B P, 5, 5, M), feat (>= B P, c_feat), par (B, HW, c_par), ext (B, HW, M), int32 centre / rows (HW) expected")
    if any(t is not None and (t.dtype != y_rows.dtype or not t.is_contiguous()) for t in (y_rows, crops, par, ext, feat)):
        raise ValueError("joint_gather_batch: the maps, crops, par, ext and feat must be contiguous tensors of one dtype")
    L.call("hesic_joint_gather_batch", L.ptr(y_rows), L.dt(y_rows), M, int(Wp), n_rows, L.ptr(centre), L.ptr(rows), int(group_offset), int(P),
           centre.numel(), B, L.ptr(crops), L.ptr(par), par.shape[2], L.ptr(ext), int(e_off), L.ptr(feat), feat.shape[1], L.stream())


def gmm_rc_decode_step(sm, B, P, M, meta, channels_per_stream, data, offsets, counts, state, first, centre, group_offset, y_rows, scale_bound=0.11):
    """The symbols of one wavefront group for every stream of a batch (``hesic_gmm_rc_decode_step``): ``sm`` fp32 (B * P, 2 M) rows
    [scales | means] of the entropy-parameter net, ``state`` int64 (B * S, 4) the coder states (begun here when ``first``), written as
    symbol - minmax into rows ``centre[group_offset + p]`` of the padded maps ``y_rows`` (B, rows, M)."""
    L.require_cuda(sm, meta, data, offsets, counts, state, centre, y_rows)
    cps, S = _rc_streams(M, channels_per_stream)
    if sm.dtype != torch.float32 or sm.numel() != B * P * 2 * M or not sm.is_contiguous():
        raise ValueError(f"gmm_rc_decode_step: sm must be contiguous fp32 ({B * P}, {2 * M}) rows")
    if (meta.shape != (B, M + 2) or meta.dtype != torch.int32 or offsets.numel() != B * S or offsets.dtype != torch.int64 or counts.numel() != B * S
            or counts.dtype != torch.int32 or state.numel() != B * S * 4 or state.dtype != torch.int64 or data.dtype != torch.uint8
            or centre.dtype != torch.int32 or y_rows.shape[0] != B or y_rows.shape[2] != M):
        raise ValueError("gmm_rc_decode_step: meta / offsets / counts / state / centre / y_rows do not fit the batch")
    d = L.GmmDesc(B, P, M, 1, L.F32, 0, 2 * M, 0, M, float(scale_bound), 0.0)
    L.call("hesic_gmm_rc_decode_step", C.byref(d), L.ptr(sm), L.ptr(sm), L.ptr(meta), cps, L.ptr(data), data.numel(), L.ptr(offsets), L.ptr(counts),
           L.ptr(state), int(bool(first)), L.ptr(centre), int(group_offset), centre.numel(), L.ptr(y_rows), L.dt(y_rows), y_rows.shape[1], L.stream())


# ----------------------------------------------------------------------------------- device rANS coder (include/hesic_rans.h)
_RANS_STATUS = ((L.RANS_OVERFLOW, "the stream overflowed its slot of 8 bytes per symbol + 16"),
                (L.RANS_BAD_TABLE, "a row index outside the table, a row size outside [2, row stride] or a zero frequency"),
                (L.RANS_BAD_ESCAPE, "an escape claims more than 8 data nibbles"),
                (L.RANS_BAD_STREAM, "the stream is shorter than 8 bytes, not whole 32-bit words or outside the payload"))


def rans_check_status(who, status):
    """``status``: the per-stream int32 words of a device rANS launch, already on the host (a list or tensor).  A non-zero word raises
    ``ValueError`` naming the first such stream."""
    for t, st in enumerate(status.tolist() if torch.is_tensor(status) else status):
        if st:
            raise ValueError(f"{who}: stream {t}: " + " and ".join(msg for bit, msg in _RANS_STATUS if st & bit))


def _rans_tables(who, table, lengths, offsets, indexes, dequant, B, n):
    L.require_cuda(table, lengths, offsets, indexes)
    if (table.dim() != 2 or any(t.dtype != torch.int32 or not t.is_contiguous() for t in (table, lengths, offsets))
            or lengths.numel() != table.shape[0] or offsets.numel() != table.shape[0]):
        raise ValueError(f"{who}: table (rows, stride), lengths (rows) and offsets (rows) must be contiguous int32 tensors")
    if table.shape[1] > L.RANS_MAX_ROW:
        raise ValueError(f"{who}: rows of {table.shape[1]} entries; the device coder holds a row in one wave's registers, up to {L.RANS_MAX_ROW}")
    istride = 0
    if indexes is not None:
        if indexes.dtype != torch.int32 or not indexes.is_contiguous() or indexes.numel() not in (n, B * n):
            raise ValueError(f"{who}: indexes must be a contiguous int32 tensor of {n} (shared) or {B * n} (per stream) entries in coding order")
        istride = n if indexes.numel() == B * n and B > 1 else 0
    med, zdt = None, None
    if dequant is not None:
        med, zdt = dequant
        L.require_cuda(med)
        med = med.detach().reshape(-1)
        if med.dtype != torch.float32 or med.numel() != table.shape[0] or not med.is_contiguous():
            raise ValueError(f"{who}: dequant = (medians, dtype) with one contiguous fp32 median per table row")
    return istride, med, zdt


def _rans_strides(t):
    """(B, n, P, (sb, sc, sp)) of a (B, n) / (B, C, P) / (B, C, H, W) tensor whose pixels lie at one stride (contiguous or channels-last)."""
    if t.dim() == 2:
        return t.shape[0], t.shape[1], t.shape[1], (t.stride(0), 0, t.stride(1))
    if t.dim() == 3:
        return t.shape[0], t.shape[1] * t.shape[2], t.shape[2], t.stride()
    if t.dim() == 4 and t.shape[3] == 1:             # a column: the stride of a size-1 dimension means nothing
        return t.shape[0], t.shape[1] * t.shape[2], t.shape[2], (t.stride(0), t.stride(1), t.stride(2))
    if t.dim() == 4 and (t.shape[2] == 1 or t.stride(2) == t.shape[3] * t.stride(3)):
        return t.shape[0], t.shape[1] * t.shape[2] * t.shape[3], t.shape[2] * t.shape[3], (t.stride(0), t.stride(1), t.stride(3))
    return None


def rans_encode_launch(symbols, table, lengths, offsets, indexes=None, dequant=None):
    """The launches of ``rans_encode`` without a synchronisation: (data, counts, status[, z_hat]) with ``data`` of the worst-case size --
    the streams lie back to back in its first ``counts.sum()`` bytes -- and ``status`` the per-stream int32 words for ``rans_check_status``."""
    L.require_cuda(symbols)
    if symbols.dtype != torch.int32 or symbols.dim() not in (2, 3, 4):
        raise ValueError("rans_encode: symbols must be an int32 (B, n), (B, C, P) or (B, C, H, W) tensor")
    geo = _rans_strides(symbols)
    if geo is None:
        symbols = symbols.contiguous()
        geo = _rans_strides(symbols)
    B, n, P, (sb, sc, sp) = geo
    if B < 1 or n < 1:
        raise ValueError("rans_encode: empty batch")
    istride, med, zdt = _rans_tables("rans_encode", table, lengths, offsets, indexes, dequant, B, n)
    z_hat = None
    if med is not None:
        # the kernel writes z_hat with the SYMBOLS' strides.  empty_like keeps them for a dense tensor only: for a sliced view (a channel
        # or column range of a larger map) it packs them, so such symbols are copied first and both tensors are dense
        def used(t):
            _, _, _, st = _rans_strides(t)
            return tuple(s_ for s_, k in zip(st, (B, n // P, P)) if k > 1)
        z_hat = torch.empty_like(symbols, dtype=zdt)
        if used(z_hat) != used(symbols):
            symbols = symbols.contiguous()
            _, _, _, (sb, sc, sp) = _rans_strides(symbols)
            z_hat = torch.empty_like(symbols, dtype=zdt)
            if used(z_hat) != used(symbols):
                raise RuntimeError("rans_encode: z_hat does not share the symbols' strides")
    dev = symbols.device
    slot = 8 * n + 16
    ws = torch.empty(((B * n * 9 + 7) // 8,), dtype=torch.int64, device=dev)
    slots = torch.empty((B, slot), dtype=torch.uint8, device=dev)
    counts = torch.empty((B,), dtype=torch.int32, device=dev)
    status = torch.empty((B,), dtype=torch.int32, device=dev)
    L.call("hesic_rans_encode", L.ptr(symbols), sb, sc, sp, B, n, P, L.ptr(indexes), istride, L.ptr(table), table.shape[0], table.shape[1],
           L.ptr(lengths), L.ptr(offsets), L.ptr(ws), ws.numel() * 8, L.ptr(slots), slot, L.ptr(counts), L.ptr(status), L.ptr(med), L.ptr(z_hat),
           L.F32 if z_hat is None else L.dt(z_hat), L.stream())
    out_offsets = torch.cumsum(counts, 0, dtype=torch.int64) - counts
    data = torch.empty((B * slot,), dtype=torch.uint8, device=dev)
    L.call("hesic_rans_compact", L.ptr(slots), slot, L.ptr(counts), L.ptr(out_offsets), B, L.ptr(data), data.numel(), L.stream())
    return (data, counts, status) if z_hat is None else (data, counts, status, z_hat)


def rans_encode(symbols, table, lengths, offsets, indexes=None, dequant=None):
    """A batch of independent rANS streams on the device (``hesic_rans_encode``), each byte for byte ``_host.rans_encode_arrays`` of its
    symbols: ``symbols`` int32 (B, n), (B, C, P) or (B, C, H, W), contiguous or channels-last (read in place), stream b = symbols[b] in
    (C, P) order; ``table`` / ``lengths`` / ``offsets`` the int32 ``_quantized_cdf`` (rows, stride), ``_cdf_length`` and ``_offset``;
    ``indexes`` None -- the row of a symbol is its channel (row 0 for a (B, n) tensor) -- or int32 rows in coding order, n entries shared
    by the batch or B * n per stream; ``dequant`` = (medians fp32 (rows), dtype) also returns z_hat = (symbols + medians[row]).to(dtype) in
    the symbols' layout.  -> (data uint8 the streams back to back, counts int32 (B)[, z_hat]), all on the device.  A non-zero status
    raises ``ValueError`` naming the stream."""
    data, counts, status, *z = rans_encode_launch(symbols, table, lengths, offsets, indexes, dequant)
    host = torch.cat([status, counts]).cpu()
    B = counts.numel()
    rans_check_status("rans_encode", host[:B])
    return (data[:int(host[B:].sum())], counts, *z)


def rans_decode(data, counts, n, table, lengths, offsets, indexes=None, dequant=None, want_symbols=None, check=True):
    """Inverse of ``rans_encode`` (``hesic_rans_decode``): ``data`` uint8 (device) the streams back to back, ``counts`` their B lengths, ``n``
    the symbols per stream as an int (-> (B, n)), (C, P) (-> (B, C, P)) or (C, H, W) (-> (B, C, H, W) channels-last).  Returns the int32
    symbols, or with ``dequant`` = (medians, dtype) z_hat = (symbols + medians[row]).to(dtype) (``want_symbols=True``: both).  A word past
    a stream's end reads as zero, as the host decoder's.  ``check=False`` skips the synchronising status check and returns
    (result, status) for ``rans_check_status``."""
    L.require_cuda(data)
    if data.dtype != torch.uint8 or data.dim() != 1 or not data.is_contiguous():
        raise ValueError("rans_decode: data must be a contiguous 1-d uint8 tensor")
    if data.data_ptr() % 4:
        data = data.clone()
    dev = data.device
    counts = torch.as_tensor(counts, dtype=torch.int32, device=dev).reshape(-1).contiguous()
    B = counts.numel()
    shape = (int(n),) if isinstance(n, int) else tuple(int(v) for v in n)
    if B < 1 or len(shape) not in (1, 2, 3) or any(v < 1 for v in shape):
        raise ValueError("rans_decode: n must be an int, (C, P) or (C, H, W), and counts non-empty")
    want_symbols = dequant is None if want_symbols is None else bool(want_symbols)
    if not want_symbols and dequant is None:
        raise ValueError("rans_decode: nothing to return")
    fmt = _CL if len(shape) == 3 else torch.contiguous_format
    like = torch.empty((B,) + shape, dtype=torch.int32, device=dev, memory_format=fmt) if want_symbols else None
    nsym = 1
    for v in shape:
        nsym *= v
    istride, med, zdt = _rans_tables("rans_decode", table, lengths, offsets, indexes, dequant, B, nsym)
    z_hat = None if med is None else torch.empty((B,) + shape, dtype=zdt, device=dev, memory_format=fmt)
    _, _, P, (sb, sc, sp) = _rans_strides(like if like is not None else z_hat)
    status = torch.empty((B,), dtype=torch.int32, device=dev)
    data_offsets = torch.cumsum(counts, 0, dtype=torch.int64) - counts
    L.call("hesic_rans_decode", L.ptr(data), data.numel(), L.ptr(data_offsets), L.ptr(counts), B, nsym, P, L.ptr(indexes), istride, L.ptr(table),
           table.shape[0], table.shape[1], L.ptr(lengths), L.ptr(offsets), L.ptr(like), sb, sc, sp, L.ptr(med), L.ptr(z_hat),
           L.F32 if z_hat is None else L.dt(z_hat), L.ptr(status), L.stream())
    out = like if z_hat is None else (z_hat if like is None else (like, z_hat))
    if not check:
        return out, status
    rans_check_status("rans_decode", status.cpu())
    return out


def quantize_symbols(y, means=None):
    """EntropyModel._quantize(x, 'symbols', means) (entropy_models.py:98-125): int32 indices."""
    L.require_cuda(y)
    B, M, H, W = y.shape
    y = _nhwc(y)
    sc = torch.ones_like(y, memory_format=_CL)
    mu = torch.empty_like(y, memory_format=_CL).fill_(0) if means is None else _nhwc(means.to(y.dtype).expand_as(y))
    yh = torch.empty_like(y, memory_format=_CL)
    lik = _empty_nhwc(B, M, H, W, torch.float32, y.device)
    sym = torch.empty((B, M, H, W), dtype=torch.int32, device=y.device).contiguous(memory_format=_CL)
    d = L.GmmDesc(B, H * W, M, 1, L.dt(y), int(means is not None), M, 0, 0, 0.11, 1e-9)
    L.call("hesic_gmm_forward", C.byref(d), L.ptr(y), L.ptr(sc), L.ptr(mu), None, None, L.ptr(yh), L.ptr(lik), L.ptr(sym),
           L.stream())
    return sym


# ----------------------------------------------------------------------------------- glue
class _Upsample4CatFn(torch.autograd.Function):
    """cat(UpsamplingBilinear2d(x4)(z), y1, dim=1) (newnet1.py:524,556-557) in one buffer."""

    @staticmethod
    def forward(ctx, z, y1):
        L.require_cuda(z, y1)
        B, Cz, H, W = z.shape
        _, Cy, Hy, Wy = y1.shape
        if (Hy, Wy) != (4 * H, 4 * W):
            raise RuntimeError("upsample4_cat: y1 must be 4x the size of z")
        z, y1 = _nhwc(z), _nhwc(y1.to(z.dtype))
        out = _empty_nhwc(B, Cz + Cy, Hy, Wy, z.dtype, z.device)
        L.call("hesic_upsample4_forward", L.ptr(z), L.ptr(out), B, H, W, Cz, Cz + Cy, 0, L.dt(z), L.stream())
        L.call("hesic_copy_channels", L.ptr(y1), L.ptr(out), B * Hy * Wy, Cy, Cy, 0, Cz + Cy, Cz, L.dt(z), L.stream())
        ctx.dims = (B, Cz, H, W, Cy)
        return out

    @staticmethod
    def backward(ctx, g):
        B, Cz, H, W, Cy = ctx.dims
        g = _nhwc(g)
        dz = _empty_nhwc(B, Cz, H, W, g.dtype, g.device)
        dy1 = _empty_nhwc(B, Cy, 4 * H, 4 * W, g.dtype, g.device)
        L.call("hesic_upsample4_backward", L.ptr(g), L.ptr(dz), B, H, W, Cz, Cz + Cy, 0, L.dt(g), L.stream())
        L.call("hesic_copy_channels", L.ptr(g), L.ptr(dy1), B * 16 * H * W, Cy, Cz + Cy, Cz, Cy, 0, L.dt(g), L.stream())
        return dz, dy1


def upsample4_cat(z, y1):
    return _apply(_Upsample4CatFn, z, y1)


class _Upsample4Fn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, z):
        L.require_cuda(z)
        B, Cz, H, W = z.shape
        z = _nhwc(z)
        out = _empty_nhwc(B, Cz, 4 * H, 4 * W, z.dtype, z.device)
        L.call("hesic_upsample4_forward", L.ptr(z), L.ptr(out), B, H, W, Cz, Cz, 0, L.dt(z), L.stream())
        ctx.dims = (B, Cz, H, W)
        return out

    @staticmethod
    def backward(ctx, g):
        B, Cz, H, W = ctx.dims
        g = _nhwc(g)
        dz = _empty_nhwc(B, Cz, H, W, g.dtype, g.device)
        L.call("hesic_upsample4_backward", L.ptr(g), L.ptr(dz), B, H, W, Cz, Cz, 0, L.dt(g), L.stream())
        return dz


def upsample4(z):
    return _apply(_Upsample4Fn, z)


class _SpatialMaxFn(torch.autograd.Function):
    """spatial_pool2d (newnet1.py:441-453) [+ LeakyReLU :497]: (B,C,H,W) -> (B,C,1,1) fp32."""

    @staticmethod
    def forward(ctx, x, leaky):
        L.require_cuda(x)
        B, Cc, H, W = x.shape
        x = _nhwc(x)
        out = torch.empty((B, Cc), dtype=torch.float32, device=x.device)
        need_arg = ctx.needs_input_grad[0]                          # the arg-max is only needed by the backward
        arg = torch.empty((B, Cc), dtype=torch.int32, device=x.device) if need_arg else None
        L.call("hesic_spatial_max", L.ptr(x), L.ptr(out), L.ptr(arg), B, H * W, Cc, L.dt(x), int(leaky), L.stream())
        ctx.save_for_backward(arg, out)
        ctx.meta = (x.shape, x.dtype, leaky)
        return out.reshape(B, Cc, 1, 1)

    @staticmethod
    def backward(ctx, g):
        arg, out = ctx.saved_tensors
        shape, dtype, leaky = ctx.meta
        B, Cc, H, W = shape
        g = g.reshape(B, Cc)
        if g.dtype != torch.float32 or not g.is_contiguous():
            g = g.to(torch.float32).contiguous()
        dx = torch.empty((B, H * W, Cc), dtype=dtype, device=g.device)
        L.call("hesic_spatial_max_backward", L.ptr(g), L.ptr(out), L.ptr(arg), L.ptr(dx), B, H * W, Cc, L.dt(dtype), int(leaky), L.stream())
        return dx.reshape(B, H, W, Cc).permute(0, 3, 1, 2), None


def spatial_max(x, leaky=False):
    return _apply(_SpatialMaxFn, x, leaky)


class _SoftmaxKFn(torch.autograd.Function):
    """softmax over K of a (B, K*M, 1, 1) tensor with channel k*M+m (newnet1.py:510-512)."""

    @staticmethod
    def forward(ctx, logits, K, M):
        L.require_cuda(logits)
        B = logits.shape[0]
        lg = logits.reshape(B, K * M).to(torch.float32).contiguous()
        w = torch.empty_like(lg)
        L.call("hesic_softmax_k_forward", L.ptr(lg), L.ptr(w), B, K, M, L.stream())
        ctx.save_for_backward(w)
        ctx.meta = (K, M, logits.dtype, logits.shape)
        return w.reshape(B, K * M, 1, 1)

    @staticmethod
    def backward(ctx, g):
        (w,) = ctx.saved_tensors
        K, M, dtype, shape = ctx.meta
        B = w.shape[0]
        g = g.reshape(B, K * M).to(torch.float32).contiguous()
        dl = torch.empty_like(w)
        L.call("hesic_softmax_k_backward", L.ptr(w), L.ptr(g), L.ptr(dl), B, K, M, L.stream())
        return dl.reshape(shape).to(dtype), None, None


def softmax_k(logits, K, M):
    return _apply(_SoftmaxKFn, logits, K, M)


class _PooledLinearFn(torch.autograd.Function):
    """conv1x1(N -> N) on a pooled (B, N, 1, 1) vector (newnet1.py:500) under autograd: three small launches instead of
    the conv tile pipeline (forward + dgrad + wgrad + colsum + reduce on 8 "pixels" cost ~0.4 ms per training step)."""

    @staticmethod
    def forward(ctx, pooled, weight, bias):
        L.require_cuda(pooled, weight)
        B, N = pooled.shape[0], pooled.shape[1]
        p = pooled.reshape(B, N).to(torch.float32).contiguous()
        w = weight.detach().reshape(N, N).to(torch.float32).contiguous()
        out = torch.empty((B, N), dtype=torch.float32, device=p.device)
        L.call("hesic_pooled_linear_forward", L.ptr(p), L.ptr(w), L.ptr(None if bias is None else bias.detach().float()), L.ptr(out),
               B, N, L.stream())
        ctx.save_for_backward(p, w)
        ctx.weight, ctx.bias = weight, bias
        ctx.meta = (pooled.dtype, weight.dtype, weight.shape, bias is not None, None if bias is None else bias.dtype)
        return out.reshape(B, N, 1, 1)

    @staticmethod
    def backward(ctx, g):
        p, w = ctx.saved_tensors
        pdt, wdt, wshape, has_b, bdt = ctx.meta
        B, N = p.shape
        g = g.reshape(B, N).to(torch.float32).contiguous()
        need_p, need_w, need_b = ctx.needs_input_grad
        dp = torch.empty_like(p) if need_p else None
        # flat gradient slots: the kernel overwrites, so it writes the (cleared, still untouched) slots themselves
        ws_, bs_ = _slot_for(ctx.weight), (_slot_for(ctx.bias) if has_b else None)
        direct = need_w and ws_ is not None and ws_.writes == 0 and (not has_b or (bs_ is not None and bs_.writes == 0))
        if direct:
            dw, db = ws_.grad, (bs_.grad if has_b else None)
        else:
            dw = torch.empty((N, N), dtype=torch.float32, device=p.device) if (need_w or (need_b and has_b)) else None
            db = torch.empty(N, dtype=torch.float32, device=p.device) if (need_b and has_b) else None
        L.call("hesic_pooled_linear_backward", L.ptr(p), L.ptr(w), L.ptr(g), L.ptr(dp), L.ptr(dw), L.ptr(db), B, N, L.stream())
        if direct:
            _slot_done(ws_)
            if has_b:
                _slot_done(bs_)
            return (None if dp is None else dp.reshape(B, N, 1, 1).to(pdt), None, None)
        return (None if dp is None else dp.reshape(B, N, 1, 1).to(pdt), dw.reshape(wshape).to(wdt) if need_w else None,
                None if db is None else db.to(bdt))


def pooled_linear(pooled, weight, bias):
    return _apply(_PooledLinearFn, pooled, weight, bias)


def mix_weights(pooled, weight, bias, K, M):
    """conv1x1(K*M -> K*M) on the pooled vector + softmax over K (newnet1.py:500,510-512).
    Forward-only HIP kernel; under autograd the caller uses the differentiable torch fallback
    below because the op is 0.001 GMAC."""
    L.require_cuda(pooled, weight)
    B = pooled.shape[0]
    p = pooled.reshape(B, K * M).to(torch.float32).contiguous()
    w = weight.detach().reshape(K * M, K * M).to(torch.float32).contiguous()
    logits = torch.empty((B, K * M), dtype=torch.float32, device=p.device)
    out = torch.empty((B, K * M), dtype=torch.float32, device=p.device)
    L.call("hesic_mix_weights_forward", L.ptr(p), L.ptr(w), L.ptr(None if bias is None else bias.detach()), L.ptr(logits),
           L.ptr(out), B, K, M, L.stream())
    return out.reshape(B, K * M, 1, 1)


# ----------------------------------------------------------------------------- reductions
RD_SUMS_FUSED = True       # module switch: False = one launch per likelihood map / image pair (rounds 1-4)


def sum_log2(lik, out=None):
    """sum(log2(lik)) as an fp64 device scalar (bits = -sum)."""
    L.require_cuda(lik)
    lik = lik.contiguous() if not lik.is_contiguous(memory_format=_CL) else lik
    if out is None:
        out = _zeros(1, torch.float64, lik.device)
    L.call("hesic_sum_log2", L.ptr(lik), lik.numel(), L.ptr(out), L.stream())
    return out


def sum_sq_diff(a, b, out=None):
    L.require_cuda(a, b)
    B, Cc, H, W = a.shape
    if out is None:
        out = _zeros(1, torch.float64, a.device)
    sa = (C.c_int64 * 4)(*a.stride())
    sb = (C.c_int64 * 4)(*b.stride())
    L.call("hesic_sum_sq_diff", L.ptr(a), L.dt(a), sa, L.ptr(b), L.dt(b), sb, B, Cc, H, W, L.ptr(out), L.stream())
    return out


def rd_sums(liks, lik_outs, pairs, sq_outs):
    """sum(log2(lik_i)) into ``lik_outs[i]`` and sum((a - b)^2) of the image pairs into ``sq_outs[i]`` -- every reduction behind one forward's
    bpp / PSNR in ONE launch (``hesic_rd_sums``; four + two launches before).  The accumulators are added to (zero-fill them first)."""
    L.require_cuda(*liks, *[t for p in pairs for t in p])
    liks = [l if (l.is_contiguous() or l.is_contiguous(memory_format=_CL)) else l.contiguous() for l in liks]
    nl, ns = len(liks), len(pairs)
    vpl, i64l = C.c_void_p * max(nl, 1), C.c_int64 * max(nl, 1)
    vps, i32s, i64s, i32d = C.c_void_p * max(ns, 1), C.c_int32 * max(ns, 1), C.c_int64 * (4 * max(ns, 1)), C.c_int32 * (4 * max(ns, 1))
    sa, sb, dims = [], [], []
    for a, b in pairs:
        sa += list(a.stride()); sb += list(b.stride()); dims += list(a.shape)
    L.call("hesic_rd_sums", nl, vpl(*[l.data_ptr() for l in liks]), i64l(*[l.numel() for l in liks]), vpl(*[o.data_ptr() for o in lik_outs]),
           ns, vps(*[a.data_ptr() for a, _ in pairs]), i32s(*[L.dt(a) for a, _ in pairs]), i64s(*sa), vps(*[b.data_ptr() for _, b in pairs]),
           i32s(*[L.dt(b) for _, b in pairs]), i64s(*sb), i32d(*dims), vps(*[o.data_ptr() for o in sq_outs]), L.stream())


def pair_metrics(liks, pairs, out=None, ws=None):
    """The sums behind bpp / PSNR PER PAIR of a batch (``hesic_pair_metrics``, include/hesic_pair_metrics.h): a ``(B, len(liks) + 4)`` fp64
    table whose row b holds sum(log2(lik_i)) over image b's slice of every likelihood map, then sse1, sse2 (sum((a - b)^2) of
    ``pairs = [(x1_hat, x1), (x2_hat, x2)]`` over image b) and sse8_1, sse8_2 (the same on the 8-bit images ``codec.quantise`` writes).
    Two launches, no atomics, no zero-fill: the table is written, and a pair's row has the same bits in every batch and at every position.
    ``liks``: fp32 maps with the batch outermost (made contiguous only when neither dense nor channels-last); ``pairs``: (B, C, H, W)
    tensors of any strides, fp32 or the active 16-bit format.  ``out`` / ``ws``: a preallocated table / workspace (uint8, 8-byte aligned)."""
    if len(pairs) != 2:
        raise ValueError("pair_metrics: two image pairs, (x1_hat, x1) and (x2_hat, x2)")
    L.require_cuda(*liks, *[t for p in pairs for t in p])
    B, Cc, H, W = pairs[0][0].shape
    for t in (t for p in pairs for t in p):
        if tuple(t.shape) != (B, Cc, H, W):
            raise ValueError(f"pair_metrics: the four images must share one shape, got {tuple(t.shape)} and {(B, Cc, H, W)}")
    nl = len(liks)
    if nl > L.PAIR_METRICS_MAX_LIK:
        raise ValueError(f"pair_metrics: at most {L.PAIR_METRICS_MAX_LIK} likelihood maps, got {nl}")
    for l in liks:
        if l.dtype != torch.float32 or l.dim() < 1 or l.shape[0] != B:
            raise ValueError(f"pair_metrics: likelihood maps are fp32 with the batch of {B} outermost, got {l.dtype} {tuple(l.shape)}")
    liks = [l if (l.is_contiguous() or (l.dim() == 4 and l.is_contiguous(memory_format=_CL))) else l.contiguous() for l in liks]
    dev = pairs[0][0].device
    numel = (C.c_int64 * max(nl, 1))(*[l.numel() for l in liks])
    need = L.lib().hesic_pair_metrics_ws_bytes(B, nl, numel, H, W)
    if need < 0:
        raise RuntimeError(f"hesic_pair_metrics_ws_bytes failed: {L.lib().hesic_last_error().decode()}")
    if ws is None:
        ws = torch.empty(need, dtype=torch.uint8, device=dev)
    if out is None:
        out = torch.empty((B, nl + 4), dtype=torch.float64, device=dev)
    elif tuple(out.shape) != (B, nl + 4) or out.dtype != torch.float64 or not out.is_contiguous():
        raise ValueError(f"pair_metrics: out must be a dense fp64 {(B, nl + 4)} tensor")
    L.require_cuda(out, ws)
    vps, i32s, i64s = C.c_void_p * 2, C.c_int32 * 2, C.c_int64 * 8
    sa, sb = [], []
    for a, b in pairs:
        sa += list(a.stride()); sb += list(b.stride())
    L.call("hesic_pair_metrics", B, nl, (C.c_void_p * max(nl, 1))(*[l.data_ptr() for l in liks]), numel,
           vps(*[a.data_ptr() for a, _ in pairs]), i32s(*[L.dt(a) for a, _ in pairs]), i64s(*sa),
           vps(*[b.data_ptr() for _, b in pairs]), i32s(*[L.dt(b) for _, b in pairs]), i64s(*sb), Cc, H, W, L.ptr(out), L.ptr(ws),
           ws.numel() * ws.element_size(), L.stream())
    return out


class _RdLossFn(torch.autograd.Function):
    """RateDistortionLoss (ywz/mywork/newtrain1.py:37-56) as two kinds of HIP reductions:
    loss = lmbda*255^2*(MSE1+MSE2) + sum_t sum(log lik_t)/(-ln2 * B*H*W).  Returns (loss, bpp, mse)."""

    @staticmethod
    def forward(ctx, lmbda, x1, x2, x1_hat, x2_hat, *liks):
        import math
        B, Cc, H, W = x1.shape
        npix = B * H * W
        acc = _zeros(3, torch.float64, x1.device)
        liks = tuple(l if (l.is_contiguous() or l.is_contiguous(memory_format=_CL)) else l.contiguous() for l in liks)
        if x1.is_cuda and RD_SUMS_FUSED and len(liks) <= 8:
            rd_sums(liks, [acc[0:1]] * len(liks), [(x1_hat, x1), (x2_hat, x2)], [acc[1:2], acc[2:3]])
        else:
            for l in liks:
                sum_log2(l, acc[0:1])
            sum_sq_diff(x1_hat, x1, acc[1:2])
            sum_sq_diff(x2_hat, x2, acc[2:3])
        if x1.is_cuda:
            out3 = torch.empty(3, dtype=torch.float32, device=x1.device)
            L.call("hesic_rd_loss_combine", L.ptr(acc), float(lmbda) * 255.0 ** 2, npix, B * Cc * H * W, L.ptr(out3), L.stream())
            loss, bpp, mse = out3[0], out3[1], out3[2]
        else:
            bpp = -acc[0] / npix
            mse = (acc[1] + acc[2]) / (B * Cc * H * W)
            loss = (lmbda * 255.0 ** 2 * mse + bpp).float()
            bpp, mse = bpp.float(), mse.float()
        ctx.save_for_backward(x1, x2, x1_hat, x2_hat, *liks)
        ctx.meta = (float(lmbda), npix, B * Cc * H * W, -1.0 / (math.log(2.0) * npix))
        ctx.mark_non_differentiable(bpp, mse)        # reported values (the reference logs them); only `loss` carries a gradient
        return loss, bpp, mse

    @staticmethod
    def backward(ctx, g_loss, g_bpp, g_mse):
        x1, x2, x1_hat, x2_hat, *liks = ctx.saved_tensors
        lmbda, npix, numel, lik_scale = ctx.meta
        # g_loss stays on the device (reading it would be a host sync): the kernels compute the gradient of the unscaled loss
        # and, unless SCALED_LOSS is off, one multiply per gradient applies g_loss (loss / accum_steps, loss scaling, ...).
        # Trainer.step calls loss.backward() on the unscaled root and switches the multiplies off.
        g = 1.0
        B, Cc, H, W = x1.shape
        grads = []
        for xh, x in ((x1_hat, x1), (x2_hat, x2)):
            gx = torch.empty((B, Cc, H, W), dtype=torch.float32, device=x.device)
            sa, sb = (C.c_int64 * 4)(*xh.stride()), (C.c_int64 * 4)(*x.stride())
            L.call("hesic_sq_diff_backward", L.ptr(xh), L.dt(xh), sa, L.ptr(x), L.dt(x), sb, B, Cc, H, W,
                   g * lmbda * 255.0 ** 2 * 2.0 / numel, L.ptr(gx), L.stream())
            grads.append(gx)
        gl = []
        for l in liks:
            o = torch.empty_like(l)
            L.call("hesic_log_backward", L.ptr(l), g * lik_scale, L.ptr(o), l.numel(), L.stream())
            gl.append(o)
        if SCALED_LOSS:
            grads = [t.mul_(g_loss) for t in grads]
            gl = [t.mul_(g_loss) for t in gl]
        return (None, None, None, grads[0], grads[1], *gl)


SCALED_LOSS = True      # False (Trainer.step): loss.backward() is called on the unscaled loss, skip the six g_loss multiplies


# ----------------------------------------------------------------------------- MS-SSIM as a training loss
MS_SSIM_WEIGHTS = (0.0448, 0.2856, 0.3001, 0.2363, 0.1333)
DISTORTIONS = ("mse", "ms-ssim")
_ms_consts = {}


def _ms_const(values, device):
    """A small fp64 device constant (per-scale counts, exponents), built by fill kernels and kept: no host-to-device copy, so a step that
    meets a new image size while it is being captured into a graph stays capturable."""
    key = (tuple(values), device)
    t = _ms_consts.get(key)
    if t is None:
        t = torch.empty(len(values), dtype=torch.float64, device=device)
        for i, v in enumerate(values):
            t[i:i + 1].fill_(float(v))
        if not torch.cuda.is_current_stream_capturing():      # a tensor made during a capture lives in that graph's memory pool
            _ms_consts[key] = t
    return t


def _ms_ssim_check(x_hat, x):
    if x_hat.shape != x.shape or x.dim() != 4:
        raise ValueError("ms_ssim: two (N, C, H, W) tensors of the same shape")
    if min(x.shape[-2:]) <= 160:
        raise ValueError("ms_ssim: the smaller image side must exceed (11 - 1) * 2^4 = 160")


def _ms_ssim_forward(a, b, data_range):
    """The launches and the arithmetic of ``models.ms_ssim`` on fp32 images ``a`` (reconstruction) and ``b`` (target); returns the (N,) fp64
    value, the fp64 sums (5, B, C, 2), the images of the five scales [(a, b)] and the valid positions per scale."""
    B, Cc, H, W = a.shape
    sums = torch.empty((5, B, Cc, 2), dtype=torch.float64, device=a.device).fill_(0)
    counts, pyramid = [], []
    for lvl in range(5):
        sa, sb = (C.c_int64 * 4)(*a.stride()), (C.c_int64 * 4)(*b.stride())
        L.call("hesic_ssim_scale", L.ptr(a), sa, L.ptr(b), sb, B, Cc, H, W, float(data_range), L.ptr(sums[lvl]), L.stream())
        counts.append((H - 10) * (W - 10))
        pyramid.append((a, b))
        if lvl < 4:
            Ho, Wo = (H + 2 * (H % 2) - 2) // 2 + 1, (W + 2 * (W % 2) - 2) // 2 + 1
            na, nb = (torch.empty((B, Cc, Ho, Wo), dtype=torch.float32, device=a.device) for _ in range(2))
            L.call("hesic_avgpool2_pad", L.ptr(a), sa, L.ptr(na), B, Cc, H, W, L.stream())
            L.call("hesic_avgpool2_pad", L.ptr(b), sb, L.ptr(nb), B, Cc, H, W, L.stream())
            a, b, H, W = na, nb, Ho, Wo
    means = sums / _ms_const(counts, sums.device).reshape(5, 1, 1, 1)
    v = torch.cat((means[:4, :, :, 1], means[4:, :, :, 0]), 0).clamp_min(0)                 # cs of scales 1-4, ssim of scale 5
    w = _ms_const(MS_SSIM_WEIGHTS, sums.device).reshape(5, 1, 1)
    return torch.prod(v ** w, 0).mean(1), sums, pyramid, counts


def _ms_ssim_backward(pyramid, sums, counts, grad_out, data_range):
    """d(sum_n grad_out[n] MS[n]) / d x_hat: five launches of ``hesic_ssim_scale_backward`` from the coarsest scale to the finest, each
    adding 0.25 x the coarser gradient of a pixel's pool cell.  ``grad_out``: (N,) fp64 on the device.  Contiguous fp32 result."""
    cnt, wts = (C.c_int64 * 5)(*counts), (C.c_double * 5)(*MS_SSIM_WEIGHTS)
    grad_out = grad_out.contiguous()
    g = None
    for lvl in range(4, -1, -1):
        a, b = pyramid[lvl]
        B, Cc, H, W = a.shape
        gx = torch.empty((B, Cc, H, W), dtype=torch.float32, device=a.device)
        L.call("hesic_ssim_scale_backward", L.ptr(a), (C.c_int64 * 4)(*a.stride()), L.ptr(b), (C.c_int64 * 4)(*b.stride()), B, Cc, H, W,
               float(data_range), L.ptr(sums), cnt, wts, 5, lvl, L.ptr(grad_out), L.ptr(g), L.ptr(gx), L.stream())
        g = gx
    return g


class _MsSsimFn(torch.autograd.Function):
    """``ms_ssim`` with a gradient for the reconstruction (the target is a constant): keeps the pooled images of scales 2-5 and the fp64 sums."""

    @staticmethod
    def forward(ctx, x_hat, x, data_range):
        a, b = (t if t.dtype == torch.float32 else t.float() for t in (x_hat, x))
        val, sums, pyramid, counts = _ms_ssim_forward(a, b, data_range)
        ctx.save_for_backward(sums, *[t for pair in pyramid for t in pair])
        ctx.meta = (counts, float(data_range))
        return val

    @staticmethod
    def backward(ctx, g_val):
        sums, *flat = ctx.saved_tensors
        counts, data_range = ctx.meta
        pyramid = [(flat[2 * i], flat[2 * i + 1]) for i in range(5)]
        return _ms_ssim_backward(pyramid, sums, counts, g_val.to(torch.float64), data_range), None, None


def ms_ssim(x_hat, x, data_range=1.0):
    """``models.ms_ssim`` (same launches, same (N,) fp64 values) as a differentiable function of ``x_hat``: the backward is five launches of
    ``hesic_ssim_scale_backward`` (csrc/msssim.hip) and returns an fp32 gradient of ``x_hat``'s shape; ``x`` is a constant.  Where a
    per-scale mean is <= 0 the definition clamps it: that image's value and gradient are 0.  16-bit images are cast to fp32 first."""
    L.require_cuda(x_hat, x)
    _ms_ssim_check(x_hat, x)
    return _apply(_MsSsimFn, x_hat, x, data_range)


class _RdMsSsimLossFn(torch.autograd.Function):
    """The R-D criterion with MS-SSIM as the distortion: loss = lmbda * ((1 - mean_n MS(x1_hat, x1)) + (1 - mean_n MS(x2_hat, x2))) + bpp --
    no 255^2 factor, reconstructions not clamped.  Returns (loss, bpp, mse, ms_ssim_loss); the MSE is still reported (the fused reduction
    behind bpp computes it anyway).  Gradients: the likelihoods' as in ``_RdLossFn``, the reconstructions' from ``hesic_ssim_scale_backward``
    with grad_out = -lmbda / N per image."""

    @staticmethod
    def forward(ctx, lmbda, x1, x2, x1_hat, x2_hat, *liks):
        import math
        B, Cc, H, W = x1.shape
        npix = B * H * W
        acc = _zeros(3, torch.float64, x1.device)
        liks = tuple(l if (l.is_contiguous() or l.is_contiguous(memory_format=_CL)) else l.contiguous() for l in liks)
        if RD_SUMS_FUSED and len(liks) <= 8:
            rd_sums(liks, [acc[0:1]] * len(liks), [(x1_hat, x1), (x2_hat, x2)], [acc[1:2], acc[2:3]])
        else:
            for l in liks:
                sum_log2(l, acc[0:1])
            sum_sq_diff(x1_hat, x1, acc[1:2])
            sum_sq_diff(x2_hat, x2, acc[2:3])
        out3 = torch.empty(3, dtype=torch.float32, device=x1.device)
        L.call("hesic_rd_loss_combine", L.ptr(acc), 0.0, npix, B * Cc * H * W, L.ptr(out3), L.stream())      # lambda 0: (bpp, bpp, mse)
        saved, metas, msl = [], [], None
        for xh, x in ((x1_hat, x1), (x2_hat, x2)):
            a, b = (t if t.dtype == torch.float32 else t.float() for t in (xh, x))
            val, sums, pyramid, counts = _ms_ssim_forward(a, b, 1.0)
            d = 1.0 - val.mean()
            msl = d if msl is None else msl + d
            saved += [sums, *[t for pair in pyramid for t in pair]]
            metas.append(counts)
        loss = (float(lmbda) * msl).float() + out3[1]
        ctx.save_for_backward(*saved, *liks)
        ctx.meta = (float(lmbda), B, metas, -1.0 / (math.log(2.0) * npix))
        bpp, mse, msl = out3[1], out3[2], msl.float()
        ctx.mark_non_differentiable(bpp, mse, msl)
        return loss, bpp, mse, msl

    @staticmethod
    def backward(ctx, g_loss, g_bpp, g_mse, g_msl):
        lmbda, B, metas, lik_scale = ctx.meta
        saved = ctx.saved_tensors
        liks = saved[22:]
        # as in _RdLossFn: g_loss stays on the device and is applied only when SCALED_LOSS is on -- here to the B values of grad_out
        # instead of the gradient images
        go = torch.empty(B, dtype=torch.float64, device=g_loss.device).fill_(-lmbda / B)
        if SCALED_LOSS:
            go = go.mul_(g_loss)
        grads = []
        for v in range(2):
            sums, *flat = saved[11 * v:11 * v + 11]
            grads.append(_ms_ssim_backward([(flat[2 * i], flat[2 * i + 1]) for i in range(5)], sums, metas[v], go, 1.0))
        gl = []
        for l in liks:
            o = torch.empty_like(l)
            L.call("hesic_log_backward", L.ptr(l), lik_scale, L.ptr(o), l.numel(), L.stream())
            gl.append(o)
        if SCALED_LOSS:
            gl = [t.mul_(g_loss) for t in gl]
        return (None, None, None, grads[0], grads[1], *gl)


def rd_loss(out, x1, x2, lmbda, distortion="mse"):
    """dict(loss, bpp_loss, mse_loss) like the reference's criterion; differentiable through ``loss``.  ``distortion="ms-ssim"``:
    loss = lmbda * ms_ssim_loss + bpp_loss with ms_ssim_loss = (1 - mean MS(x1_hat, x1)) + (1 - mean MS(x2_hat, x2)) (no 255^2 factor; images
    with a side > 160), reported next to the other three."""
    if distortion not in DISTORTIONS:
        raise ValueError(f"rd_loss: distortion must be one of {DISTORTIONS}, got {distortion!r}")
    lk = out["likelihoods"]
    if distortion == "ms-ssim":
        L.require_cuda(x1, x2, out["x1_hat"], out["x2_hat"])
        _ms_ssim_check(out["x1_hat"], x1)
        _ms_ssim_check(out["x2_hat"], x2)
        loss, bpp, mse, msl = _RdMsSsimLossFn.apply(lmbda, x1, x2, out["x1_hat"], out["x2_hat"], lk["y1"], lk["y2"], lk["z1"], lk["z2"])
        return {"loss": loss, "bpp_loss": bpp.detach(), "mse_loss": mse.detach(), "ms_ssim_loss": msl.detach()}
    loss, bpp, mse = _RdLossFn.apply(lmbda, x1, x2, out["x1_hat"], out["x2_hat"], lk["y1"], lk["y2"], lk["z1"], lk["z2"])
    return {"loss": loss, "bpp_loss": bpp.detach(), "mse_loss": mse.detach()}


def set_phase_fusion(mode):
    """How transposed stride-2 layers run on the implicit-GEMM kernels (``hesic_conv2d_set_phase_fusion``): 0 = one block per (tile,
    output phase), 1 = auto (the four phases of a tile in one block when the launch fills the chip that way; default), 2 = whenever the
    shape is eligible.  Results are bit-identical in every mode.  Returns the previous mode."""
    prev = int(L.lib().hesic_conv2d_set_phase_fusion(int(mode)))
    if prev < 0:
        raise ValueError(f"set_phase_fusion: bad mode {mode}: {L.lib().hesic_last_error().decode()}")
    return prev

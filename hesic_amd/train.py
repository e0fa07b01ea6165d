"""Training harness of the path (the build's counterpart of ywz/mywork/newtrain1.py:74-111): R-D loss, the
two-optimiser update order, and plain data parallelism -- one process per GPU, gradients averaged with RCCL
all-reduce over xGMI (``torch.distributed`` backend "nccl" on ROCm).

The reference has no multi-device code at all; pairs are independent, the loss normalises by the
LOCAL batch (newtrain1.py:45-47), so averaging rank gradients reproduces the single-process gradient of the
concatenated batch exactly.

Layout (round 2).  The parameters of an optimiser group live in ONE flat fp32 buffer and so do their gradients
(``FlatGroup``): ``p.data`` / ``p.grad`` are views.  That makes the bookkeeping of a step a handful of launches: one fill
clears all gradients, the weight-gradient kernels ADD into their slot in place (``functional.GradSlot``: no unpack, no
AccumulateGrad copy/add), the all-reduce runs in place on contiguous slices of the flat gradient (no ``torch.cat`` /
``copy_`` pack and unpack), one Adam launch updates everything.  The collective is issued per bucket as soon as the
bucket's last gradient has been written, so it overlaps the rest of the backward pass, and every piece is capturable:
``GraphedTrainer`` records the step -- collectives included -- into one HIP graph per rank.
"""
from __future__ import annotations

import ctypes as C
import os as _os

import torch
import torch.distributed as dist

from . import functional as Fn


class MultiTensorAdam(torch.optim.Adam):
    """``torch.optim.Adam(params, lr)`` with the update of all tensors in a handful of HIP launches
    (``hesic_adam_step``: 24 tensors per launch, descriptors in the kernel arguments).

    State layout and ``state_dict`` are those of ``torch.optim.Adam(capturable=True)`` (per-parameter fp32 ``step`` on the
    device, ``exp_avg``, ``exp_avg_sq``), so checkpoints move between the two.  Why: the multi-tensor (foreach) torch
    step falls back to one elementwise launch per parameter for its 0-dim step counters -- ~290 launches, 1.2 ms of the
    9 ms graphed training step.  Anything this kernel does not cover (CPU tensors, non-fp32, non-contiguous, amsgrad,
    weight decay, maximize) goes to the parent's step.  Self-contained: ``step()`` bumps the version counters of what it
    updated and starts a new epoch for the packed-weight caches, like any in-place optimiser."""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8):
        super().__init__(params, lr=lr, betas=betas, eps=eps, capturable=True, foreach=True)

    @torch.no_grad()
    def step(self, closure=None):
        from . import _lib as L
        for group in self.param_groups:
            ps = [p for p in group["params"] if p.grad is not None]
            ok = (not group.get("amsgrad") and not group.get("weight_decay") and not group.get("maximize")
                  and not isinstance(group["lr"], torch.Tensor)
                  and all(p.is_cuda and p.dtype == torch.float32 and p.grad.dtype == torch.float32 and not p.grad.is_sparse
                          and p.is_contiguous() and p.grad.is_contiguous() for p in ps))
            if not ok:
                return super().step(closure)
        loss = closure() if closure is not None else None
        for group in self.param_groups:
            ps = [p for p in group["params"] if p.grad is not None]
            for p in ps:
                st = self.state[p]
                if len(st) == 0:
                    st["step"] = torch.zeros((), dtype=torch.float32, device=p.device)
                    st["exp_avg"] = torch.zeros_like(p, memory_format=torch.contiguous_format)
                    st["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.contiguous_format)
            b1, b2 = group["betas"]
            for i in range(0, len(ps), L.ADAM_MAX_TENSORS):
                part = ps[i:i + L.ADAM_MAX_TENSORS]
                c = L.AdamChunk()
                for j, p in enumerate(part):
                    st = self.state[p]
                    c.p[j], c.g[j], c.m[j], c.v[j] = p.data_ptr(), p.grad.data_ptr(), st["exp_avg"].data_ptr(), st["exp_avg_sq"].data_ptr()
                    c.step[j], c.numel[j] = st["step"].data_ptr(), p.numel()
                c.n, c.lr, c.beta1, c.beta2, c.eps = len(part), float(group["lr"]), float(b1), float(b2), float(group["eps"])
                L.call("hesic_adam_step", C.byref(c), L.stream())
            # the kernel writes through raw pointers: tell PyTorch (version counters, like any in-place optimiser) and the
            # packed-weight / GDN / bottleneck caches (keyed on those counters) that the parameters moved
            if ps:
                torch.autograd.graph.increment_version(ps)
        return loss


# ------------------------------------------------------------------------------------------------ flat buffers
class FlatGroup:
    """The parameters of one optimiser group as views into one flat fp32 buffer, their gradients as views into another.

    ``p.data`` and ``p.grad`` are re-pointed (values are kept); state-dict keys, shapes and ``nn.Module`` structure are
    untouched.  Every tensor starts on a 256-byte boundary (the kernels read biases / GDN parameters with 16-byte loads).
    Moving the module afterwards (``.to()``, ``.cuda()``) would break the aliasing: build the group last."""

    ALIGN = 64      # floats

    def __init__(self, params):
        seen, self.params = set(), []
        for p in params:
            if p.requires_grad and id(p) not in seen:
                seen.add(id(p))
                self.params.append(p)
        if not self.params:
            raise ValueError("FlatGroup: no trainable parameters")
        dev = self.params[0].device
        if any(p.device != dev or p.dtype != torch.float32 for p in self.params):
            raise ValueError("FlatGroup: fp32 parameters on one device")
        self.offsets, off = [], 0
        for p in self.params:
            self.offsets.append(off)
            off += -(-p.numel() // self.ALIGN) * self.ALIGN
        self.numel = off
        self.flat_p = torch.zeros(off, dtype=torch.float32, device=dev)
        self.flat_g = torch.zeros(off, dtype=torch.float32, device=dev)
        self.grad_views = []
        with torch.no_grad():
            for p, o in zip(self.params, self.offsets):
                view = self.flat_p[o:o + p.numel()].view(p.shape)
                view.copy_(p.detach())
                p.data = view
                g = self.flat_g[o:o + p.numel()].view(p.shape)
                p.grad = g
                self.grad_views.append(g)
        self.slots = [Fn.GradSlot(g, name=str(i)) for i, g in enumerate(self.grad_views)]
        if dev.type == "cuda":
            import weakref
            keys = Fn.register_grad_slots(zip(self.params, self.slots))
            weakref.finalize(self, Fn.clear_grad_slots, keys)       # a dead group must not keep its gradient buffer registered

    def zero_grad(self):
        """One fill for every gradient of the group (a kernel, not a memset: graph-safe); re-attaches ``p.grad`` views that
        user code dropped (``zero_grad(set_to_none=True)``)."""
        self.flat_g.fill_(0)
        for p, g, s in zip(self.params, self.grad_views, self.slots):
            if p.grad is not g:
                p.grad = g
            s.writes = 0

    def view_like_params(self, flat):
        return [flat[o:o + p.numel()].view(p.shape) for p, o in zip(self.params, self.offsets)]


class FlatAdam:
    """``torch.optim.Adam(params, lr)`` (newtrain1.py:294-295; no amsgrad / weight decay) over a ``FlatGroup``: ONE update
    launch for the whole group (``hesic_adam_step`` on the flat buffers; padding elements have zero gradient and stay
    zero).  ``state_dict()`` / ``load_state_dict()`` speak ``torch.optim.Adam``'s per-parameter format.

    ``controls`` (a dict with ``max_norm`` -- ``None``: no clipping --, ``skip_nonfinite`` and ``also_require``, another ``FlatAdam`` on
    the control path or ``None``) switches the step to the device-resident controls of include/hesic_train_ctl.h: ``step()`` is then
    ``hesic_grad_norm_ctl`` (the global L2 norm of the flat gradient, the clip coefficient and the apply / skip decision, written into the
    control block ``ctl``) followed by ``hesic_adam_step_ctl``, which reads the learning rate, the coefficient and the decision from that
    block.  Nothing is read back: the pair can be recorded into a HIP graph, and ``sync_lr()`` (a device fill OUTSIDE the graph) changes
    the rate every later replay uses.  Without ``controls`` a step is the single ``hesic_adam_step`` it always was."""

    def __init__(self, group: FlatGroup, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, controls=None):
        self.group, self.betas, self.eps = group, (float(betas[0]), float(betas[1])), float(eps)
        self.exp_avg = torch.zeros_like(group.flat_p)
        self.exp_avg_sq = torch.zeros_like(group.flat_p)
        self.step_count = torch.zeros((), dtype=torch.float32, device=group.flat_p.device)
        self.param_groups = [{"params": group.params, "lr": float(lr), "betas": self.betas, "eps": self.eps}]
        self.ctl = self.partials = self.also_require = self._ctl_lr = None
        if controls is not None:
            from . import _lib as L
            dev = group.flat_p.device
            block = [0.0] * L.CTL_FLOATS
            block[L.CTL_LR] = float(lr)
            block[L.CTL_MAX_NORM] = 0.0 if controls.get("max_norm") is None else float(controls["max_norm"])
            block[L.CTL_SKIP_NONFINITE] = 1.0 if controls.get("skip_nonfinite") else 0.0
            block[L.CTL_CLIP_COEF], block[L.CTL_APPLIED] = 1.0, 1.0
            self.ctl = torch.tensor(block, dtype=torch.float32).to(dev)
            self.partials = torch.zeros(L.GRAD_NORM_MAX_BLOCKS, dtype=torch.float64, device=dev)
            self.also_require = controls.get("also_require")
            self._ctl_lr = float(lr)

    def sync_lr(self):
        """Control path: bring the control block's learning rate to ``param_groups[0]["lr"]`` (one device fill when it changed, nothing
        otherwise).  Never call it while a graph is being captured: the fill would be recorded with today's value."""
        lr = float(self.param_groups[0]["lr"])
        if self.ctl is not None and lr != self._ctl_lr:
            self.ctl[0:1].fill_(lr)
            self._ctl_lr = lr

    def zero_grad(self, set_to_none=False):
        self.group.zero_grad()

    @torch.no_grad()
    def step(self):
        from . import _lib as L
        g = self.group
        c = L.AdamChunk()
        c.p[0], c.g[0], c.m[0], c.v[0] = g.flat_p.data_ptr(), g.flat_g.data_ptr(), self.exp_avg.data_ptr(), self.exp_avg_sq.data_ptr()
        c.step[0], c.numel[0] = self.step_count.data_ptr(), g.numel
        c.n, c.lr, c.beta1, c.beta2, c.eps = 1, float(self.param_groups[0]["lr"]), self.betas[0], self.betas[1], self.eps
        if self.ctl is None:
            L.call("hesic_adam_step", C.byref(c), L.stream())
        else:
            # the flat gradient is read twice and never scaled: the norm's launch pair decides, the update applies g * clip_coef
            L.call("hesic_grad_norm_ctl", L.ptr(g.flat_g), g.numel, L.ptr(self.partials), L.ptr(self.ctl),
                   None if self.also_require is None else L.ptr(self.also_require.ctl), L.stream())
            L.call("hesic_adam_step_ctl", C.byref(c), L.ptr(self.ctl), L.stream())
        # the kernel writes through raw pointers: bump the version counters (like any in-place optimiser) -- every cache of
        # packed weights / GDN parameters / bottleneck tables is keyed on them
        torch.autograd.graph.increment_version(g.params)

    def state_dict(self):
        m, v = self.group.view_like_params(self.exp_avg), self.group.view_like_params(self.exp_avg_sq)
        state = {i: {"step": self.step_count.clone(), "exp_avg": m[i].clone(), "exp_avg_sq": v[i].clone()} for i in range(len(m))}
        pg = {"lr": self.param_groups[0]["lr"], "betas": self.betas, "eps": self.eps, "weight_decay": 0, "amsgrad": False, "maximize": False,
              "foreach": None, "capturable": True, "differentiable": False, "fused": None, "params": list(range(len(m)))}
        return {"state": state, "param_groups": [pg]}

    @torch.no_grad()
    def load_state_dict(self, sd):
        m, v = self.group.view_like_params(self.exp_avg), self.group.view_like_params(self.exp_avg_sq)
        for i, st in sd["state"].items():
            m[int(i)].copy_(st["exp_avg"])
            v[int(i)].copy_(st["exp_avg_sq"])
            self.step_count.fill_(float(st["step"]))
        if sd.get("param_groups"):
            self.param_groups[0]["lr"] = sd["param_groups"][0].get("lr", self.param_groups[0]["lr"])
            self.sync_lr()


class FlatReducer:
    """Gradient averaging over the ranks, in place on a ``FlatGroup``'s flat gradient buffer.

    The buffer is cut into ~``bucket_mb`` buckets of whole parameters.  With ``overlap`` a bucket's all-reduce is issued
    (``async_op``: on the backend's own stream, after an event on the compute stream) the moment its last gradient has been
    written -- gradient kernels report through ``GradSlot.on_write``, parameters that go through autograd's AccumulateGrad
    through a post-accumulate hook -- so the collective runs under the rest of the backward pass.  How many writes complete
    a parameter (encoder1's weights receive two per step) is learned in the first step, which reduces everything at
    ``finish()``.  ``finish()`` launches what is left (parameters without gradient on this rank still take part: ranks stay
    in step), waits and -- for backends without an averaging reduction (gloo) -- divides.  world_size 1: all no-ops.

    ``collective`` (round 5; environment default ``HESIC_DP_COLLECTIVE``): "allreduce" -- one in-place all-reduce per bucket (a ring on
    RCCL: 2 (N-1)/N of the bucket over ONE xGMI link per hop, ~1.6 ms for the 140 MB of HESIC at N = 8) -- or "rsag": the same
    sum as a reduce-scatter into this rank's 1/N of the bucket followed by an all-gather of the shards, both in place on the flat buffer;
    on a fully connected xGMI node every rank then exchanges 1/N of the bucket with each of its 7 peers at once (~0.23 ms).  The part of a
    bucket beyond a multiple of N elements (< N values) goes through a small all-reduce.  Values are equal to "allreduce" up to the
    summation order (``tests/test_dp_gloo.py``); unmeasured on hardware until an 8-GPU node exists."""

    def __init__(self, group: FlatGroup, bucket_mb: float = 25.0, process_group=None, overlap=True, force=False, collective=None):
        self.group, self.pg, self.overlap = group, process_group, overlap
        self.collective = collective or _os.environ.get("HESIC_DP_COLLECTIVE", "allreduce")
        if self.collective not in ("allreduce", "rsag"):
            raise ValueError("FlatReducer: collective must be 'allreduce' or 'rsag'")
        up = dist.is_available() and dist.is_initialized()
        self.world = dist.get_world_size(process_group) if up else 1
        self.buckets, self._work, self._expected, self._events = [], [], None, [0] * len(group.params)
        self.compute_stream = None
        # ``force``: issue the collectives even in a 1-rank group (a 1-GPU box can then exercise RCCL bring-up and the capture
        # of the all-reduces into the step's HIP graph)
        self.active = self.world > 1 or (force and up)
        if not self.active:
            return
        self.avg_op = dist.get_backend(process_group) == "nccl"
        cap = max(1, int(bucket_mb * (1 << 20) / 4))
        lo, members = 0, []
        for i in range(len(group.params)):
            end = group.offsets[i + 1] if i + 1 < len(group.params) else group.numel
            members.append(i)
            if end - lo >= cap or i + 1 == len(group.params):
                self.buckets.append({"lo": lo, "hi": end, "members": members, "pending": len(members), "launched": False})
                lo, members = end, []
        self._bucket_of = {}
        for bi, b in enumerate(self.buckets):
            for i in b["members"]:
                self._bucket_of[i] = bi
        # the closures hold the reducer only weakly and the hook handles are kept: a second reducer / Trainer on the same model
        # must not leave this one's hooks firing (and its flat buffers alive) -- ``close()`` removes them
        import weakref
        me = weakref.ref(self)

        def fire(i):
            r = me()
            if r is not None:
                r._event(i)
        self._handles = []
        for i, (p, s) in enumerate(zip(group.params, group.slots)):
            s.on_write = (lambda slot, i=i: fire(i))
            self._handles.append(p.register_post_accumulate_grad_hook(lambda p_, i=i: fire(i)))
        # diagnostics (``timing = True``, eager steps on RCCL only): every bucket's all-reduce runs synchronously on a communication
        # stream of its own between two events, ``report()`` gives per-bucket durations and the share hidden under the backward pass
        self.timing, self._comm, self._timed, self._bwd_end = False, None, [], None

    def close(self):
        """Detach from the parameters (hooks, slot callbacks)."""
        for h in getattr(self, "_handles", []):
            h.remove()
        self._handles = []
        for s in self.group.slots:
            s.on_write = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def begin(self):
        """Call before the backward pass of every step."""
        if not self.active:
            return
        self._events = [0] * len(self.group.params)
        self.compute_stream = torch.cuda.current_stream() if self.group.flat_g.is_cuda else None
        for b in self.buckets:
            b["pending"], b["launched"] = len(b["members"]), False

    def _event(self, i):
        self._events[i] += 1
        if self._expected is None or self._events[i] != self._expected[i]:
            return
        b = self.buckets[self._bucket_of[i]]
        b["pending"] -= 1
        if b["pending"] == 0 and self.overlap and not b["launched"]:
            self._launch(b)

    def _launch(self, b):
        b["launched"] = True
        op = dist.ReduceOp.AVG if self.avg_op else dist.ReduceOp.SUM
        buf = self.group.flat_g[b["lo"]:b["hi"]]
        if buf.is_cuda:
            # a bucket's gradients are written on the compute stream: the stream the collective is issued from waits for it
            cur = torch.cuda.current_stream()
            if self.compute_stream is not None and self.compute_stream != cur:
                cur.wait_stream(self.compute_stream)
        if self.timing and self.avg_op and buf.is_cuda:
            if self._comm is None:
                self._comm = torch.cuda.Stream(device=buf.device)
            self._comm.wait_stream(torch.cuda.current_stream())
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            with torch.cuda.stream(self._comm):
                e0.record()
                for w in self._collect(buf, op, False):              # synchronous on the communication stream: e1 is its completion
                    pass
                e1.record()
            self._timed.append((b["hi"] - b["lo"], e0, e1))
            return
        self._work.extend(self._collect(buf, op, True))

    def _collect(self, buf, op, async_op):
        """The bucket's sum over the ranks, in place: one all-reduce, or reduce-scatter + all-gather (see the class docstring)."""
        if self.collective == "allreduce" or self.world < 2:
            return [dist.all_reduce(buf, op=op, group=self.pg, async_op=async_op)]
        n, W = buf.numel(), self.world
        main = n - n % W
        works = []
        if main:
            rank = dist.get_rank(self.pg)
            shard = buf[rank * (main // W):(rank + 1) * (main // W)]
            # the all-gather reads the shard the reduce-scatter wrote: the two are issued in order on the backend's stream; with async_op the
            # first is waited for before the second is issued only on backends that run collectives on the caller's thread (gloo)
            w1 = dist.reduce_scatter_tensor(shard, buf[:main], op=op, group=self.pg, async_op=async_op)
            if async_op and not self.avg_op:
                w1.wait()
                w1 = None
            w2 = dist.all_gather_into_tensor(buf[:main], shard, group=self.pg, async_op=async_op)
            works += [w for w in (w1, w2) if w is not None]
        if main < n:
            works.append(dist.all_reduce(buf[main:], op=op, group=self.pg, async_op=async_op))
        return [w for w in works if w is not None]

    def finish(self):
        """Call once after the backward pass: launches the remaining buckets, waits, averages."""
        if not self.active:
            return
        if self.timing and self.avg_op and self.group.flat_g.is_cuda:
            self._bwd_end = torch.cuda.Event(enable_timing=True)
            self._bwd_end.record()                       # the backward pass ends here on the compute stream
        for b in self.buckets:
            if not b["launched"]:
                self._launch(b)
        if self._comm is not None and self._timed:
            torch.cuda.current_stream().wait_stream(self._comm)
        for w in self._work:
            w.wait()
        self._work.clear()
        if not self.avg_op and self.world > 1:
            self.group.flat_g.div_(self.world)
        if self._expected is None:
            # a parameter that saw no gradient event this step completes its bucket at finish() in later steps too
            self._expected = [e if e > 0 else -1 for e in self._events]


def _step_controls(cls, clip_max_norm, skip_nonfinite, live_lr):
    """The step controls of the trainer class named ``cls``, checked and normalised: ``(clip_max_norm as a float or None, skip_nonfinite,
    live_lr)``.  Called first in a constructor: a bad argument is refused before any device or dtype check."""
    if clip_max_norm is not None:
        import math
        ok = isinstance(clip_max_norm, (int, float)) and not isinstance(clip_max_norm, bool)
        if not ok or not math.isfinite(clip_max_norm) or clip_max_norm <= 0:
            raise ValueError(f"{cls}: clip_max_norm must be a finite positive number (or None: no clipping), got {clip_max_norm!r}")
        clip_max_norm = float(clip_max_norm)
    for name, flag in (("skip_nonfinite", skip_nonfinite), ("live_lr", live_lr)):
        if not isinstance(flag, bool):
            raise TypeError(f"{cls}: {name} must be a bool, got {type(flag).__name__}")
    return clip_max_norm, skip_nonfinite, live_lr


def _control_readout(optimizer, skipped_from=None):
    """``{"grad_norm", "clip_coef", "skipped"}`` of ``optimizer``'s control block: views while a graph is captured (every replay refreshes them),
    copies otherwise.  ``skipped_from``: the optimiser whose block holds the count (default: ``optimizer`` itself)."""
    from . import _lib as L
    own = (lambda t: t) if torch.cuda.is_current_stream_capturing() else torch.clone
    ctl, counts = optimizer.ctl, (optimizer if skipped_from is None else skipped_from).ctl
    return {"grad_norm": own(ctl[L.CTL_GRAD_NORM]), "clip_coef": own(ctl[L.CTL_CLIP_COEF]), "skipped": own(counts[L.CTL_SKIPPED])}


class Trainer:
    """Holds the model, ``Adam(parameters, lr)`` + ``Adam(aux_parameters, aux_lr)`` (newtrain1.py:294-295) over flat
    parameter / gradient buffers and, when a process group is up, one in-place reducer per optimiser group.

    Step controls (all off by default; with none set a step issues exactly the launches it always did):

    - ``clip_max_norm``: clip the gradient of ``model.parameters()`` to this global L2 norm before the main Adam, with
      ``torch.nn.utils.clip_grad_norm_``'s coefficient ``min(1, max_norm / (norm + 1e-6))``.  The norm is taken of the flat gradient buffer
      AFTER the reduction over the ranks (every rank sees the same buffer and reaches the same coefficient).  The bottlenecks' aux group is
      not clipped, as ``clip_grad_norm_(model.parameters(), ...)`` would not touch it in the reference's loop.
    - ``skip_nonfinite``: a NaN / Inf anywhere in the main gradient skips the step AS A WHOLE -- parameters, both optimisers' moments and
      both step counters stay as they were; the aux group has the same guard on its own gradient (which can only withhold the aux update:
      the main one has been applied by then).
    - ``live_lr``: the learning rates are read from device memory by every step, so ``set_lr`` and direct writes to
      ``optimizer.param_groups[0]["lr"]`` (torch's schedulers) take effect under ``GraphedTrainer``'s replay too.

    Any of the three puts the step on the control path (``FlatAdam(controls=...)``): on the device nothing is read back and the step stays
    capturable.  ``step`` then also returns ``grad_norm`` (of the main group, before clipping), ``clip_coef`` and ``skipped``, the running
    count of steps in which an update was withheld.  The gradient buffers are left unscaled.  Host modules (the gloo tests) get the same
    semantics from ``clip_grad_norm_`` and an ``isfinite`` test around ``torch.optim.Adam``.  ``Stage2Trainer`` and ``MultiTensorAdam``
    have no such controls: a user loop on them can call torch's own ``clip_grad_norm_``."""

    def __init__(self, model, lr=1e-4, aux_lr=1e-3, lmbda=1e-2, bucket_mb=25.0, overlap=True, force_collectives=False, collective=None,
                 distortion="mse", clip_max_norm=None, skip_nonfinite=False, live_lr=False):
        if distortion not in Fn.DISTORTIONS:
            raise ValueError(f"Trainer: distortion must be one of {Fn.DISTORTIONS}, got {distortion!r}")
        clip_max_norm, skip_nonfinite, live_lr = _step_controls("Trainer", clip_max_norm, skip_nonfinite, live_lr)
        self.clip_max_norm, self.skip_nonfinite, self.live_lr = clip_max_norm, skip_nonfinite, live_lr
        self.controls = clip_max_norm is not None or skip_nonfinite or live_lr
        # "ms-ssim": loss = lmbda * ((1 - MS-SSIM(x1_hat, x1)) + (1 - MS-SSIM(x2_hat, x2))) + bpp (functional.rd_loss); lmbda has no 255^2
        # factor there, so values of the MSE criterion do not carry over
        self.model, self.lmbda, self.distortion = model, float(lmbda), distortion
        main, aux = list(model.parameters()), list(model.aux_parameters())
        self.main_group, self.aux_group = FlatGroup(main), FlatGroup(aux)
        self.on_gpu = self.main_group.flat_p.is_cuda
        if self.on_gpu:
            ctl = {"max_norm": clip_max_norm, "skip_nonfinite": skip_nonfinite, "also_require": None} if self.controls else None
            self.optimizer = FlatAdam(self.main_group, lr=lr, controls=ctl)
            # the aux group: no clipping, the same guard, and never applied in a step whose main update was withheld
            self.aux_optimizer = FlatAdam(self.aux_group, lr=aux_lr,
                                          controls=dict(ctl, max_norm=None, also_require=self.optimizer) if self.controls else None)
        else:       # host modules (the gloo tests): torch's Adam on the same views
            self.optimizer = torch.optim.Adam(self.main_group.params, lr=lr)
            self.aux_optimizer = torch.optim.Adam(self.aux_group.params, lr=aux_lr)
        # EB matrices/biases/factors get their gradient from the main backward but are stepped by the aux
        # optimiser after the aux backward adds the quantile gradient: both groups are reduced,
        # the aux group only after the aux backward.
        self.main_reducer = FlatReducer(self.main_group, bucket_mb, overlap=overlap, force=force_collectives, collective=collective)
        self.aux_reducer = FlatReducer(self.aux_group, bucket_mb, overlap=False, force=force_collectives, collective=collective)
        self.world = self.main_reducer.world
        self._host_stats = {"grad_norm": torch.zeros(()), "clip_coef": torch.ones(()), "skipped": 0, "applied": True}

    def set_lr(self, lr, aux_lr=None):
        """Set the learning rate of the main optimiser (and of the aux optimiser when ``aux_lr`` is given) for every following step: writes
        ``param_groups`` and, on the control path, the device control blocks (a device fill, outside any graph)."""
        self.optimizer.param_groups[0]["lr"] = float(lr)
        if aux_lr is not None:
            self.aux_optimizer.param_groups[0]["lr"] = float(aux_lr)
        self._sync_lr()

    def _sync_lr(self):
        if self.controls and self.on_gpu and not torch.cuda.is_current_stream_capturing():
            self.optimizer.sync_lr()
            self.aux_optimizer.sync_lr()

    def _host_step(self, aux):
        """The control path for host modules: torch's own clip and an isfinite test around ``torch.optim.Adam.step``."""
        st = self._host_stats
        if not aux:
            params = self.main_group.params
            if self.clip_max_norm is not None:
                norm = torch.nn.utils.clip_grad_norm_(params, self.clip_max_norm)
                coef = torch.clamp(self.clip_max_norm / (norm + 1e-6), max=1.0)
            else:
                norm, coef = torch.linalg.vector_norm(self.main_group.flat_g), torch.ones(())
            st["grad_norm"], st["clip_coef"] = norm.detach(), coef.detach()
            st["applied"] = not (self.skip_nonfinite and not bool(torch.isfinite(norm)))
            if st["applied"]:
                self.optimizer.step()
            return
        applied = st["applied"] and not (self.skip_nonfinite and not bool(torch.isfinite(self.aux_group.flat_g).all()))
        if applied:
            self.aux_optimizer.step()
        else:
            st["skipped"] += 1

    def _forward_loss(self, x1, x2, h_matrix, noise):
        out = self.model(x1, x2, h_matrix, noise=noise)
        return Fn.rd_loss(out, x1, x2, self.lmbda, distortion=self.distortion)

    def _check_inputs(self, x1, x2):
        """Host-side refusals, before anything is launched (or staged into a graph's static buffers)."""
        if self.distortion == "ms-ssim" and min(min(x1.shape[-2:]), min(x2.shape[-2:])) <= 160:
            raise ValueError("Trainer: distortion='ms-ssim' needs images whose smaller side exceeds (11 - 1) * 2^4 = 160 (five scales of an "
                             f"11-tap window), got {tuple(x1.shape[-2:])}")

    def step(self, x1, x2, h_matrix, noise=None):
        """One iteration in the reference's order: zero both -> forward -> R-D loss backward -> (reduce) -> optimizer.step
        -> aux loss backward -> (reduce) -> aux_optimizer.step.  Returns the loss dict (device scalars, no sync)."""
        self._check_inputs(x1, x2)
        self._sync_lr()                           # control path: param_groups -> control block (not while capturing: GraphedTrainer does it)
        self.model.train()
        self.main_group.zero_grad()
        self.aux_group.zero_grad()
        self.main_reducer.begin()
        self.aux_reducer.begin()
        prev = Fn.train_pack_cache(True)          # packed conv weights persist across the step, one batched repack below
        scaled, Fn.SCALED_LOSS = Fn.SCALED_LOSS, False     # backward() starts at the unscaled loss: no g_loss multiplies
        slots = Fn.grad_slots_active(True)        # gradient kernels add straight into the flat buffer (cleared above) for THIS step only
        defer = Fn.defer_wgrad_finish(self.on_gpu)     # finishing passes of the weight gradients: batches of 8 layers per launch
        try:
            crit = self._forward_loss(x1, x2, h_matrix, noise)
            crit["loss"].backward()
        finally:
            Fn.defer_wgrad_finish(defer)          # flushes what is still queued: every weight gradient is in (or on its way into) the flat buffer
            Fn.train_pack_cache(prev)
            Fn.SCALED_LOSS = scaled
            Fn.grad_slots_active(slots)
        self.main_reducer.finish()
        if self.controls and not self.on_gpu:
            self._host_step(aux=False)
        else:
            self.optimizer.step()                 # control path: norm of the REDUCED gradient -> decision -> update, all on the device
        if self.on_gpu:
            Fn.repack_all()                       # every packed conv weight of the step refreshed (and re-tagged) in ONE launch
        aux = self.model.aux_loss()
        slots = Fn.grad_slots_active(True)
        try:
            aux.backward()
        finally:
            Fn.grad_slots_active(slots)
        self.aux_reducer.finish()
        if self.controls and not self.on_gpu:
            self._host_step(aux=True)
        else:
            self.aux_optimizer.step()
        # detached scalars only: a returned loss that still requires grad would keep this step's autograd graph (and its
        # AccumulateGrad nodes, bound to this step's stream) alive into the next one
        crit = {k: v.detach() for k, v in crit.items()}
        crit["aux_loss"] = aux.detach()
        if self.controls and self.on_gpu:
            crit.update(_control_readout(self.optimizer, self.aux_optimizer))    # the aux block's count includes the steps the main group withheld
        elif self.controls:
            st = self._host_stats
            crit["grad_norm"], crit["clip_coef"], crit["skipped"] = st["grad_norm"], st["clip_coef"], torch.tensor(float(st["skipped"]))
        return crit


class _GraphedStep:
    """A step recorded once into a HIP graph and replayed: the base of ``GraphedTrainer`` and ``GraphedEnhancerTrainer``, listed BEFORE the
    eager trainer whose ``step`` and ``set_lr`` it wraps (``super()`` here is that trainer).

    The first ``warmup`` calls run eagerly on a side stream (real steps), the next call captures, every later call is a copy of the inputs into
    the static buffers -- nothing, when the producer wrote into ``static_inputs()`` -- plus one graph launch.  A subclass's ``step`` stages,
    syncs the learning rate, may drop a stale graph, and ends in ``_run``; ``_captured`` and ``_replayed`` are its hooks.  Without step
    controls the captured Adam holds its learning rate by value and ``set_lr`` refuses after the capture."""

    _ADAM = "Adam launch"       # how ``set_lr``'s refusal names the captured optimiser work

    class _Slot:
        """One captured step: its call count, graph, static inputs and static outputs."""
        __slots__ = ("calls", "graph", "inputs", "out")

        def __init__(self):
            self.calls, self.graph, self.inputs, self.out = 0, None, None, None

    def _init_graph(self, warmup, why):
        if int(warmup) < 1:
            raise ValueError(f"{type(self).__name__}: warmup >= 1 ({why})")
        self.warmup = int(warmup)
        # one slot per key; ``calls`` / ``graph`` / ``_in`` / ``_out`` are those of the slot in use (a trainer with one kind of step never
        # leaves the ``None`` slot)
        self._slots = {None: _GraphedStep._Slot()}
        self._slot = self._slots[None]

    def _use_slot(self, key):
        slot = self._slots.get(key)
        if slot is None:
            slot = self._slots[key] = _GraphedStep._Slot()
        self._slot = slot
        return slot

    calls = property(lambda self: self._slot.calls, lambda self, v: setattr(self._slot, "calls", v))
    graph = property(lambda self: self._slot.graph, lambda self, v: setattr(self._slot, "graph", v))
    _in = property(lambda self: self._slot.inputs, lambda self, v: setattr(self._slot, "inputs", v))
    _out = property(lambda self: self._slot.out, lambda self, v: setattr(self._slot, "out", v))

    def set_lr(self, *rates, **kw):
        if any(slot.graph is not None for slot in self._slots.values()) and not self.controls:
            raise RuntimeError(f"{type(self).__name__}.set_lr: the captured step holds its learning rate by value in the kernel arguments of "
                               f"its {self._ADAM}, a replay cannot see a new one -- build the trainer with live_lr=True (the rate is then "
                               "read from device memory by every replay)")
        super().set_lr(*rates, **kw)

    def static_inputs(self):
        """The step's static input tensors ``(x1, x2, h_matrix)``, or ``None`` before the first step.  A producer that writes a batch straight
        into them and passes them to ``step`` saves the staging copies: ``_stage`` finds equal pointers and copies nothing."""
        return self._in

    def _stage(self, *inputs):
        if self._in is None:
            self._in = tuple(t.clone() for t in inputs)
        else:
            for dst, src in zip(self._in, inputs):
                if src.data_ptr() != dst.data_ptr():
                    dst.copy_(src)

    def _captured(self):
        pass

    def _run(self, eager=None, **kw):
        """Count the call, then the eager step on the static inputs -- on a side stream (warm-up) or under capture -- or a replay.  ``eager``:
        the wrapped trainer's step method (default: its ``step``)."""
        if eager is None:
            eager = super().step
        self.calls += 1
        if self.graph is None and self.calls <= self.warmup:
            side = torch.cuda.Stream(device=self._in[0].device)
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):
                out = eager(*self._in, **kw)
            torch.cuda.current_stream().wait_stream(side)
            return out
        if self.graph is None:
            self.graph = torch.cuda.CUDAGraph()
            # The process group's watchdog thread polls the events of the warm-up steps' collectives; under the default ("global")
            # capture mode such a query from ANOTHER thread while this one captures is an error that takes the process down
            # ("operation not permitted when stream is capturing", seen with one RCCL rank).  Drain first, and confine the capture
            # rules to this thread.
            torch.cuda.synchronize()
            with torch.cuda.graph(self.graph, capture_error_mode="thread_local"):
                self._out = eager(*self._in, **kw)
            self._captured()
        self.graph.replay()
        self._replayed()            # a replay runs no Python: the captured Adam moved the parameters without touching their version counters
        return self._out


class GraphedTrainer(_GraphedStep, Trainer):
    """``Trainer.step`` recorded once into a HIP graph and replayed -- with a process group up, one graph per rank with the
    bucketed RCCL all-reduces inside it (collectives are stream work like any kernel; their forked comm-stream nodes keep the
    overlap with the backward pass in the graph).

    One training step is a few hundred launches, most of them a few microseconds long: eagerly the Python/ctypes launch work
    exceeds the GPU time, so the step is host-bound.  The first ``warmup`` calls run eagerly on a side stream (they are real
    steps: they pack weights, size workspaces, let autograd allocate and teach the reducer how many writes complete each
    gradient), the next call captures zero_grad -> forward -> R-D backward -> reduce -> Adam -> aux backward -> reduce -> aux
    Adam and every later call is a copy of the inputs into the static buffers plus one graph launch.  The quantisation noise
    is drawn inside the graph by the graph-safe Philox generator unless a ``noise`` dict is given at capture time (then it is
    a static input too).  The returned dict holds the graph's static loss tensors (overwritten by the next call).

    The learning rate: WITHOUT step controls (``clip_max_norm`` / ``skip_nonfinite`` / ``live_lr``, see ``Trainer``) the captured Adam
    launches hold the rate of the capture BY VALUE in their kernel arguments -- a later write to ``optimizer.param_groups[0]["lr"]`` is
    ignored by every replay, and ``set_lr`` refuses with a ``RuntimeError`` rather than pretend.  WITH any of them (``live_lr=True`` is the
    one that asks for nothing else) the rate lives in the control block: ``set_lr`` and writes to ``param_groups`` are picked up before
    every replay by a device fill outside the graph."""

    _ADAM = "Adam launches"

    def __init__(self, model, *args, warmup=3, **kw):
        super().__init__(model, *args, **kw)
        if not self.on_gpu:
            raise RuntimeError("GraphedTrainer needs the model on a ROCm device")
        self._init_graph(warmup, "the packed-weight registry and the reducer's write counts are created by an eager step")
        self._noise = None
        # only RCCL's collectives are stream work; gloo stages through the host (synchronises) and cannot be captured
        self.capturable = not (self.main_reducer.active and not self.main_reducer.avg_op)
        if not self.capturable:
            import warnings
            warnings.warn("GraphedTrainer: the process group's backend is not nccl/RCCL -- its collectives cannot be captured into a HIP "
                          "graph, steps run eagerly")

    def _stage(self, x1, x2, h_matrix, noise):
        first = self._in is None
        super()._stage(x1, x2, h_matrix)
        if first:
            self._noise = None if noise is None else {k: v.clone() for k, v in noise.items()}
        elif self._noise is not None:
            if noise is None:
                raise RuntimeError("GraphedTrainer: the step was captured with explicit noise tensors")
            for k, dst in self._noise.items():
                dst.copy_(noise[k])

    def _replayed(self):
        # every cache keyed on the parameters' version counters (bottleneck tables, packed GDN parameters, inference weight packs) must
        # start a new epoch
        Fn.invalidate_weight_cache()

    def step(self, x1, x2, h_matrix, noise=None):
        if not self.capturable:
            return super().step(x1, x2, h_matrix, noise=noise)
        self._check_inputs(x1, x2)
        self._stage(x1, x2, h_matrix, noise)
        self._sync_lr()                           # control path: this call's rate, filled in ahead of the capture / the replay
        return self._run(noise=self._noise)


class HomographyTrainer:
    """HomographyNet's training loop (udh/udh/QHtrain.py:88-102) on the device: ``delta = net(patch_a, patch_b)`` in training mode,
    ``homography.photometric_loss``, backward, ``Adam(net.parameters(), lr)`` -- one ``FlatGroup`` over the parameters, so a step is one fill
    that clears every gradient, the forward and backward kernels (the weight gradients go straight into their flat slots) and one Adam
    launch.  Nothing is read back to the host, and with up to 64 rows per batch a step -- and a run resumed from ``state_dict()`` -- repeats
    its bits (larger batches take the fc layers' conv route, whose bias sums end in float atomics).  The compute dtype is fp32 for the duration of a step (``net`` must store fp32 maps).

    ``clip_max_norm``, ``skip_nonfinite`` and ``live_lr`` are ``Trainer``'s step controls (``FlatAdam(controls=...)``): with any of them set
    ``step`` also returns ``grad_norm`` (before clipping), ``clip_coef`` and ``skipped``.  ``seed`` seeds the dropout masks
    (``net.set_dropout_state(seed, 0)``).

    The trainer is EAGER: the dropout masks' step counter is a kernel argument passed by value, so a captured HIP graph would replay one
    mask forever.  ``step`` raises while a stream is capturing.  ``GraphedHomographyTrainer`` is the same step with the counter in device
    memory, recorded into a HIP graph."""

    _CAPTURABLE = False         # GraphedHomographyTrainer: the dropout state lives on the device, the step may be recorded

    def __init__(self, net, lr=1e-4, seed=0, clip_max_norm=None, skip_nonfinite=False, live_lr=False):
        clip_max_norm, skip_nonfinite, live_lr = _step_controls("HomographyTrainer", clip_max_norm, skip_nonfinite, live_lr)
        if getattr(net, "dtype", torch.float32) != torch.float32:
            raise NotImplementedError("HomographyTrainer: the net must store fp32 maps (Net(dtype=torch.float32))")
        self.net = net
        self.group = FlatGroup(net.parameters())
        if not self.group.flat_p.is_cuda:
            raise RuntimeError("HomographyTrainer: the HIP path needs the net on a ROCm device (no CPU fallback)")
        self.controls = clip_max_norm is not None or skip_nonfinite or live_lr
        ctl = {"max_norm": clip_max_norm, "skip_nonfinite": skip_nonfinite, "also_require": None} if self.controls else None
        self.optimizer = FlatAdam(self.group, lr=lr, controls=ctl)
        net.set_dropout_state(seed, 0)

    def set_lr(self, lr):
        """The learning rate of every following step (``param_groups`` and, on the control path, the device control block)."""
        self.optimizer.param_groups[0]["lr"] = float(lr)
        self.optimizer.sync_lr()

    def _train_step(self, name, patch_a, patch_b, criterion):
        """zero the flat gradient -> train-mode forward -> ``criterion(delta)`` -> backward -> one Adam launch.  Returns device scalars."""
        capturing = torch.cuda.is_current_stream_capturing()
        if capturing and not self._CAPTURABLE:
            raise RuntimeError(f"HomographyTrainer.{name} is eager: the dropout step counter is passed to the kernels by value, a captured "
                               "graph would replay one mask forever")
        if not capturing:                         # a fill recorded into a graph would hold today's rate
            self.optimizer.sync_lr()
        self.net.train()
        self.group.zero_grad()
        prev_dtype = Fn.compute_dtype()
        Fn.set_compute_dtype(torch.float32)
        try:
            pack = Fn.train_pack_cache(True)          # packed conv weights persist across the step, one batched repack below
            slots = Fn.grad_slots_active(True)        # gradient kernels write straight into the flat buffer (cleared above)
            try:
                with torch.enable_grad():
                    loss = criterion(self.net(patch_a, patch_b))
                loss.backward()
            finally:
                Fn.grad_slots_active(slots)
                Fn.train_pack_cache(pack)
            self.optimizer.step()
            Fn.repack_all()
        finally:
            Fn.set_compute_dtype(prev_dtype)
        out = {"loss": loss.detach()}
        if self.controls:
            out.update(_control_readout(self.optimizer))         # copies, unless GraphedHomographyTrainer is capturing
        return out

    def _eval_delta(self, patch_a, patch_b):
        """The net's deltas in eval mode (no dropout, no graph) with fp32 maps; the module's mode is left as it was."""
        was, prev_dtype = self.net.training, Fn.compute_dtype()
        self.net.eval()
        Fn.set_compute_dtype(torch.float32)
        try:
            return self.net(patch_a, patch_b)
        finally:
            Fn.set_compute_dtype(prev_dtype)
            self.net.train(was)

    def step(self, img_a, patch_a, patch_b, corners):
        """zero the flat gradient -> train-mode forward -> photometric loss -> backward -> one Adam launch.  Returns device scalars."""
        from . import homography
        return self._train_step("step", patch_a, patch_b, lambda delta: homography.photometric_loss(delta, img_a, patch_b, corners))

    @torch.no_grad()
    def evaluate(self, img_a, patch_a, patch_b, corners):
        """The photometric loss of the net in eval mode (no dropout, no graph); the module's mode is left as it was."""
        from . import homography
        return homography.photometric_loss(self._eval_delta(patch_a, patch_b), img_a, patch_b, corners)

    def step_supervised(self, patch_a, patch_b, delta):
        """``step`` with a known label (a synthetic warp, ``DevicePairCache.homonet_synth_batch``): ``loss = mse_loss(net(patch_a, patch_b),
        delta)``, the mean over the 8 B numbers -- in torch, there is no hot path in it --, then the same backward, Adam launch, controls,
        eager-only rule and return dict."""
        return self._train_step("step_supervised", patch_a, patch_b, lambda out: torch.nn.functional.mse_loss(out, delta))

    @torch.no_grad()
    def evaluate_supervised(self, patch_a, patch_b, delta):
        """``(loss, corner_error)`` of the net in eval mode against the label: the supervised MSE (a 0-d device tensor) and, per pair, the
        mean corner error in pixels of the frame (``homography.corner_error``, a (B,) fp32 device tensor)."""
        from . import homography
        out = self._eval_delta(patch_a, patch_b)
        return torch.nn.functional.mse_loss(out, delta), homography.corner_error(out, delta)

    def _prepare_pairs(self, x1, x2, xy, pic_size, rho, rng):
        from . import homography
        grey1, _, patch1, patch2, corners = homography.prepare_inputs(x1, x2, xy, pic_size, self.net.side * 8, rho, rng)
        return grey1, patch1, patch2, corners

    def step_pairs(self, x1, x2, xy=None, pic_size=256, rho=45, rng=None):
        """``step`` on a stereo batch that is on the device: ``homography.prepare_inputs`` (one launch; the window side is the net's,
        ``xy=None`` draws the loader's random windows) gives QHtrain's ``img_a, patch_a, patch_b, corners``."""
        return self.step(*self._prepare_pairs(x1, x2, xy, pic_size, rho, rng))

    def evaluate_pairs(self, x1, x2, xy=None, pic_size=256, rho=45, rng=None):
        """``evaluate`` on a stereo batch that is on the device (see ``step_pairs``)."""
        return self.evaluate(*self._prepare_pairs(x1, x2, xy, pic_size, rho, rng))

    def state_dict(self):
        return {"state_dict": {k: v.detach().clone() for k, v in self.net.state_dict().items()}, "optimizer": self.optimizer.state_dict(),
                "dropout": tuple(self.net.dropout_state())}

    def load_state_dict(self, sd):
        """Parameters (copied into the flat buffer's views), Adam state and the dropout (seed, step): the next step continues bit for bit
        (batches of up to 64 rows; see ``homography``'s module docstring)."""
        self.net.load_state_dict(sd["state_dict"])
        self.optimizer.load_state_dict(sd["optimizer"])
        self.net.set_dropout_state(*sd["dropout"])


class GraphedHomographyTrainer(_GraphedStep, HomographyTrainer):
    """``HomographyTrainer.step`` and ``step_supervised`` recorded into HIP graphs and replayed, by ``GraphedTrainer``'s protocol
    (``_GraphedStep``).  What kept the eager trainer out of a graph -- the dropout step counter in the kernel arguments -- lives in device
    memory here (``net.dropout_on_device()``): the captured forward begins with ``hesic_dropout_state_take``, so every replay draws the mask
    the eager trainer would draw in that step, bit for bit, and a checkpoint moves between the two trainers in both directions.

    Each KIND of step (``"step"``: ``(img_a, patch_a, patch_b, corners)``; ``"supervised"``: ``(patch_a, patch_b, delta)``) has its own
    slot: the first ``warmup`` calls of a kind run eagerly on a side stream (real steps), the next one captures, every later one copies the
    inputs into the slot's static tensors (nothing, when the producer wrote into ``static_inputs(kind)``) and launches the graph.  A kind's
    graph belongs to the first input shapes that get through their warm-up; a call with other shapes (an epoch's ragged last batch) runs
    eagerly through the same device-state kernels -- no second capture, no error, the same bits.  The returned dict holds the slot's static
    device scalars (``loss``, and with controls ``grad_norm``, ``clip_coef``, ``skipped``), overwritten by the next call of that kind.

    After a replay the parameters' version counters are bumped, as the eager Adam does, and the registered training packs -- refreshed on
    the device by the captured ``repack_all`` -- are marked current: ``evaluate`` and eager steps between replays see the trained weights
    and keep using the buffers the graphs hold by address.  Without step controls the captured Adam holds its learning rate by value and
    ``set_lr`` refuses after the first capture.  ``step_pairs`` is not offered here (``NotImplementedError``): its input prep draws
    windows on the host; prepare the batch (``homography.prepare_inputs`` or a ``DevicePairCache`` with ``out=static_inputs(kind)``) and
    call ``step``."""

    _CAPTURABLE = True
    KINDS = ("step", "supervised")

    def __init__(self, net, *args, warmup=3, **kw):
        super().__init__(net, *args, **kw)
        self._init_graph(warmup, "the packed-weight registry is created by an eager step")
        net.dropout_on_device(True)
        self._kind_key = {}         # kind -> the (kind, input shapes) key of its captured slot

    def graph_slot(self, kind="step"):
        """The captured slot of ``kind`` (``calls``, ``graph``, ``inputs``, ``out``), or ``None`` before its capture."""
        if kind not in self.KINDS:
            raise ValueError(f"GraphedHomographyTrainer: kind is one of {self.KINDS}, got {kind!r}")
        key = self._kind_key.get(kind)
        return None if key is None else self._slots[key]

    def static_inputs(self, kind="step"):
        """The static input tensors of ``kind``'s captured slot (in the order of that step's arguments), or ``None`` before its capture."""
        slot = self.graph_slot(kind)
        return None if slot is None else slot.inputs

    def _replayed(self):
        torch.autograd.graph.increment_version(self.group.params)       # Net._fc1_nhwc, the _fc_pack packers: keyed on the version counters
        Fn.packs_replayed(self.group.params)

    def _graphed(self, kind, eager, inputs):
        key = (kind, tuple(tuple(t.shape) for t in inputs))
        self.optimizer.sync_lr()                  # control path: this call's rate, filled in ahead of the capture / the replay
        if self._kind_key.get(kind, key) != key:
            return eager(*inputs)                 # not the shapes of this kind's graph: the eager route, on the same device state
        slot = self._use_slot(key)
        self._stage(*inputs)
        out = self._run(eager=eager)
        if slot.graph is not None and kind not in self._kind_key:
            # the first shapes to get through their warm-up own the kind's graph; the other candidates' static tensors are let go
            self._kind_key[kind] = key
            for other in [k for k in self._slots if k is not None and k[0] == kind and k != key]:
                del self._slots[other]
        return out

    def load_state_dict(self, sd):
        """``HomographyTrainer.load_state_dict``, then the registered training packs are refreshed from the loaded parameters: a replay
        starts at the forward and reads them as they stand (the eager step finds their tags stale and re-packs by itself)."""
        super().load_state_dict(sd)
        Fn.repack_all()

    def step(self, img_a, patch_a, patch_b, corners):
        return self._graphed("step", super().step, (img_a, patch_a, patch_b, corners))

    def step_supervised(self, patch_a, patch_b, delta):
        return self._graphed("supervised", super().step_supervised, (patch_a, patch_b, delta))

    def step_pairs(self, *args, **kw):
        raise NotImplementedError("GraphedHomographyTrainer.step_pairs: prepare the batch (homography.prepare_inputs) and call step")


def comm_report(reducer):
    """Per-bucket all-reduce timings of the steps run with ``reducer.timing = True`` (synchronises the device): a list of
    {mb, ms, gbps} per launch order, the total, and ``hidden_frac`` = the share of the communication time that lay before the end
    of the backward pass on the compute stream (what the overlap hides; 0 for a reducer built with overlap=False)."""
    torch.cuda.synchronize()
    recs, total, hidden = [], 0.0, 0.0
    for numel, e0, e1 in reducer._timed:
        ms = e0.elapsed_time(e1)
        recs.append({"mb": round(numel * 4 / 1e6, 2), "ms": round(ms, 4), "gbps": round(numel * 4 / 1e6 / max(ms, 1e-6), 1)})
        total += ms
        if reducer._bwd_end is not None:
            # [t0, t1]: this all-reduce on a clock whose zero is the end of the backward pass (event times are comparable across
            # streams; negative = before it); the part before zero ran under the backward pass
            t0, t1 = reducer._bwd_end.elapsed_time(e0), reducer._bwd_end.elapsed_time(e1)
            hidden += max(0.0, min(t1, 0.0) - min(t0, 0.0))
    reducer._timed.clear()
    return {"buckets": recs, "total_ms": round(total, 4), "hidden_frac": round(hidden / total, 4) if total > 0 else None}


def init_distributed(backend=None):
    """Process-group bring-up from the torchrun environment (RANK / LOCAL_RANK / WORLD_SIZE / MASTER_*).
    Returns (rank, world_size, local_rank); a plain single-process run returns (0, 1, 0)."""
    import os
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if world == 1:
        return 0, 1, 0
    rank, local = int(os.environ["RANK"]), int(os.environ.get("LOCAL_RANK", "0"))
    if backend is None:
        # HESIC_DIST_BACKEND=gloo + HESIC_SINGLE_DEVICE=1: several ranks sharing ONE GPU (functional check of the multi-rank code
        # paths on a 1-GPU box; RCCL itself refuses two ranks on one device)
        backend = os.environ.get("HESIC_DIST_BACKEND") or ("nccl" if torch.cuda.is_available() else "gloo")
    if os.environ.get("HESIC_SINGLE_DEVICE"):
        local = 0
    if torch.cuda.is_available():
        torch.cuda.set_device(local)
    if not dist.is_initialized():
        dist.init_process_group(backend=backend, rank=rank, world_size=world)
    return rank, world, local


class Stage2Trainer:
    """Stage 2 of the reference's schedule (ywz/mywork/newtrain6_real.py:120-167): the compression model is FROZEN in eval mode (rounded
    latents, no noise), the enhancement net ``Independent_EN`` trains on its reconstructions with
    ``loss = lambda * 255^2 * (MSE(x1_hat', x1) + MSE(x2_hat', x2))`` (:83-91, ``kind=0``) and one Adam over ITS parameters (:287); the
    bottlenecks' aux loss is computed there but never stepped (:169-171).  The frozen forward runs under ``no_grad`` in whatever 16-bit /
    fp32 mode is selected for inference; the enhancement net's forward / backward in ``train_dtype`` (bf16 or fp32)."""

    def __init__(self, model, enhancer, lr=1e-4, lmbda=1e-2, train_dtype=None):
        self.model, self.enhancer, self.lmbda = model, enhancer, float(lmbda)
        # training runs in bfloat16 (fp32 exponent range) or fp32: with float16 inference selected the enhancer needs an explicit training
        # format (with train_dtype=None the first step failed inside an operator instead of here)
        if train_dtype is None and Fn.compute_dtype() == torch.float16:
            train_dtype = torch.bfloat16
        if train_dtype not in (None, torch.bfloat16, torch.float32):
            raise ValueError("Stage2Trainer: train_dtype is None, torch.bfloat16 or torch.float32 (float16 is an inference format)")
        self.train_dtype = train_dtype
        self.optimizer = MultiTensorAdam(list(enhancer.parameters()), lr=lr) if next(enhancer.parameters()).is_cuda else \
            torch.optim.Adam(enhancer.parameters(), lr=lr)

    def step(self, x1, x2, h_matrix):
        self.model.eval()
        self.enhancer.train()
        self.optimizer.zero_grad(set_to_none=True)
        with torch.no_grad():
            out = self.model(x1, x2, h_matrix)
        keep = Fn.compute_dtype()
        if self.train_dtype is not None and self.train_dtype != keep:
            Fn.set_compute_dtype(self.train_dtype)
        try:
            out2 = self.enhancer(out["x1_hat"].float(), out["x2_hat"].float(), h_matrix)
            mse = ((out2["x1_hat"].float() - x1) ** 2).mean() + ((out2["x2_hat"].float() - x2) ** 2).mean()
            loss = self.lmbda * 255 ** 2 * mse
            loss.backward()
        finally:
            if Fn.compute_dtype() != keep:
                Fn.set_compute_dtype(keep)
        self.optimizer.step()
        return {"loss": loss.detach(), "mse_loss": mse.detach()}


class EnhancerTrainer:
    """Stage 2 as a first-class path: ``Stage2Trainer``'s loss and ``train_dtype`` handling (the f16-inference / bf16-training switch
    included) over flat buffers, with ``Trainer``'s step controls.

    The enhancer's parameters live in one ``FlatGroup`` stepped by one ``FlatAdam``; ``clip_max_norm``, ``skip_nonfinite`` and ``live_lr``
    mean what they mean on ``Trainer`` (the same control block, the same returned ``grad_norm`` / ``clip_coef`` / ``skipped``, ``set_lr``), and
    with none of them set no control launch is issued.  The data-gradient weights of the enhancer's 40 convs live in one more flat buffer
    that ONE ``hesic_c32_mirror_weights`` launch per step refreshes (``functional.register_mirror_views``), and the two output layers plus the
    criterion are one autograd node (``Independent_EN.criterion``).  A step: zero the flat gradient -> mirror launch -> frozen forward
    (``no_grad``, eval mode) -> ``enhancer.criterion`` -> ``loss.backward()`` with the gradient slots and the mirror registry active and
    ``SCALED_LOSS`` off -> Adam.  The frozen model's parameters never receive a gradient and its aux loss is not computed (the reference
    computes it and never steps it, newtrain6_real.py:169-171).  Every launch of the step reduces in a fixed order, so equal inputs and state
    give equal bits."""

    def __init__(self, model, enhancer, lr=1e-4, lmbda=1e-2, train_dtype=None, clip_max_norm=None, skip_nonfinite=False, live_lr=False):
        clip_max_norm, skip_nonfinite, live_lr = _step_controls("EnhancerTrainer", clip_max_norm, skip_nonfinite, live_lr)
        if train_dtype is None and Fn.compute_dtype() == torch.float16:
            train_dtype = torch.bfloat16
        if train_dtype not in (None, torch.bfloat16, torch.float32):
            raise ValueError("EnhancerTrainer: train_dtype is None, torch.bfloat16 or torch.float32 (float16 is an inference format)")
        self.model, self.enhancer, self.lmbda, self.train_dtype = model, enhancer, float(lmbda), train_dtype
        self.clip_max_norm, self.skip_nonfinite, self.live_lr = clip_max_norm, skip_nonfinite, live_lr
        self.controls = clip_max_norm is not None or skip_nonfinite or live_lr
        self.group = FlatGroup(enhancer.parameters())
        self.on_gpu = self.group.flat_p.is_cuda
        if not self.on_gpu:
            raise RuntimeError("EnhancerTrainer: the HIP path needs the enhancer on a ROCm device (no CPU fallback)")
        ctl = {"max_norm": clip_max_norm, "skip_nonfinite": skip_nonfinite, "also_require": None} if self.controls else None
        self.optimizer = FlatAdam(self.group, lr=lr, controls=ctl)
        # the mirror table: every 3x3 conv of up to 32 x 32 channels, its weight's offset in the flat parameters and its slot in flat_m
        import weakref
        offset = {id(p): o for p, o in zip(self.group.params, self.group.offsets)}
        entries, views, off = [], [], 0
        for p in self.group.params:
            if p.dim() == 4 and tuple(p.shape[2:]) == (3, 3) and p.shape[0] <= 32 and p.shape[1] <= 32:
                entries.append((offset[id(p)], off, p.shape[0], p.shape[1], 32))
                views.append((p, off, p.shape[1] * 32 * 9))
                off += -(-p.shape[1] * 32 * 9 // FlatGroup.ALIGN) * FlatGroup.ALIGN
        self.mirror_layers = len(entries)
        if entries:
            self.flat_m = torch.zeros(off, dtype=torch.float32, device=self.group.flat_p.device)
            self.mirror_table = Fn.mirror_table(entries, self.flat_m.device)
            keys = Fn.register_mirror_views((p, self.flat_m[o:o + n].view(p.shape[1], 32, 3, 3)) for p, o, n in views)
            weakref.finalize(self, Fn.clear_mirror_views, keys)

    def set_lr(self, lr):
        """The learning rate of every following step (``param_groups`` and, on the control path, the device control block)."""
        self.optimizer.param_groups[0]["lr"] = float(lr)
        self._sync_lr()

    def _sync_lr(self):
        if self.controls and not torch.cuda.is_current_stream_capturing():
            self.optimizer.sync_lr()

    def step(self, x1, x2, h_matrix):
        """One iteration (see the class docstring); returns detached device scalars ``{"loss", "mse_loss"}`` plus ``grad_norm``, ``clip_coef``
        and ``skipped`` when controls are set."""
        self._sync_lr()                           # control path: param_groups -> control block (not while capturing)
        self.model.eval()
        self.enhancer.train()
        self.group.zero_grad()
        if self.mirror_layers:
            Fn.c32_mirror_weights(self.group.flat_p, self.flat_m, self.mirror_table, self.mirror_layers)
        with torch.no_grad():
            out = self.model(x1, x2, h_matrix)
        keep = Fn.compute_dtype()
        if self.train_dtype is not None and self.train_dtype != keep:
            Fn.set_compute_dtype(self.train_dtype)
        scaled, Fn.SCALED_LOSS = Fn.SCALED_LOSS, False     # backward() starts at the unscaled loss
        slots = Fn.grad_slots_active(True)
        mirror = Fn.mirror_views_active(self.mirror_layers > 0)
        try:
            with torch.enable_grad():
                crit = self.enhancer.criterion(out["x1_hat"].float(), out["x2_hat"].float(), h_matrix, x1, x2, self.lmbda)
                crit["loss"].backward()
        finally:
            Fn.mirror_views_active(mirror)
            Fn.grad_slots_active(slots)
            Fn.SCALED_LOSS = scaled
            if Fn.compute_dtype() != keep:
                Fn.set_compute_dtype(keep)
        res = {"loss": crit["loss"].detach(), "mse_loss": crit["mse_loss"].detach()}
        self.optimizer.step()
        if self.controls:
            res.update(_control_readout(self.optimizer))
        return res


class GraphedEnhancerTrainer(_GraphedStep, EnhancerTrainer):
    """``EnhancerTrainer.step`` recorded once into a HIP graph and replayed, by ``GraphedTrainer``'s protocol (``_GraphedStep``): the first ``warmup`` calls run
    eagerly on a side stream (real steps), the next call captures, every later call copies the inputs into the static buffers (nothing, when the
    producer wrote into ``static_inputs()``) and launches the graph.  The returned dict holds the graph's static tensors (overwritten by the
    next call).  Without step controls the captured Adam holds its learning rate by value and ``set_lr`` refuses after the capture; with any of
    them the rate is read from device memory by every replay.  After a replay the enhancer's parameters get their version counters bumped (what
    the eager optimiser step does); the global pack-cache epoch is left alone, because the graph reads the frozen model's cached packed weights
    by address -- and when somebody else moves that epoch (``functional.invalidate_weight_cache``), the next call runs eagerly and the one
    after it captures again.  Stage 2 has no collectives: one process, one device."""

    def __init__(self, model, enhancer, *args, warmup=3, **kw):
        super().__init__(model, enhancer, *args, **kw)
        self._init_graph(warmup, "workspaces and the frozen model's packed weights are created by an eager step")
        self._epoch = None

    def _captured(self):
        self._epoch = Fn._epoch_n

    def _replayed(self):
        # Bump the version counters, as the eager ``FlatAdam.step`` does: every cache keyed on the ENHANCER's parameters misses from here on.
        # ``GraphedTrainer`` starts a new global cache epoch instead; here that would also drop the FROZEN model's packed weights, which the
        # graph reads by address (see above).
        torch.autograd.graph.increment_version(self.group.params)

    def step(self, x1, x2, h_matrix):
        self._stage(x1, x2, h_matrix)
        self._sync_lr()                           # this call's rate, filled in ahead of the capture / the replay
        if self.graph is not None and Fn._epoch_n != self._epoch:
            # Somebody started a new pack-cache epoch (``invalidate_weight_cache``) since the capture: the frozen model's next eager forward
            # replaces -- and frees -- the packed weights this graph reads.  Drop the graph: one eager step re-packs, the next call captures.
            self.graph, self._out, self.calls = None, None, self.warmup - 1
        return self._run()

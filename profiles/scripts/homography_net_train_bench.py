#!/usr/bin/env python3
"""What HomographyNet's training costs, one process on one box, warm, median of ``--runs`` (7) with the variants alternating:

    step      ``train.HomographyTrainer.step`` at patch_size = 128, 1 x 256 x 256 images, B = 16 and B = 64, eager, host clock around
              ``--step-reps`` steps that end in a device synchronise;
    linear    ``hesic_linear_forward`` / ``_dgrad`` / ``_wgrad`` at fc.2's size (1024 x 32768) and fc.5's (8 x 1024), B = 16 and B = 64,
              and on the SAME tensors the route that existed before: the 1x1 implicit-GEMM conv of ``functional._ConvFn`` including the
              re-pack a changed weight forces (forward, and the other orientation for the data gradient) and ``hesic_conv2d_wgrad_direct``
              (fc.5, eight outputs: the strided kernels that route takes);
    pool      ``hesic_maxpool2_backward`` at the three pool sizes of the net, B = 16;
    flatten   ``hesic_flatten_dropout_forward`` / ``_backward`` at (B, 256, 128), p = 0.5, B = 16 and B = 64;

every kernel as the HIP-event time of ``--reps`` replays of a captured graph, next to the bytes it has to move (from the shapes) and the time
a plain device copy of as many bytes takes on this box -- the ratio to the copy is the figure to read.

Writes profiles/homography_net_train_bench.json and prints it.  Run it under a time limit of its own:

    timeout -k 10 600 python profiles/scripts/homography_net_train_bench.py
"""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)


def _med(v):
    s = sorted(v)
    return {"median": round(s[len(s) // 2], 3), "min": round(s[0], 3), "max": round(s[-1], 3), "runs": len(s)}


def _event_us(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps * 1e3


def _graph_of(fn):
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _ in range(2):
            keep = fn()
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        keep = fn()
    return g, keep


def _copy_of(nbytes):
    src = torch.empty(max(nbytes // 8, 1), dtype=torch.float32, device="cuda").normal_()       # a copy moves 2 x its size
    dst = torch.empty_like(src)
    return lambda: dst.copy_(src)


def _measure(variants, runs, reps):
    """variants: {name: (callable, bytes or None)} -> {name: {"us", "bytes", "copy_same_bytes_us", "times_the_copy"}}; one copy per byte count."""
    copies = {nb: _copy_of(nb) for nb in {nb for _, nb in variants.values() if nb}}
    t = {k: [] for k in variants}
    tc = {nb: [] for nb in copies}
    for _ in range(runs + 1):                    # run 0 is the warm-up of every variant
        for k, (fn, _) in variants.items():
            t[k].append(_event_us(fn, reps))
        for nb, fn in copies.items():
            tc[nb].append(_event_us(fn, reps))
    out = {}
    for k, (_, nb) in variants.items():
        out[k] = {"us": _med(t[k][1:])}
        if nb:
            c = _med(tc[nb][1:])
            out[k].update(bytes=nb, copy_same_bytes_us=c, times_the_copy=round(out[k]["us"]["median"] / c["median"], 2))
    return out


class _Ctx:
    """Stand-in for an autograd context: keeps what ``_ConvFn.forward`` saves so that the pieces of its backward can be replayed alone."""
    needs_input_grad = (True, True, True, False)

    def save_for_backward(self, *t):
        self.saved_tensors = t


def linear_routes(runs, reps, B, In, Out):
    from hesic_amd import _lib as L
    from hesic_amd import functional as Fn
    gen = torch.Generator().manual_seed(0)
    x = (torch.rand((B, In), generator=gen) - 0.5).cuda()
    w = ((torch.rand((Out, In), generator=gen) - 0.5) * (6.0 / In) ** 0.5).cuda()
    b = torch.zeros(Out).cuda()
    gy = (torch.rand((B, Out), generator=gen) - 0.5).cuda()
    y, gx, dw, db = torch.empty((B, Out), device="cuda"), torch.empty_like(x), torch.empty_like(w), torch.empty_like(b)
    nws = int(L.lib().hesic_linear_forward_ws_bytes(B, In, Out))
    ws = torch.empty(nws, dtype=torch.uint8, device="cuda")

    def fwd():
        L.call("hesic_linear_forward", L.ptr(x), L.ptr(w), L.ptr(b), L.ptr(y), B, In, Out, L.ACT_RELU, L.F32, L.ptr(ws), nws, L.stream())

    def dgrad():
        L.call("hesic_linear_dgrad", L.ptr(gy), L.ptr(w), L.ptr(gx), B, In, Out, L.F32, L.stream())

    def wgrad():
        L.call("hesic_linear_wgrad", L.ptr(x), L.ptr(gy), L.ptr(dw), L.ptr(db), B, In, Out, 0, L.F32, L.stream())

    # the route that existed before, on the same tensors
    x4 = x.view(B, In, 1, 1).contiguous(memory_format=torch.channels_last)
    w4, gy4 = w.view(Out, In, 1, 1), gy.view(B, Out, 1, 1).contiguous(memory_format=torch.channels_last)
    cfg = (1, 1, 0, False, L.ACT_RELU, 0, 0, Fn.PackedWeight(), None)
    ctx = _Ctx()
    with torch.no_grad():
        Fn._ConvFn.forward(ctx, x4, w4, b, cfg)
    grads = Fn._narrow_conv_grads if ctx.narrow else Fn._wide_conv_grads

    def conv_fwd():
        Fn.invalidate_weight_cache()             # the optimiser has moved the weight: the forward re-packs it
        return Fn._ConvFn.forward(_Ctx(), x4, w4, b, cfg)

    def conv_dgrad():
        Fn.invalidate_weight_cache()             # ... and the data gradient packs the other orientation
        return grads(x4, w4, gy4, cfg, ctx.dims, True, True, False, b)[0]

    def conv_wgrad():
        return grads(x4, w4, gy4, cfg, ctx.dims, True, False, True, b)[1]

    wbytes = In * Out * 4
    with torch.no_grad():
        variants = {"linear_forward": (_graph_of(fwd)[0].replay, wbytes), "conv_route_forward": (_graph_of(conv_fwd)[0].replay, None),
                    "linear_dgrad": (_graph_of(dgrad)[0].replay, wbytes), "conv_route_dgrad": (_graph_of(conv_dgrad)[0].replay, None),
                    "linear_wgrad": (_graph_of(wgrad)[0].replay, wbytes), "conv_route_wgrad": (_graph_of(conv_wgrad)[0].replay, None)}
        rec = _measure(variants, runs, reps)
    rec["shape"] = {"B": B, "In": In, "Out": Out}
    rec["conv_route_kernels"] = "strided (narrow)" if ctx.narrow else "implicit GEMM + wgrad_direct"
    for k in ("forward", "dgrad", "wgrad"):
        rec[f"conv_route_over_linear_{k}"] = round(rec[f"conv_route_{k}"]["us"]["median"] / rec[f"linear_{k}"]["us"]["median"], 2)
    return rec


def pools(runs, reps, B=16):
    from hesic_amd import _lib as L
    variants = {}
    keep = []
    for Cc, side in ((64, 128), (64, 64), (128, 32)):
        x = torch.relu(torch.randn((B, side, side, Cc), device="cuda"))
        gy = torch.randn((B, side // 2, side // 2, Cc), device="cuda")
        gx = torch.empty_like(x)
        keep.append((x, gy, gx))

        def fn(x=x, gy=gy, gx=gx, Cc=Cc, side=side):
            L.call("hesic_maxpool2_backward", L.ptr(x), L.ptr(gy), L.ptr(gx), B, side, side, Cc, L.F32, L.stream())
        variants[f"maxpool2_backward_{Cc}x{side}x{side}"] = (_graph_of(fn)[0].replay, (2 * x.numel() + gy.numel()) * 4)
    return dict(_measure(variants, runs, reps), B=B)


def flatten(runs, reps, B):
    from hesic_amd import _lib as L
    from hesic_amd import functional as Fn
    HW, Cc = 256, 128
    x, g = torch.randn((B, HW, Cc), device="cuda"), torch.randn((B, HW * Cc), device="cuda")
    y, gx = torch.empty_like(g), torch.empty_like(x)
    cfg = Fn.dropout_args(0.5, 1, 0, 0)
    variants = {
        "flatten_dropout_forward": (_graph_of(lambda: L.call("hesic_flatten_dropout_forward", L.ptr(x), L.ptr(y), B, HW, Cc, *cfg, L.F32, L.stream()))[0].replay,
                                    2 * x.numel() * 4),
        "flatten_dropout_backward": (_graph_of(lambda: L.call("hesic_flatten_dropout_backward", L.ptr(g), L.ptr(gx), B, HW, Cc, *cfg, L.F32, L.stream()))[0].replay,
                                     2 * x.numel() * 4)}
    return dict(_measure(variants, runs, reps), shape={"B": B, "HW": HW, "C": Cc})


def steps(runs, step_reps, batches=(16, 64)):
    from hesic_amd import homography, synthetic, train
    rec, t, jobs = {}, {}, {}
    for B in batches:
        net = homography.Net(patch_size=128)
        synthetic.fill_homography_state_dict_(net.state_dict())
        tr = train.HomographyTrainer(net.cuda(), lr=1e-6, seed=0)
        gen = torch.Generator().manual_seed(B)
        img_a = torch.rand((B, 1, 256, 256), generator=gen).cuda()
        patch_a, patch_b = img_a[:, :, 64:192, 64:192].contiguous(), torch.rand((B, 1, 128, 128), generator=gen).cuda()
        corners = (torch.full((B, 1, 2), 64.0) + torch.tensor([[0.0, 0.0], [128, 0.0], [128, 128], [0.0, 128]])).cuda()
        jobs[B], t[B] = (tr, (img_a, patch_a, patch_b, corners)), []
    for _ in range(runs + 1):
        for B, (tr, args) in jobs.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(step_reps):
                out = tr.step(*args)
            torch.cuda.synchronize()
            t[B].append((time.perf_counter() - t0) / step_reps * 1e3)
            rec[f"B{B}"] = {"loss_finite": bool(torch.isfinite(out["loss"]))}
    for B in batches:
        rec[f"B{B}"]["ms_per_step"] = _med(t[B][1:])
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--step-reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "homography_net_train_bench.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("homography_net_train_bench: needs a ROCm device")
    rec = {"device": torch.cuda.get_device_name(0), "runs": a.runs, "reps_per_run": a.reps, "step": steps(a.runs, a.step_reps)}
    for name, (In, Out) in (("fc2", (32768, 1024)), ("fc5", (1024, 8))):
        for B in (16, 64):
            rec[f"{name}_B{B}"] = linear_routes(a.runs, a.reps, B, In, Out)
    rec["pool"] = pools(a.runs, a.reps)
    for B in (16, 64):
        rec[f"flatten_B{B}"] = flatten(a.runs, a.reps, B)
    with open(a.out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print(json.dumps(rec))


if __name__ == "__main__":
    main()

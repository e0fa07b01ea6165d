#!/usr/bin/env python3
"""What training for MS-SSIM costs, one process on one box, warm, median of ``--runs`` (7) with the variants alternating:

    (a) kernels   one view's ``functional.ms_ssim`` forward (5 x hesic_ssim_scale + 8 x hesic_avgpool2_pad + the (5, B, C) combination) and
                  its backward (5 x hesic_ssim_scale_backward) at B = 8, 3 x 512 x 512 fp32: HIP-event time of ``--reps`` replays of each, captured
                  as a graph (eagerly the host's launch work exceeds the device time), next to the bytes each moves (from the shapes: every
                  image and gradient read or written once per launch that touches it) and the time a plain copy of as many bytes takes on
                  this box -- the yardstick of DESIGN.md section 8.4, not the nominal HBM rate;
    (b) step      the ``GraphedTrainer`` step at B = 8, 512 x 512, bfloat16, with distortion "mse" and "ms-ssim": host clock around ``--steps``
                  replays ending in a synchronise; the difference, and 2 x (a) (two views) beside it.

Writes profiles/msssim_loss_bench.json and prints it.  Run it under a time limit of its own:

    timeout -k 10 600 python profiles/scripts/msssim_loss_bench.py

``--trace`` instead replays the "ms-ssim" step ten times and nothing else: the workload of
``rocprofv3 --kernel-trace --stats -- python profiles/scripts/msssim_loss_bench.py --trace``.
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


def pyramid_bytes(B, C, H, W):
    """Bytes the forward and the backward of one view move, from the shapes alone."""
    px = []
    for _ in range(5):
        px.append(B * C * H * W)
        H, W = (H + 2 * (H % 2) - 2) // 2 + 1, (W + 2 * (W % 2) - 2) // 2 + 1
    fwd = sum(8 * p for p in px) + sum(8 * px[s] + 8 * px[s + 1] for s in range(4))      # ssim reads x, y; the pools read x, y and write both
    bwd = sum(8 * px[s] + 4 * px[s] for s in range(5)) + sum(4 * px[s + 1] for s in range(4))      # reads x, y (+ the coarser gradient), writes g
    return fwd, bwd


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
        for _ in range(3):
            keep = fn()
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        keep = fn()
    return g, keep


def kernels(runs, reps, B=8, C=3, H=512, W=512):
    from hesic_amd import functional as Fn
    gen = torch.Generator().manual_seed(0)
    x = torch.rand((B, C, H, W), generator=gen)
    xh = (x + 0.05 * torch.randn((B, C, H, W), generator=gen)).clamp(0, 1).cuda()
    x = x.cuda()
    go = torch.full((B,), -1.0 / B, dtype=torch.float64, device="cuda")
    with torch.no_grad():
        val, sums, pyramid, counts = Fn._ms_ssim_forward(xh, x, 1.0)
        gf, _ = _graph_of(lambda: Fn._ms_ssim_forward(xh, x, 1.0)[0])
        gb, _ = _graph_of(lambda: Fn._ms_ssim_backward(pyramid, sums, counts, go, 1.0))
    fwd_b, bwd_b = pyramid_bytes(B, C, H, W)
    src = {n: torch.empty(n // 8, dtype=torch.float32, device="cuda").normal_() for n in (fwd_b, bwd_b)}      # a copy moves 2 x its size
    dst = {n: torch.empty_like(t) for n, t in src.items()}
    t = {"forward": [], "backward": [], "copy_forward_bytes": [], "copy_backward_bytes": []}
    for _ in range(runs + 1):                      # run 0 is the warm-up of every variant
        t["forward"].append(_event_us(gf.replay, reps))
        t["copy_forward_bytes"].append(_event_us(lambda: dst[fwd_b].copy_(src[fwd_b]), reps))
        t["backward"].append(_event_us(gb.replay, reps))
        t["copy_backward_bytes"].append(_event_us(lambda: dst[bwd_b].copy_(src[bwd_b]), reps))
    rec = {"shape": [B, C, H, W], "reps_per_run": reps, "ms_ssim": [round(float(v), 6) for v in val],
           "forward": {"us": _med(t["forward"][1:]), "bytes": fwd_b, "copy_same_bytes_us": _med(t["copy_forward_bytes"][1:])},
           "backward": {"us": _med(t["backward"][1:]), "bytes": bwd_b, "copy_same_bytes_us": _med(t["copy_backward_bytes"][1:])}}
    for k in ("forward", "backward"):
        rec[k]["gb_per_s"] = round(rec[k]["bytes"] / rec[k]["us"]["median"] / 1e3, 1)
        rec[k]["copy_gb_per_s"] = round(rec[k]["bytes"] / rec[k]["copy_same_bytes_us"]["median"] / 1e3, 1)
        rec[k]["times_the_copy"] = round(rec[k]["us"]["median"] / rec[k]["copy_same_bytes_us"]["median"], 2)
    return rec


def _trainer(distortion, lmbda, B, size):
    from hesic_amd import models, synthetic
    from hesic_amd.train import GraphedTrainer
    net = models.HSIC()
    synthetic.fill_state_dict_(net.state_dict())
    tr = GraphedTrainer(net.cuda(), lr=1e-4, aux_lr=1e-3, lmbda=lmbda, distortion=distortion)
    batch = tuple(t.cuda() for t in synthetic.stereo_batch(0, B, size, size))
    for _ in range(tr.warmup + 2):                 # eager warm-up steps, the capture, one replay
        out = tr.step(*batch)
    torch.cuda.synchronize()
    assert tr.graph is not None
    return tr, batch, out


def steps(runs, n_steps, B=8, size=512):
    import hesic_amd
    hesic_amd.set_compute_dtype(torch.bfloat16)
    variants = {"mse": _trainer("mse", 0.0067, B, size), "ms-ssim": _trainer("ms-ssim", 31.73, B, size)}
    t = {k: [] for k in variants}
    for rep in range(runs + 1):                    # run 0 is dropped
        for k, (tr, batch, _) in variants.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(n_steps):
                out = tr.step(*batch)
            torch.cuda.synchronize()
            if rep:
                t[k].append((time.perf_counter() - t0) / n_steps * 1e3)
    rec = {"batch": B, "size": size, "dtype": "bfloat16", "steps_per_run": n_steps}
    for k, (tr, batch, _) in variants.items():
        out = tr.step(*batch)
        rec[k] = {"step_ms": _med(t[k]), "last": {n: round(float(v), 6) for n, v in out.items()}}
    rec["difference_ms"] = round(rec["ms-ssim"]["step_ms"]["median"] - rec["mse"]["step_ms"]["median"], 3)
    hesic_amd.set_compute_dtype(torch.float32)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--trace", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "msssim_loss_bench.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("msssim_loss_bench: needs a ROCm device")
    if a.trace:
        import hesic_amd
        hesic_amd.set_compute_dtype(torch.bfloat16)
        tr, batch, _ = _trainer("ms-ssim", 31.73, 8, 512)
        for _ in range(10):
            tr.step(*batch)
        torch.cuda.synchronize()
        return
    rec = {"device": torch.cuda.get_device_name(0), "runs": a.runs}
    rec["kernels"] = kernels(a.runs, a.reps)
    rec["step"] = steps(a.runs, a.steps)
    rec["two_views_forward_backward_ms"] = round(2 * (rec["kernels"]["forward"]["us"]["median"] + rec["kernels"]["backward"]["us"]["median"]) / 1e3, 3)
    with open(a.out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print(json.dumps(rec))


if __name__ == "__main__":
    main()

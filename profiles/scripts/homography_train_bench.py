#!/usr/bin/env python3
"""What the photometric loss costs, one process on one box, warm, median of ``--runs`` (7) with the variants alternating:

    forward   ``homography.photometric_loss`` at B = 16, 1 x 256 x 256 images, 128 x 128 patches, fp32 (hesic_photometric_forward: the DLT,
              the sampling pass with its per-block partials, the finishing pass);
    backward  its gradient to the corner deltas (hesic_photometric_backward: the per-pixel pass, the finishing pass with the DLT adjoint);

each as the HIP-event time of ``--reps`` replays of a captured graph (eagerly the host's launch work exceeds the device time), next to the
bytes it moves (from the shapes: patch_b read once and as many bytes of img_a under the patch's footprint) and the time a plain device copy
of as many bytes takes on this box.  At two megabytes these launches are latency-bound: the ratio to the copy is the figure to read, not a
share of the HBM rate.

Writes profiles/homography_train_bench.json and prints it.  Run it under a time limit of its own:

    timeout -k 10 300 python profiles/scripts/homography_train_bench.py
"""
import argparse
import json
import os
import sys

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
        for _ in range(3):
            keep = fn()
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        keep = fn()
    return g, keep


def photometric(runs, reps, B=16, C=1, H=256, W=256, P=128):
    from hesic_amd import functional as Fn
    from hesic_amd import geometry
    gen = torch.Generator().manual_seed(0)
    img_a = torch.rand((B, C, H, W), generator=gen).cuda()
    patch_b = torch.rand((B, C, P, P), generator=gen).cuda()
    tl = torch.full((B, 1, 2), 64.0)
    corners = (tl + torch.tensor([[0.0, 0.0], [P, 0.0], [P, P], [0.0, P]])).cuda()
    delta = ((torch.rand((B, 4, 2), generator=gen) - 0.5) * 64.0).cuda()
    ac = geometry.DEFAULT_ALIGN_CORNERS
    one = torch.ones((), device="cuda")

    class Ctx:                                   # the forward's context, kept to replay the backward alone
        needs_input_grad = (True, False, False, False, False)

        def save_for_backward(self, *t):
            self.saved_tensors = t

    ctx = Ctx()
    with torch.no_grad():
        loss = Fn._PhotometricFn.forward(ctx, delta, img_a, patch_b, corners, ac)
        gf, _ = _graph_of(lambda: Fn._PhotometricFn.forward(Ctx(), delta, img_a, patch_b, corners, ac))
        gb, keep = _graph_of(lambda: Fn._PhotometricFn.backward(ctx, one)[0])
    nbytes = 2 * B * C * P * P * 4
    src = torch.empty(nbytes // 8, dtype=torch.float32, device="cuda").normal_()       # a copy moves 2 x its size
    dst = torch.empty_like(src)
    t = {"forward": [], "backward": [], "copy": []}
    for _ in range(runs + 1):                    # run 0 is the warm-up of every variant
        t["forward"].append(_event_us(gf.replay, reps))
        t["copy"].append(_event_us(lambda: dst.copy_(src), reps))
        t["backward"].append(_event_us(gb.replay, reps))
    rec = {"shape": {"B": B, "C": C, "image": [H, W], "patch": [P, P]}, "reps_per_run": reps, "loss": round(float(loss), 6),
           "grad_abs_max": float(keep.abs().max()), "bytes": nbytes, "copy_same_bytes_us": _med(t["copy"][1:])}
    for k in ("forward", "backward"):
        rec[k] = {"us": _med(t[k][1:])}
        rec[k]["times_the_copy"] = round(rec[k]["us"]["median"] / rec["copy_same_bytes_us"]["median"], 2)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "homography_train_bench.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("homography_train_bench: needs a ROCm device")
    rec = {"device": torch.cuda.get_device_name(0), "runs": a.runs, "photometric": photometric(a.runs, a.reps)}
    with open(a.out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print(json.dumps(rec))


if __name__ == "__main__":
    main()

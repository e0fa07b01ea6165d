#!/usr/bin/env python3
"""What recording HomographyNet's training step into a HIP graph buys, one process on one box, warm, median of ``--runs`` (7) with the
variants alternating:

    step      ``train.HomographyTrainer.step`` (eager: the baseline, the code path of the parent commit) against
              ``train.GraphedHomographyTrainer.step`` (one graph launch) at patch_size = 128, 1 x 256 x 256 frames, B = 16 and B = 64, host
              clock around ``--step-reps`` steps that end in a device synchronise; and the number of entry-point calls (``_lib.call``) the
              capture recorded -- torch's own launches (fills, the cat, the supervised MSE) are not among them;
    folder    ``homography_train.train_epoch``, the loop ``python -m hesic_amd.homography_train --cache device`` runs, per step, on 64
              synthetic 512 x 512 PNG pairs with batches of 16, with and without ``--graphed``'s trainer, under both supervisions: one epoch
              (four steps, ending in the read-back of the loss) per sample, the first two epochs of every variant left out (warm-up, capture);
    kernels   ``hesic_dropout_state_take`` and the ``_state`` forms of flatten + dropout at (B, 256, 128) and (B, 1, 1024), p = 0.5, next to
              the by-value entries on the same tensors, every one as the HIP-event time of ``--reps`` replays of a captured graph.

Writes profiles/homography_graphed_bench.json and prints it.  Run it under a time limit of its own:

    timeout -k 10 600 python profiles/scripts/homography_graphed_bench.py
"""
import argparse
import json
import os
import random
import sys
import tempfile
import time
from pathlib import Path

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)


def _med(v, digits=3):
    s = sorted(v)
    return {"median": round(s[len(s) // 2], digits), "min": round(s[0], digits), "max": round(s[-1], digits), "runs": len(s)}


def _verdict(eager, graphed):
    """Whether the replay beats the eager step by more than the eager step's own min-max spread over its runs."""
    gain, spread = eager["median"] - graphed["median"], eager["max"] - eager["min"]
    return {"gain_ms": round(gain, 3), "eager_spread_ms": round(spread, 3), "speedup": round(eager["median"] / graphed["median"], 3),
            "faster_beyond_spread": bool(gain > spread)}


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
            fn()
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        fn()
    return g


class _CountCalls:
    """Counts every ``_lib.call`` of the process while it is active -- the autograd threads' too, which the thread-local ``call_hook`` does
    not see."""

    def __enter__(self):
        from hesic_amd import _lib as L
        self.L, self.real, self.names = L, L.call, []

        def counting(name, *args):
            self.names.append(name)
            return self.real(name, *args)
        L.call = counting
        return self

    def __exit__(self, *exc):
        self.L.call = self.real


def steps(runs, step_reps, batches=(16, 64)):
    from hesic_amd import homography, synthetic, train
    rec, t, jobs = {}, {}, {}
    for B in batches:
        gen = torch.Generator().manual_seed(B)
        img_a = torch.rand((B, 1, 256, 256), generator=gen).cuda()
        patch_a, patch_b = img_a[:, :, 64:192, 64:192].contiguous(), torch.rand((B, 1, 128, 128), generator=gen).cuda()
        corners = (torch.full((B, 1, 2), 64.0) + torch.tensor([[0.0, 0.0], [128, 0.0], [128, 128], [0.0, 128]])).cuda()
        args = (img_a, patch_a, patch_b, corners)
        rec[f"B{B}"] = {}
        for name, cls in (("eager", train.HomographyTrainer), ("graphed", train.GraphedHomographyTrainer)):
            net = homography.Net(patch_size=128)
            synthetic.fill_homography_state_dict_(net.state_dict())
            tr = cls(net.cuda(), lr=1e-6, seed=0)
            if name == "graphed":
                for _ in range(tr.warmup):
                    tr.step(*args)
                with _CountCalls() as c:
                    tr.step(*args)                  # captures (and replays once)
                assert tr.graph_slot("step").graph is not None
                rec[f"B{B}"]["entry_calls_in_captured_graph"] = len(c.names)
                rec[f"B{B}"]["distinct_entry_points_in_captured_graph"] = len(set(c.names))
                args = tr.static_inputs("step")     # the producer's case: nothing is staged
            jobs[(B, name)], t[(B, name)] = (tr, args), []
    for _ in range(runs + 1):                       # run 0 is the warm-up of every variant
        for key, (tr, args) in jobs.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(step_reps):
                out = tr.step(*args)
            torch.cuda.synchronize()
            t[key].append((time.perf_counter() - t0) / step_reps * 1e3)
            rec[f"B{key[0]}"][f"{key[1]}_loss_finite"] = bool(torch.isfinite(out["loss"]))
    for B in batches:
        e, g = _med(t[(B, "eager")][1:]), _med(t[(B, "graphed")][1:])
        rec[f"B{B}"].update(eager_ms_per_step=e, graphed_ms_per_step=g, **_verdict(e, g))
    return rec


def _write_pairs(root, split, first_seed, n, side):
    from PIL import Image
    from hesic_amd import codec, synthetic
    for side_name in ("left", "right"):
        (root / split / side_name).mkdir(parents=True, exist_ok=True)
    for i0 in range(0, n, 8):
        x1, x2, _ = synthetic.stereo_batch(first_seed + i0, min(8, n - i0), side, side)
        for name, x in (("left", x1), ("right", x2)):
            for i, img in enumerate(codec.quantise(x)):
                Image.fromarray(img).save(root / split / name / f"pair{i0 + i:03d}.png")


def folder(runs, pairs=64, side=512, batch=16):
    from hesic_amd import homography, homography_train as HT, train
    rec = {"pairs": pairs, "side": side, "batch_size": batch, "steps_per_epoch": pairs // batch}
    with tempfile.TemporaryDirectory() as tmp:
        root = Path(tmp)
        _write_pairs(root, "train", 1000, pairs, side)
        a = HT.parser().parse_args([str(root), "--cache", "device", "--batch_size", str(batch)])
        listed = HT.list_pairs(a.root, "train")
        cache = HT.build_cache(a.root, "train", listed, a)
        jobs, t = {}, {}
        for sup in ("photometric", "synthetic"):
            for name, cls in (("eager", train.HomographyTrainer), ("graphed", train.GraphedHomographyTrainer)):
                torch.manual_seed(0)
                tr = cls(homography.Net(patch_size=a.patchsize).cuda(), lr=a.learning_rate, seed=0)
                jobs[(sup, name)], t[(sup, name)] = (tr, {}), []
        for epoch in range(runs + 2):               # epochs 0 and 1: warm-up and, for the graphed trainers, the capture
            for (sup, name), (tr, spare) in jobs.items():
                srng = random.Random(f"0/{epoch}/synth") if sup == "synthetic" else None
                _, n, secs = HT.train_epoch(tr, listed, a, random.Random(f"0/{epoch}"), torch.device("cuda", 0), cache, srng, spare)
                t[(sup, name)].append(secs / n * 1e3)
        for sup in ("photometric", "synthetic"):
            e, g = _med(t[(sup, "eager")][2:]), _med(t[(sup, "graphed")][2:])
            assert jobs[(sup, "graphed")][0].graph_slot("step" if sup == "photometric" else "supervised").graph is not None
            rec[sup] = dict(eager_ms_per_step=e, graphed_ms_per_step=g, **_verdict(e, g))
    return rec


def kernels(runs, reps, B):
    from hesic_amd import _lib as L
    from hesic_amd import functional as Fn
    rec = {}
    for HW, Cc, site in ((256, 128, 0), (1, 1024, 1)):
        x, g = torch.randn((B, HW, Cc), device="cuda"), torch.randn((B, HW * Cc), device="cuda")
        y, gx = torch.empty_like(g), torch.empty_like(x)
        cfg = Fn.dropout_args(0.5, 1, 0, site)
        state = Fn.dropout_state(1, 0, "cuda")
        taken = Fn.dropout_state_take(state)
        scfg = (cfg[0], cfg[1], L.ptr(taken), site)
        variants = {
            "dropout_state_take": lambda: L.call("hesic_dropout_state_take", L.ptr(state), L.ptr(taken), L.stream()),
            "forward": lambda: L.call("hesic_flatten_dropout_forward", L.ptr(x), L.ptr(y), B, HW, Cc, *cfg, L.F32, L.stream()),
            "forward_state": lambda: L.call("hesic_flatten_dropout_forward_state", L.ptr(x), L.ptr(y), B, HW, Cc, *scfg, L.F32, L.stream()),
            "backward": lambda: L.call("hesic_flatten_dropout_backward", L.ptr(g), L.ptr(gx), B, HW, Cc, *cfg, L.F32, L.stream()),
            "backward_state": lambda: L.call("hesic_flatten_dropout_backward_state", L.ptr(g), L.ptr(gx), B, HW, Cc, *scfg, L.F32, L.stream())}
        graphs = {k: _graph_of(fn) for k, fn in variants.items()}
        t = {k: [] for k in graphs}
        for _ in range(runs + 1):
            for k, gr in graphs.items():
                t[k].append(_event_us(gr.replay, reps))
        rec[f"{B}x{HW}x{Cc}"] = {k: {"us": _med(v[1:])} for k, v in t.items()}
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--step-reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "homography_graphed_bench.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("homography_graphed_bench: needs a ROCm device")
    rec = {"device": torch.cuda.get_device_name(0), "runs": a.runs, "reps_per_run": a.reps, "step_reps": a.step_reps,
           "step": steps(a.runs, a.step_reps)}
    rec["folder"] = folder(a.runs)
    for B in (16, 64):
        rec[f"kernels_B{B}"] = kernels(a.runs, a.reps, B)
    with open(a.out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print(json.dumps(rec))


if __name__ == "__main__":
    main()

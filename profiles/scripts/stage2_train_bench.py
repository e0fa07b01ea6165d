#!/usr/bin/env python3
"""What a stage-2 training step costs, one process on one box, warm, variants alternating, median of ``--runs`` (7):

    step      B = 8, 512 x 512, bf16 enhancer under f16 inference, wall-clock per step over ``--steps`` steps with one synchronisation at the end:
              * stage2_trainer: ``train.Stage2Trainer.step`` (the test vehicle, unchanged: torch Adam, per-layer mirror, torch criterion);
              * enhancer_trainer: ``train.EnhancerTrainer.step``;
              * graphed_enhancer_trainer: ``train.GraphedEnhancerTrainer.step`` (one graph launch);
              * folder_loop: ``train_stage2.train_epoch`` per step on a synthetic folder of 16 pairs from the device cache, the gather writing
                into the graphed step's static inputs.
    kernels   each new kernel as a graph replay (HIP events over ``--reps`` replays) against a device copy of the bytes it moves.
    elementwise  the launches between the convs of the training ``ResidualBlock``s that a later change could fold into the conv epilogues -- 36
              ``hesic_act_backward``, 24 forward skip adds, 24 gradient adds of autograd, all on (8, 32, 512, 512) 16-bit maps -- replayed ALONE
              as one graph at the step's shapes, as a share of the graphed step.  A model of the step's launches, not a trace of them.

Writes profiles/stage2_train_bench.json and prints it.  Run it under a time limit of its own:

    timeout -k 10 600 python profiles/scripts/stage2_train_bench.py
"""
import argparse
import json
import os
import sys
import tempfile
import time
from pathlib import Path

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
LAMBDA = 0.01


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


def _wall_ms(fn, steps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps * 1e3


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


def _alternate(variants, runs):
    t = {k: [] for k in variants}
    for _ in range(runs + 1):                        # run 0 is the warm-up of every variant
        for k, fn in variants.items():
            t[k].append(fn())
    return {k: _med(v[1:]) for k, v in t.items()}


def _enhancer():
    from hesic_amd import models, synthetic
    en = models.Independent_EN()
    synthetic.fill_state_dict_(en.state_dict())
    return en.cuda()


def steps(runs, nsteps, B, size, tmp):
    from PIL import Image
    from hesic_amd import codec, pair_cache, synthetic, train, train_stage2
    x1, x2, Hm = (t.cuda() for t in synthetic.stereo_batch(0, B, size, size))
    # a frozen model per variant: a replay starts a new pack-cache epoch, which would make the eager variants repack a shared model's weights
    nets = [codec.load_model(None, torch.float16) for _ in range(4)]
    old = train.Stage2Trainer(nets[0], _enhancer(), lr=1e-4, lmbda=LAMBDA)
    eager = train.EnhancerTrainer(nets[1], _enhancer(), lr=1e-4, lmbda=LAMBDA)
    graphed = train.GraphedEnhancerTrainer(nets[2], _enhancer(), lr=1e-4, lmbda=LAMBDA)
    loop = train.GraphedEnhancerTrainer(nets[3], _enhancer(), lr=1e-4, lmbda=LAMBDA)
    n = 2 * B
    a, b, Hs = synthetic.stereo_batch(100, n, size, size)
    for side, x in (("left", a), ("right", b)):
        d = Path(tmp) / "train" / side
        d.mkdir(parents=True)
        for i, img in enumerate(codec.quantise(x)):
            Image.fromarray(img).save(d / f"{i:03d}.png")
    (Path(tmp) / "train" / "H").mkdir()
    for i in range(n):
        np.save(Path(tmp) / "train" / "H" / f"{i:03d}.npy", Hs[i].double().numpy())
    cache = pair_cache.DevicePairCache(tmp, "train", mode="device")
    epoch = [0]

    def folder_loop():
        torch.cuda.synchronize()
        t0, done = time.perf_counter(), 0
        while done < nsteps:
            plan = pair_cache.epoch_plan(len(cache), cache.sizes, B, size, size, 0, epoch[0], True, True)
            epoch[0] += 1
            done += train_stage2.train_epoch(loop, cache, plan, size, size)[1]       # its read-back synchronises
        return (time.perf_counter() - t0) / done * 1e3

    variants = {"stage2_trainer": lambda: _wall_ms(lambda: old.step(x1, x2, Hm), nsteps),
                "enhancer_trainer": lambda: _wall_ms(lambda: eager.step(x1, x2, Hm), nsteps),
                "graphed_enhancer_trainer": lambda: _wall_ms(lambda: graphed.step(x1, x2, Hm), nsteps),
                "folder_loop": folder_loop}
    rec = {"shape": {"B": B, "H": size, "W": size, "inference": "f16", "training": "bf16"}, "steps_per_run": nsteps}
    for k, v in _alternate(variants, runs).items():
        rec[k + "_ms"] = v
    base = rec["stage2_trainer_ms"]["median"]
    for k in ("enhancer_trainer", "graphed_enhancer_trainer", "folder_loop"):
        rec[k + "_over_stage2_trainer"] = round(rec[k + "_ms"]["median"] / base, 3)
    assert graphed.graph is not None and loop.graph is not None
    return rec


def kernels(runs, reps, B, size):
    import hesic_amd
    from hesic_amd import functional as Fn
    from hesic_amd import synthetic
    keep = Fn.compute_dtype()
    hesic_amd.set_compute_dtype(torch.bfloat16)
    try:
        x1, x2, _ = (t.cuda() for t in synthetic.stereo_batch(0, B, size, size))
        y1, y2 = (x1 + 0.01).contiguous(), (x2 - 0.01).contiguous()
        k = LAMBDA * 255 ** 2
        out = torch.empty(4, dtype=torch.float64, device="cuda")
        ws = torch.empty(1 << 16, dtype=torch.uint8, device="cuda")
        maps = [torch.empty((B, size, size, 32), dtype=torch.bfloat16, device="cuda").permute(0, 3, 1, 2) for _ in range(2)]
        en = _enhancer()
        ws_ = [p.detach() for p in en.parameters() if p.dim() == 4]
        entries, so, do = [], 0, 0
        for w in ws_:
            entries.append((so, do, w.shape[0], w.shape[1], 32))
            so += -(-w.numel() // 64) * 64
            do += -(-w.shape[1] * 32 * 9 // 64) * 64
        src = torch.zeros(so, device="cuda")
        dst = torch.empty(do, device="cuda")
        table = Fn.mirror_table(entries, "cuda")
        moved = {"en_loss": 4 * x1.numel() * 4, "en_loss_grad": 4 * x1.numel() * 4 + 2 * maps[0].numel() * 2,
                 "c32_mirror_weights": sum(w.numel() for w in ws_) * 4 + sum(e[3] * 32 * 9 for e in entries) * 4}
        calls = {"en_loss": lambda: Fn.en_loss(y1, x1, y2, x2, k, out=out, ws=ws),
                 "en_loss_grad": lambda: Fn.en_loss_grad(y1, x1, y2, x2, k, out=maps),
                 "c32_mirror_weights": lambda: Fn.c32_mirror_weights(src, dst, table, len(entries))}
        variants, copies = {}, {}
        for name, fn in calls.items():
            g = _graph_of(fn)
            a = torch.empty(moved[name] // 8, dtype=torch.float32, device="cuda").normal_()        # a copy moves 2 x its size
            c = torch.empty_like(a)
            gc = _graph_of(lambda a=a, c=c: c.copy_(a))
            copies[name] = (a, c)
            variants[name] = lambda g=g: _event_us(g.replay, reps)
            variants[name + "_copy"] = lambda gc=gc: _event_us(gc.replay, reps)
        res = _alternate(variants, runs)
        rec = {}
        for name in calls:
            rec[name] = {"bytes_moved": moved[name], "us": res[name], "copy_us": res[name + "_copy"],
                         "times_the_copy": round(res[name]["median"] / res[name + "_copy"]["median"], 2),
                         "gb_per_s": round(moved[name] / res[name]["median"] / 1e3, 1)}
        # the elementwise launches between the convs, at the step's shapes, alone
        from hesic_amd import _lib as L
        t = [torch.empty((B, size, size, 32), dtype=torch.bfloat16, device="cuda").normal_().permute(0, 3, 1, 2) for _ in range(3)]

        def elementwise():
            for _ in range(36):
                L.call("hesic_act_backward", L.ptr(t[0]), L.ptr(t[1]), L.ptr(t[2]), t[0].numel(), L.ACT_LEAKY, L.dt(t[0]), L.stream())
            for _ in range(48):
                torch.add(t[0], t[1], out=t[2])

        ge = _graph_of(elementwise)
        rec["elementwise_between_convs_us"] = _alternate({"e": lambda: _event_us(ge.replay, max(reps // 20, 5))}, runs)["e"]
        return rec
    finally:
        hesic_amd.set_compute_dtype(keep)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "stage2_train_bench.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("stage2_train_bench: needs a ROCm device")
    with tempfile.TemporaryDirectory() as tmp:
        rec = {"device": torch.cuda.get_device_name(0), "runs": a.runs, "reps_per_run": a.reps,
               "step": steps(a.runs, a.steps, a.batch, a.size, tmp), "kernels": kernels(a.runs, a.reps, a.batch, a.size)}
    share = rec["kernels"]["elementwise_between_convs_us"]["median"] / 1e3 / rec["step"]["graphed_enhancer_trainer_ms"]["median"]
    rec["elementwise_share_of_the_graphed_step"] = round(share, 3)
    with open(a.out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print(json.dumps(rec))


if __name__ == "__main__":
    main()

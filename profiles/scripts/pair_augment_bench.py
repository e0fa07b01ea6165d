#!/usr/bin/env python3
"""What the stereo-aware augmentation in the pair gather costs, one process on one box, warm, median of ``--runs`` (7), variants alternating
(the workload and the helpers are train_folder_bench.py's):

    gather    B = 8, 512 x 512 crops out of 860 x 1080 stored images, the HIP-event time of ``--reps`` replays of a captured graph of
              * old / old_again: ``hesic_pair_batch_gather`` -- the yardstick, measured twice per round so that the spread of its own repeated
                medians is on record;
              * aug_0 .. aug_7:  ``hesic_pair_batch_gather_aug`` with every item carrying that flag value (1 hflip, 2 vflip, 4 swap);
              * aug_mixed:       the new entry with item b carrying flags b (what an augmented epoch launches);
              * copy:            a plain device copy of as many bytes (2 x 8 x 512^2 x 3 read, four times that written).
              ``over_old`` is a variant's median over the old entry's; ``old_spread`` the old entry's own old_again / old.
    step      seconds per training step at B = 8, 512 x 512, bf16, ``GraphedTrainer``, ``train_folder.train_epoch`` on a
              ``DevicePairCache(mode="device")`` over a generated folder of 64 pairs of 860 x 1080, per epoch of 8 steps from the second epoch
              on: the plan without augmentation (measured twice per round) against the plan with all three flags.

Every stage runs under a time limit of its own (``--limit`` seconds, SIGALRM).  Writes profiles/pair_augment_bench.json and prints it.  Run it
under a time limit too:

    timeout -k 10 900 python profiles/scripts/pair_augment_bench.py
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

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from train_folder_bench import ROOT, _Limit, _event_us, _graph_of, _med, _smooth_pairs  # noqa: E402

ALL = ("hflip", "vflip", "swap")


def gather(runs, reps, limit, B=8, P=512, H=860, W=1080):
    from hesic_amd import _lib as L
    from hesic_amd import functional as Fn
    g = np.random.Generator(np.random.PCG64(0))
    stored = torch.from_numpy(g.integers(0, 256, size=(2 * B, H, W, 3), dtype=np.uint8)).cuda()
    table = torch.from_numpy(np.tile(np.eye(3).reshape(1, 9), (B, 1)) + g.normal(0, 1e-3, size=(B, 9))).cuda()
    items = Fn.pair_items(B)
    for b in range(B):
        it = items[b]
        it["left"], it["right"], it["pitch_px"], it["rows"] = stored[2 * b].data_ptr(), stored[2 * b + 1].data_ptr(), W, H
        it["x0"], it["y0"], it["h_index"] = int(g.integers(0, W - P)), int(g.integers(0, H - P)), b
        it["hx"], it["hy"] = it["x0"], it["y0"]
    out = [torch.empty(s, device="cuda") for s in [(B, 3, P, P), (B, 3, P, P), (B, 3, 3)]]
    nbytes = 2 * B * P * P * 3 * 5
    src = torch.empty(nbytes // 8, dtype=torch.float32, device="cuda").normal_()          # a copy moves 2 x its size
    dst = torch.empty_like(src)

    def graph(entry, flags):
        it = items.copy()
        it["reserved"] = flags
        Fn.check_pair_items(it, B, P, P, Fn.PAIR_FLAG_MASK if entry.endswith("_aug") else 0)
        dev = torch.from_numpy(it.view(np.uint8).reshape(B, 48)).cuda()
        keep.append(dev)
        return _graph_of(lambda: L.call(entry, L.ptr(dev), L.ptr(table), B, P, P, *[L.ptr(t) for t in out], L.stream())).replay

    keep = []
    with _Limit(limit, "gather capture"):
        variants = {"old": graph("hesic_pair_batch_gather", 0)}
        for f in range(8):
            variants[f"aug_{f}"] = graph("hesic_pair_batch_gather_aug", f)
        variants["aug_mixed"] = graph("hesic_pair_batch_gather_aug", list(range(8)) * (B // 8))
        variants["old_again"] = graph("hesic_pair_batch_gather", 0)
        variants["copy"] = lambda: dst.copy_(src)
    t = {k: [] for k in variants}
    with _Limit(limit, "gather timing"):
        for _ in range(runs + 1):                # run 0 is the warm-up of every variant
            for k, fn in variants.items():
                t[k].append(_event_us(fn, reps))
    rec = {"shape": {"B": B, "crop": [P, P], "stored": [H, W]}, "bytes": nbytes, "graph_replay_us": {k: _med(v[1:]) for k, v in t.items()}}
    old = rec["graph_replay_us"]["old"]["median"]
    rec["over_old"] = {k: round(v["median"] / old, 3) for k, v in rec["graph_replay_us"].items() if k not in ("old", "copy")}
    rec["old_spread"] = {"old_again_over_old": rec["over_old"]["old_again"],
                         "min_over_median": round(rec["graph_replay_us"]["old"]["min"] / old, 3),
                         "max_over_median": round(rec["graph_replay_us"]["old"]["max"] / old, 3)}
    rec["times_the_copy"] = {k: round(v["median"] / rec["graph_replay_us"]["copy"]["median"], 2) for k, v in rec["graph_replay_us"].items() if k != "copy"}
    return rec


def steps(runs, limit, B=8, P=512, H=860, W=1080, pairs=64):
    from PIL import Image
    import hesic_amd
    from hesic_amd import models, pair_cache, synthetic, train, train_folder
    rec = {"shape": {"B": B, "crop": [P, P], "stored": [H, W], "pairs": pairs, "steps_per_epoch": pairs // B, "dtype": "bf16", "graphed": True}}
    with tempfile.TemporaryDirectory() as tmp:
        with _Limit(limit, "writing the folder"):
            for c0 in range(0, pairs, 16):
                a, b = _smooth_pairs(16, H, W, 1 + c0)
                for d in ("left", "right", "H"):
                    (Path(tmp) / "train" / d).mkdir(parents=True, exist_ok=True)
                for i in range(16):
                    Image.fromarray(a[i]).save(Path(tmp) / "train" / "left" / f"{c0 + i:03d}.png")
                    Image.fromarray(b[i]).save(Path(tmp) / "train" / "right" / f"{c0 + i:03d}.png")
                    np.save(Path(tmp) / "train" / "H" / f"{c0 + i:03d}.npy", synthetic.homography(c0 + i).astype(np.float64))
        hesic_amd.set_compute_dtype(torch.bfloat16)
        net = models.HSIC()
        synthetic.fill_state_dict_(net.state_dict())
        tr = train.GraphedTrainer(net.cuda().train(), lr=1e-6, aux_lr=1e-6, lmbda=1e-2)
        with _Limit(limit, "decoding into the device cache"):
            dev = pair_cache.DevicePairCache(tmp, "train", mode="device", workers=3)

        def epoch(e, augment):
            plan = pair_cache.epoch_plan(len(dev), dev.sizes, B, P, P, 0, e, True, True, augment=augment)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            _, n, _ = train_folder.train_epoch(tr, dev, plan, P, P)             # ends in the epoch's read-back
            return (time.perf_counter() - t0) / n * 1e3, plan.augmented()

        variants = {"none": (), "all_flags": ALL, "none_again": ()}
        t, counts = {k: [] for k in variants}, []
        for e in range(runs + 1):                # epoch 0 is the warm-up of every variant (and holds the capture)
            for k, augment in variants.items():
                with _Limit(limit, f"{k} epoch {e}"):
                    ms, c = epoch(e, augment)
                    t[k].append(ms)
                    if k == "all_flags" and e:
                        counts.append(c)
    for k in variants:
        rec[k + "_ms_per_step"] = _med(t[k][1:])
    none = rec["none_ms_per_step"]["median"]
    rec["all_flags_over_none"] = round(rec["all_flags_ms_per_step"]["median"] / none, 3)
    rec["none_again_over_none"] = round(rec["none_again_ms_per_step"]["median"] / none, 3)
    rec["flagged_items_of_the_timed_epochs"] = {k: sum(c[k] for c in counts) for k in ALL}
    rec["items_of_the_timed_epochs"] = runs * pairs
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--limit", type=int, default=240, help="seconds every stage may take")
    ap.add_argument("--only", choices=("gather", "steps"), default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pair_augment_bench.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("pair_augment_bench: needs a ROCm device")
    rec = {"device": torch.cuda.get_device_name(0), "runs": a.runs, "reps_per_run": a.reps}
    if a.only != "steps":
        rec["gather"] = gather(a.runs, a.reps, a.limit)
    if a.only != "gather":
        rec["steps"] = steps(a.runs, a.limit)
    with open(a.out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print(json.dumps(rec))


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""What feeding HSIC's training step from a folder costs, one process on one box, warm, median of ``--runs`` (7), variants alternating:

    gather    ``hesic_pair_batch_gather`` at B = 8, 512 x 512 crops out of 860 x 1080 stored images: the HIP-event time of ``--reps`` replays of
              a captured graph, next to a plain device copy of as many bytes (2 x 8 x 512^2 x 3 read, four times that written) -- the
              ratio to the copy is the figure to read;
    step      seconds per training step at B = 8, 512 x 512, bf16, ``GraphedTrainer``, on a generated folder of 64 pairs of 860 x 1080, per
              epoch of 8 steps, from the second epoch on:
              * device: ``train_folder.train_epoch`` on a ``DevicePairCache(mode="device")``;
              * stream: the same on ``mode="stream"``;
              * floor:  the trainer's step alone on a resident batch;
              * loader: the route that existed before -- ``compressai.datasets.ImageFolder`` behind ``DataLoader(num_workers=3)``, fp32
                batches uploaded per step -- feeding the same trainer;
              and the seconds the first epoch's decode into the device arena took.

Every stage runs under a time limit of its own (``--limit`` seconds, SIGALRM).  Writes profiles/train_folder_bench.json and prints it.  Run it
under a time limit too:

    timeout -k 10 900 python profiles/scripts/train_folder_bench.py
"""
import argparse
import json
import os
import signal
import sys
import tempfile
import time
from pathlib import Path

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)


def _med(v, nd=3):
    s = sorted(v)
    return {"median": round(s[len(s) // 2], nd), "min": round(s[0], nd), "max": round(s[-1], nd), "runs": len(s)}


class _Limit:
    def __init__(self, seconds, what):
        self.seconds, self.what = int(seconds), what

    def _fire(self, *_):
        raise SystemExit(f"train_folder_bench: {self.what} exceeded its limit of {self.seconds} s")

    def __enter__(self):
        signal.signal(signal.SIGALRM, self._fire)
        signal.alarm(self.seconds)

    def __exit__(self, *exc):
        signal.alarm(0)
        return False


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


def _smooth_pairs(n, h, w, seed):
    """uint8 (n, h, w, 3) pairs with image-like content: a coarse random grid upsampled, the right view shifted by a few pixels."""
    g = np.random.Generator(np.random.PCG64(seed))
    coarse = torch.from_numpy(g.random((n, 3, h // 16 + 2, w // 16 + 2), dtype=np.float32))
    big = torch.nn.functional.interpolate(coarse, size=(h + 16, w + 16), mode="bicubic", align_corners=False).clamp(0, 1)
    big = (big + 0.03 * torch.from_numpy(g.standard_normal(big.shape, dtype=np.float32))).clamp(0, 1)
    q = (big * 255).round().to(torch.uint8).permute(0, 2, 3, 1).numpy()
    return np.ascontiguousarray(q[:, 4:4 + h, 4:4 + w]), np.ascontiguousarray(q[:, 7:7 + h, 10:10 + w])


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
    Fn.check_pair_items(items, B, P, P)
    items_dev = torch.from_numpy(items.view(np.uint8).reshape(B, 48)).cuda()
    out = [torch.empty(s, device="cuda") for s in [(B, 3, P, P), (B, 3, P, P), (B, 3, 3)]]
    nbytes = 2 * B * P * P * 3 * 5
    src = torch.empty(nbytes // 8, dtype=torch.float32, device="cuda").normal_()          # a copy moves 2 x its size
    dst = torch.empty_like(src)
    with _Limit(limit, "gather capture"):
        graph = _graph_of(lambda: L.call("hesic_pair_batch_gather", L.ptr(items_dev), L.ptr(table), B, P, P, *[L.ptr(t) for t in out], L.stream()))
    tg, tc = [], []
    with _Limit(limit, "gather timing"):
        for _ in range(runs + 1):                # run 0 is the warm-up of both
            tg.append(_event_us(graph.replay, reps))
            tc.append(_event_us(lambda: dst.copy_(src), reps))
    gr, cp = _med(tg[1:]), _med(tc[1:])
    return {"shape": {"B": B, "crop": [P, P], "stored": [H, W]}, "bytes": nbytes, "graph_replay_us": gr, "copy_same_bytes_us": cp,
            "times_the_copy": round(gr["median"] / cp["median"], 2), "gather_GBps": round(nbytes / gr["median"] / 1e3, 1)}


def steps(runs, limit, B=8, P=512, H=860, W=1080, pairs=64):
    from PIL import Image
    import hesic_amd
    from hesic_amd import models, pair_cache, synthetic, train, train_folder
    from hesic_amd.compressai.datasets import ImageFolder, to_tensor
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
        stream = pair_cache.DevicePairCache(tmp, "train", mode="stream", workers=3)
        rec["decode_seconds"] = round(dev.decode_seconds, 3)
        rec["arena_bytes"] = int(dev.arena.numel())
        ds = ImageFolder(tmp, transform=to_tensor, patch_size=(P, P), split="train")

        def epoch(cache, e):
            plan = pair_cache.epoch_plan(len(cache), cache.sizes, B, P, P, 0, e, True, True)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            _, n, _ = train_folder.train_epoch(tr, cache, plan, P, P)          # ends in the epoch's read-back
            return (time.perf_counter() - t0) / n * 1e3

        def floor(e):
            x = tr.static_inputs()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(pairs // B):
                tr.step(*x)
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) / (pairs // B) * 1e3

        def loader(e):
            dl = torch.utils.data.DataLoader(ds, batch_size=B, num_workers=3, shuffle=True, pin_memory=False, drop_last=True)
            torch.cuda.synchronize()
            t0, n = time.perf_counter(), 0
            for d in dl:
                tr.step(d[0].cuda(), d[1].cuda(), d[2].cuda())
                n += 1
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) / n * 1e3

        variants = {"device": lambda e: epoch(dev, e), "stream": lambda e: epoch(stream, e), "floor": floor, "loader": loader}
        t = {k: [] for k in variants}
        for e in range(runs + 1):                # epoch 0 is the warm-up of every variant (and holds the capture)
            for k, fn in variants.items():
                with _Limit(limit, f"{k} epoch {e}"):
                    t[k].append(fn(e))
    for k in variants:
        rec[k + "_ms_per_step"] = _med(t[k][1:])
    fl = rec["floor_ms_per_step"]["median"]
    for k in ("device", "stream", "loader"):
        rec[k + "_over_floor"] = round(rec[k + "_ms_per_step"]["median"] / fl, 2)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--limit", type=int, default=240, help="seconds every stage may take")
    ap.add_argument("--only", choices=("gather", "steps"), default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "train_folder_bench.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("train_folder_bench: needs a ROCm device")
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

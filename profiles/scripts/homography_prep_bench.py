#!/usr/bin/env python3
"""What turning a stereo batch into HomographyNet's inputs costs, one process on one box, warm, median of ``--runs`` (7), variants alternating:

    prepare   ``homography.prepare_inputs`` at B = 8, 3 x 512 x 512 -> 256 x 256 with 128 x 128 windows, uint8 and float32 input:
              * eager: the public call (window draw, the (B, 2) origins' upload, one launch), host clock around ``--reps`` calls that end in
                a device synchronise;
              * graph: ``functional.homonet_prepare`` (the launch alone) as the HIP-event time of ``--reps`` replays of a captured graph,
                next to the bytes it has to move (every input sample once, every output once) and the time a plain device copy of as many
                bytes takes on this box -- the ratio to the copy is the figure to read;
              * host: the route that existed before for the same eight pairs -- ``ImageFolder._homonet_inputs`` per item in torch CPU ops
                plus the upload of its results -- on the host clock;
    folder    the wall time per training step of ``python -m hesic_amd.homography_train``'s epoch loop (PNG reading, stacking, the bytes'
              upload, ``step_pairs``) against ``HomographyTrainer.step`` alone on resident inputs, B = 16, patch_size = 128, 512 x 512 pairs.

Writes profiles/homography_prep_bench.json and prints it.  Run it under a time limit of its own:

    timeout -k 10 600 python profiles/scripts/homography_prep_bench.py
"""
import argparse
import json
import os
import random
import sys
import tempfile
import time
from pathlib import Path

import numpy as np
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


def _host_us(fn, reps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps * 1e6


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


def prepare(runs, reps, host_reps, B=8, H=512, W=512, S=256, P=128, rho=45):
    from hesic_amd import functional as Fn
    from hesic_amd import homography
    from hesic_amd.compressai.datasets import MEAN, STD, ImageFolder
    a, b = _smooth_pairs(B, H, W, 0)
    u1, u2 = (torch.from_numpy(v).cuda().permute(0, 3, 1, 2) for v in (a, b))               # the folder trainer's layout
    f1, f2 = (v.float().div(255.0).contiguous() for v in (u1, u2))                           # HSIC.forward's inputs
    xy = torch.tensor(homography.window_origins(B, "centre", S, P), dtype=torch.int32).cuda()
    out = [torch.empty(s, device="cuda") for s in [(B, 1, S, S), (B, 1, S, S), (B, 1, P, P), (B, 1, P, P), (B, 4, 2)]]
    out_bytes = sum(t.numel() for t in out) * 4 + xy.numel() * 4
    ds = object.__new__(ImageFolder)
    ds.homopic_size, ds.homopatch_size, ds.rho = S, P, rho

    def host_route():
        items = [ds._homonet_inputs(a[i], b[i]) for i in range(B)]
        return [torch.stack([it[k] for it in items]).cuda() for k in range(3)]

    variants = {}
    for name, (x1, x2) in (("uint8", (u1, u2)), ("float32", (f1, f2))):
        nbytes = 2 * x1.numel() * x1.element_size() + out_bytes
        g = _graph_of(lambda x1=x1, x2=x2: Fn.homonet_prepare(x1, x2, xy, S, P, float(MEAN), float(STD), out=out))
        src = torch.empty(nbytes // 8, dtype=torch.float32, device="cuda").normal_()          # a copy moves 2 x its size
        dst = torch.empty_like(src)
        variants[name] = {"graph": (lambda g=g: _event_us(g.replay, reps)), "copy": (lambda src=src, dst=dst: _event_us(lambda: dst.copy_(src), reps)),
                          "eager": (lambda x1=x1, x2=x2: _host_us(lambda: homography.prepare_inputs(x1, x2, None, S, P, rho), reps)),
                          "bytes": nbytes}
    t = {(n, k): [] for n in variants for k in ("graph", "copy", "eager")}
    th = []
    for _ in range(runs + 1):                    # run 0 is the warm-up of every variant
        for n, v in variants.items():
            for k in ("graph", "copy", "eager"):
                t[(n, k)].append(v[k]())
        th.append(_host_us(host_route, host_reps))
    rec = {"shape": {"B": B, "H": H, "W": W, "pic_size": S, "patch_size": P}, "host_route_us": _med(th[1:])}
    for n, v in variants.items():
        gr, cp, ea = _med(t[(n, "graph")][1:]), _med(t[(n, "copy")][1:]), _med(t[(n, "eager")][1:])
        rec[n] = {"bytes": v["bytes"], "graph_replay_us": gr, "copy_same_bytes_us": cp, "times_the_copy": round(gr["median"] / cp["median"], 2),
                  "eager_call_us": ea, "host_route_over_eager": round(rec["host_route_us"]["median"] / ea["median"], 1)}
    return rec


def folder(runs, B=16, H=512, W=512, steps_per_run=4):
    from PIL import Image
    from hesic_amd import homography, homography_train, synthetic, train
    with tempfile.TemporaryDirectory() as tmp:
        a, b = _smooth_pairs(B * steps_per_run, H, W, 1)
        for side, x in (("left", a), ("right", b)):
            d = Path(tmp) / "train" / side
            d.mkdir(parents=True)
            for i, img in enumerate(x):
                Image.fromarray(img).save(d / f"{i:03d}.png")
        args = homography_train.parser().parse_args([tmp, "--batch_size", str(B)])
        pairs = homography_train.list_pairs(tmp, "train")
        net = homography.Net(patch_size=128)
        synthetic.fill_homography_state_dict_(net.state_dict())
        tr = train.HomographyTrainer(net.cuda(), lr=1e-6, seed=0)
        x1, x2 = (torch.from_numpy(v[:B]).cuda().permute(0, 3, 1, 2) for v in (a, b))
        grey1, _, p1, p2, corners = homography.prepare_inputs(x1, x2, "centre")
        t_folder, t_pairs, t_step = [], [], []
        for r in range(runs + 1):
            _, n, secs = homography_train.train_epoch(tr, pairs, args, random.Random(r), torch.device("cuda"))
            t_folder.append(secs / n * 1e3)
            t_pairs.append(_host_us(lambda: tr.step_pairs(x1, x2, "centre"), steps_per_run) / 1e3)
            t_step.append(_host_us(lambda: tr.step(grey1, p1, p2, corners), steps_per_run) / 1e3)
    rec = {"shape": {"B": B, "H": H, "W": W, "patch_size": 128, "steps_per_run": steps_per_run},
           "folder_ms_per_step": _med(t_folder[1:]), "step_pairs_resident_ms": _med(t_pairs[1:]), "step_alone_ms": _med(t_step[1:])}
    rec["folder_over_step"] = round(rec["folder_ms_per_step"]["median"] / rec["step_alone_ms"]["median"], 2)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--host-reps", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "homography_prep_bench.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("homography_prep_bench: needs a ROCm device")
    rec = {"device": torch.cuda.get_device_name(0), "runs": a.runs, "reps_per_run": a.reps, "prepare": prepare(a.runs, a.reps, a.host_reps),
           "folder": folder(a.runs)}
    with open(a.out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print(json.dumps(rec))


if __name__ == "__main__":
    main()

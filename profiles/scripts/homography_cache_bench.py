#!/usr/bin/env python3
"""What feeding HomographyNet from stored uint8 images costs, one process on one box, warm, median of ``--runs`` (7), variants alternating:

    kernel    B = 8 whole 512 x 512 uint8 HWC images -> 256 x 256 with 128 x 128 windows, as the HIP-event time of ``--reps`` replays of a
              captured graph that holds the launch alone:
              * items:   ``hesic_homonet_prepare_items`` on eight separately stored pairs (descriptors resident);
              * strided: ``hesic_homonet_prepare`` on the same images stacked as one (B, H, W, 3) tensor viewed as (B, 3, H, W);
              * copy:    a plain device copy of as many bytes as the launch has to move (every input sample once, every output once);
              the two forms' outputs are compared bit for bit first.  Next to them the eager public calls on the host clock
              (``functional.homonet_prepare_items``: host checks, descriptor upload, launch).
    loop      the wall time per training step of ``python -m hesic_amd.homography_train``'s epoch loop under ``--cache host`` (PNG reading
              on one thread, stacking, the bytes' upload, ``step_pairs``), ``device`` and ``stream``, against ``HomographyTrainer.step``
              alone on resident inputs: B = 16, patch_size = 128, 512 x 512 pairs; ``decode_seconds`` of the set.
    mixed     one epoch over a folder of two image sizes under ``--cache device`` with and without ``--mix-sizes``: steps and seconds.

Writes profiles/homography_cache_bench.json and prints it.  Run it under a time limit of its own:

    timeout -k 10 600 python profiles/scripts/homography_cache_bench.py
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
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from homography_prep_bench import _event_us, _graph_of, _host_us, _med, _smooth_pairs  # noqa: E402


def _write(root, split, a, b, start=0):
    from PIL import Image
    for side, x in (("left", a), ("right", b)):
        d = Path(root) / split / side
        d.mkdir(parents=True, exist_ok=True)
        for i, img in enumerate(x):
            Image.fromarray(img).save(d / f"{start + i:03d}.png")


def kernel(runs, reps, B=8, H=512, W=512, S=256, P=128):
    from hesic_amd import _lib as L
    from hesic_amd import functional as Fn
    from hesic_amd import homography
    from hesic_amd.compressai.datasets import MEAN, STD
    a, b = _smooth_pairs(B, H, W, 0)
    s1, s2 = torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda()                    # stacked (B, H, W, 3): the strided form's input
    u1, u2 = s1.permute(0, 3, 1, 2), s2.permute(0, 3, 1, 2)
    stored = [(torch.from_numpy(a[i]).cuda(), torch.from_numpy(b[i]).cuda()) for i in range(B)]      # eight allocations of their own
    windows = homography.window_origins(B, "centre", S, P)
    xy = torch.tensor(windows, dtype=torch.int32).cuda()
    items = Fn.homonet_items(B)
    for i, ((l, r), (wx, wy)) in enumerate(zip(stored, windows)):
        items[i] = (l.data_ptr(), r.data_ptr(), W, H, 0, 0, W, H, wx, wy)
    items_dev = torch.from_numpy(items.view("uint8").reshape(B, 48)).cuda()
    shapes = [(B, 1, S, S), (B, 1, S, S), (B, 1, P, P), (B, 1, P, P), (B, 4, 2)]
    out_i, out_s = ([torch.empty(s, device="cuda") for s in shapes] for _ in range(2))

    def launch_items():
        L.call("hesic_homonet_prepare_items", L.ptr(items_dev), B, S, P, float(MEAN), float(STD), *[L.ptr(t) for t in out_i], L.stream())

    def launch_strided():
        Fn.homonet_prepare(u1, u2, xy, S, P, float(MEAN), float(STD), out=out_s)

    launch_items()
    launch_strided()
    torch.cuda.synchronize()
    same = all(torch.equal(x, y) for x, y in zip(out_i, out_s))
    out_bytes = sum(t.numel() for t in out_i) * 4
    nbytes = 2 * s1.numel() + out_bytes + items_dev.numel()
    src = torch.empty(nbytes // 8, dtype=torch.float32, device="cuda").normal_()           # a copy moves 2 x its size
    dst = torch.empty_like(src)
    gi, gs = _graph_of(launch_items), _graph_of(launch_strided)
    variants = {"items_graph_replay_us": lambda: _event_us(gi.replay, reps), "strided_graph_replay_us": lambda: _event_us(gs.replay, reps),
                "copy_same_bytes_us": lambda: _event_us(lambda: dst.copy_(src), reps),
                "items_eager_call_us": lambda: _host_us(lambda: Fn.homonet_prepare_items(items, S, P, float(MEAN), float(STD), out=out_i), reps),
                "strided_eager_call_us": lambda: _host_us(launch_strided, reps)}
    t = {k: [] for k in variants}
    for _ in range(runs + 1):                    # run 0 is the warm-up of every variant
        for k, fn in variants.items():
            t[k].append(fn())
    rec = {"shape": {"B": B, "H": H, "W": W, "pic_size": S, "patch_size": P}, "bytes": nbytes, "outputs_equal_bit_for_bit": bool(same)}
    rec.update({k: _med(v[1:]) for k, v in t.items()})
    rec["items_times_the_copy"] = round(rec["items_graph_replay_us"]["median"] / rec["copy_same_bytes_us"]["median"], 2)
    rec["strided_times_the_copy"] = round(rec["strided_graph_replay_us"]["median"] / rec["copy_same_bytes_us"]["median"], 2)
    rec["items_over_strided"] = round(rec["items_graph_replay_us"]["median"] / rec["strided_graph_replay_us"]["median"], 3)
    return rec


def _trainer():
    from hesic_amd import homography, synthetic, train
    net = homography.Net(patch_size=128)
    synthetic.fill_homography_state_dict_(net.state_dict())
    return train.HomographyTrainer(net.cuda(), lr=1e-6, seed=0)


def loop(runs, B=16, H=512, W=512, steps_per_run=4):
    from hesic_amd import homography, homography_train
    dev = torch.device("cuda")
    with tempfile.TemporaryDirectory() as tmp:
        a, b = _smooth_pairs(B * steps_per_run, H, W, 1)
        _write(tmp, "train", a, b)
        pairs = homography_train.list_pairs(tmp, "train")
        args = {m: homography_train.parser().parse_args([tmp, "--batch_size", str(B), "--cache", m]) for m in ("host", "device", "stream")}
        caches = {"host": None, "device": homography_train.build_cache(tmp, "train", pairs, args["device"]),
                  "stream": homography_train.build_cache(tmp, "train", pairs, args["stream"])}
        tr = _trainer()
        x1, x2 = (torch.from_numpy(v[:B]).cuda().permute(0, 3, 1, 2) for v in (a, b))
        grey1, _, p1, p2, corners = homography.prepare_inputs(x1, x2, "centre")
        t = {m: [] for m in args}
        t_step = []
        for r in range(runs + 1):
            for m in args:
                _, n, secs = homography_train.train_epoch(tr, pairs, args[m], random.Random(r), dev, caches[m])
                t[m].append(secs / n * 1e3)
            t_step.append(_host_us(lambda: tr.step(grey1, p1, p2, corners), steps_per_run) / 1e3)
        decode = caches["device"].decode_seconds
    rec = {"shape": {"B": B, "H": H, "W": W, "patch_size": 128, "steps_per_run": steps_per_run, "pairs": B * steps_per_run, "workers": 3},
           "host_ms_per_step": _med(t["host"][1:]), "device_ms_per_step": _med(t["device"][1:]), "stream_ms_per_step": _med(t["stream"][1:]),
           "step_alone_ms": _med(t_step[1:]), "decode_seconds": round(decode, 3)}
    rec["host_over_device"] = round(rec["host_ms_per_step"]["median"] / rec["device_ms_per_step"]["median"], 2)
    rec["device_over_step"] = round(rec["device_ms_per_step"]["median"] / rec["step_alone_ms"]["median"], 3)
    rec["stream_over_step"] = round(rec["stream_ms_per_step"]["median"] / rec["step_alone_ms"]["median"], 2)
    return rec


def mixed(runs, B=16, n_each=24, sizes=((512, 512), (384, 448))):
    from hesic_amd import homography_train
    dev = torch.device("cuda")
    with tempfile.TemporaryDirectory() as tmp:
        for k, (h, w) in enumerate(sizes):
            a, b = _smooth_pairs(n_each, h, w, 2 + k)
            _write(tmp, "train", a, b, start=k * n_each)
        pairs = homography_train.list_pairs(tmp, "train")
        args = {"grouped": homography_train.parser().parse_args([tmp, "--batch_size", str(B), "--cache", "device"]),
                "mixed": homography_train.parser().parse_args([tmp, "--batch_size", str(B), "--cache", "device", "--mix-sizes"])}
        cache = homography_train.build_cache(tmp, "train", pairs, args["mixed"])
        tr = _trainer()
        t, steps = {k: [] for k in args}, {}
        for r in range(runs + 1):
            for k in args:
                _, steps[k], secs = homography_train.train_epoch(tr, pairs, args[k], random.Random(r), dev, cache)
                t[k].append(secs * 1e3)
    rec = {"shape": {"B": B, "sizes": [list(s) for s in sizes], "pairs_of_each": n_each, "patch_size": 128, "cache": "device"}}
    for k in args:
        rec[k] = {"steps_per_epoch": steps[k], "ms_per_epoch": _med(t[k][1:])}
    rec["mixed_over_grouped"] = round(rec["mixed"]["ms_per_epoch"]["median"] / rec["grouped"]["ms_per_epoch"]["median"], 3)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "homography_cache_bench.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("homography_cache_bench: needs a ROCm device")
    rec = {"device": torch.cuda.get_device_name(0), "runs": a.runs, "reps_per_run": a.reps, "kernel": kernel(a.runs, a.reps), "loop": loop(a.runs),
           "mixed": mixed(a.runs)}
    with open(a.out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print(json.dumps(rec))


if __name__ == "__main__":
    main()

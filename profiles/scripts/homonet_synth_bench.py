#!/usr/bin/env python3
"""What synthetic-warp pairs for HomographyNet cost, one process on one box, warm, median of ``--runs`` (7), variants alternating:

    kernel    B = 16 whole 512 x 512 uint8 HWC images -> 256 x 256 with 128 x 128 windows, as the HIP-event time of ``--reps`` replays of a
              captured graph that holds the entry alone:
              * synth:  ``hesic_homonet_synth_items`` on the left views (three launches; descriptors resident, deltas drawn with rho = 45);
              * items:  ``hesic_homonet_prepare_items`` on the same pairs (both views, one launch);
              * copy:   a plain device copy of as many bytes as the synth entry has to move (every input sample once, every output
                        once, grey_a a second time for the read-back).
              The synth entry's grey_a / patch_a / corners are compared bit for bit with the item entry's first.
    loop      the wall time per training step of ``python -m hesic_amd.homography_train``'s epoch loop under ``--cache device`` with
              ``--supervision synthetic`` against ``photometric``: B = 16, patch_size = 128, 512 x 512 pairs.

Writes profiles/homonet_synth_bench.json and prints it.  Run it under a time limit of its own:

    timeout -k 10 600 python profiles/scripts/homonet_synth_bench.py
"""
import argparse
import json
import os
import random
import sys
import tempfile

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from homography_cache_bench import _trainer, _write  # noqa: E402
from homography_prep_bench import _event_us, _graph_of, _med, _smooth_pairs  # noqa: E402


def kernel(runs, reps, B=16, H=512, W=512, S=256, P=128, rho=45):
    from hesic_amd import _lib as L
    from hesic_amd import functional as Fn
    from hesic_amd import geometry, homography
    from hesic_amd.compressai.datasets import MEAN, STD
    a, b = _smooth_pairs(B, H, W, 0)
    stored = [(torch.from_numpy(a[i]).cuda(), torch.from_numpy(b[i]).cuda()) for i in range(B)]
    windows = homography.window_origins(B, None, S, P, rho, random.Random(0))
    deltas = homography.draw_deltas(B, windows, P, rho, random.Random(1))
    items, synth = Fn.homonet_items(B), Fn.homonet_synth_items(B)
    for i, ((l, r), (wx, wy)) in enumerate(zip(stored, windows)):
        items[i] = (l.data_ptr(), r.data_ptr(), W, H, 0, 0, W, H, wx, wy)
        synth[i] = (l.data_ptr(), W, H, 0, 0, W, H, wx, wy, deltas[i])
    Fn.check_homonet_synth_items(synth, S, P)
    items_dev = torch.from_numpy(items.view("uint8").reshape(B, 48)).cuda()
    synth_dev = torch.from_numpy(synth.view("uint8").reshape(B, 72)).cuda()
    out_i = [torch.empty(s, device="cuda") for s in [(B, 1, S, S), (B, 1, S, S), (B, 1, P, P), (B, 1, P, P), (B, 4, 2)]]
    out_s = [torch.empty(s, dtype=torch.float64 if k == 4 else torch.float32, device="cuda")
             for k, s in enumerate([(B, 1, S, S), (B, 1, P, P), (B, 4, 2), (B, 4, 2), (B, 9), (B, 1, S, S), (B, 1, P, P)])]
    align = int(bool(geometry.DEFAULT_ALIGN_CORNERS))

    def launch_items():
        L.call("hesic_homonet_prepare_items", L.ptr(items_dev), B, S, P, float(MEAN), float(STD), *[L.ptr(t) for t in out_i], L.stream())

    def launch_synth():
        L.call("hesic_homonet_synth_items", L.ptr(synth_dev), B, S, P, float(MEAN), float(STD), align, *[L.ptr(t) for t in out_s], L.stream())

    launch_items()
    launch_synth()
    torch.cuda.synchronize()
    same = torch.equal(out_s[0], out_i[0]) and torch.equal(out_s[1], out_i[2]) and torch.equal(out_s[2], out_i[4])
    finite = all(bool(torch.isfinite(t).all()) for t in out_s)
    nbytes = stored[0][0].numel() * B + sum(t.numel() * t.element_size() for t in out_s) + out_s[0].numel() * 4 + synth_dev.numel()
    src = torch.empty(nbytes // 8, dtype=torch.float32, device="cuda").normal_()           # a copy moves 2 x its size
    dst = torch.empty_like(src)
    gi, gs = _graph_of(launch_items), _graph_of(launch_synth)
    variants = {"synth_graph_replay_us": lambda: _event_us(gs.replay, reps), "items_graph_replay_us": lambda: _event_us(gi.replay, reps),
                "copy_same_bytes_us": lambda: _event_us(lambda: dst.copy_(src), reps)}
    t = {k: [] for k in variants}
    for _ in range(runs + 1):                    # run 0 is the warm-up of every variant
        for k, fn in variants.items():
            t[k].append(fn())
    rec = {"shape": {"B": B, "H": H, "W": W, "pic_size": S, "patch_size": P, "rho": rho, "align_corners": align}, "synth_bytes": nbytes,
           "launches": 3, "first_view_equals_item_entry_bit_for_bit": bool(same), "outputs_finite": finite}
    rec.update({k: _med(v[1:]) for k, v in t.items()})
    rec["synth_times_the_copy"] = round(rec["synth_graph_replay_us"]["median"] / rec["copy_same_bytes_us"]["median"], 2)
    rec["synth_over_items"] = round(rec["synth_graph_replay_us"]["median"] / rec["items_graph_replay_us"]["median"], 3)
    return rec


def loop(runs, B=16, H=512, W=512, steps_per_run=4):
    from hesic_amd import homography_train
    dev = torch.device("cuda")
    with tempfile.TemporaryDirectory() as tmp:
        a, b = _smooth_pairs(B * steps_per_run, H, W, 1)
        _write(tmp, "train", a, b)
        pairs = homography_train.list_pairs(tmp, "train")
        args = homography_train.parser().parse_args([tmp, "--batch_size", str(B), "--cache", "device"])
        cache = homography_train.build_cache(tmp, "train", pairs, args)
        tr = _trainer()
        t = {"photometric": [], "synthetic": []}
        for r in range(runs + 1):
            for k in t:
                srng = random.Random(f"{r}/synth") if k == "synthetic" else None
                _, n, secs = homography_train.train_epoch(tr, pairs, args, random.Random(r), dev, cache, srng)
                t[k].append(secs / n * 1e3)
    rec = {"shape": {"B": B, "H": H, "W": W, "patch_size": 128, "steps_per_run": steps_per_run, "pairs": B * steps_per_run, "cache": "device"},
           "photometric_ms_per_step": _med(t["photometric"][1:]), "synthetic_ms_per_step": _med(t["synthetic"][1:])}
    rec["synthetic_over_photometric"] = round(rec["synthetic_ms_per_step"]["median"] / rec["photometric_ms_per_step"]["median"], 3)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "homonet_synth_bench.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("homonet_synth_bench: needs a ROCm device")
    rec = {"device": torch.cuda.get_device_name(0), "runs": a.runs, "reps_per_run": a.reps, "kernel": kernel(a.runs, a.reps), "loop": loop(a.runs)}
    with open(a.out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print(json.dumps(rec))


if __name__ == "__main__":
    main()

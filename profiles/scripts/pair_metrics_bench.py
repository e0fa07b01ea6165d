#!/usr/bin/env python3
"""What the per-pair rate-distortion metrics cost, one process on one box, warm, median of ``--runs`` (7), variants alternating:

    kernel    on the four likelihood maps and two image pairs of one HSIC forward (f16, B = 8 and B = 1, 512 x 512), HIP-event time of
              ``--reps`` replays of a captured graph:
              * pair_metrics: ``functional.pair_metrics`` (two launches, a (B, 8) table, no zero-fill);
              * rd_sums: ``functional.rd_sums`` (the existing batch-level kernel, unchanged: one launch, one fp64 atomic per block on six
                addresses), alone and with the zero-fill of its accumulators that a caller owes it (``models.rate_distortion``);
              * copy: a plain device copy of as many bytes as the reductions read;
    folder    ``python -m hesic_amd.eval_folder`` on a synthetic folder of 16 pairs of 512 x 512 with sidecars: pairs/s of the walk (PNG
              reading, upload, forward, metrics, MS-SSIM, one read-back) at --batch 8 and --batch 1, with and without --coded.

Writes profiles/pair_metrics_bench.json and prints it.  Run it under a time limit of its own:

    timeout -k 10 600 python profiles/scripts/pair_metrics_bench.py
"""
import argparse
import json
import os
import sys
import tempfile
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


def kernel(net, runs, reps, B, size=512):
    from hesic_amd import functional as Fn
    from hesic_amd import synthetic
    x1, x2, Hm = (t.cuda() for t in synthetic.stereo_batch(0, B, size, size))
    with torch.no_grad():
        out = net(x1, x2, Hm)
    torch.cuda.synchronize()
    keys = list(out["likelihoods"])
    liks = [out["likelihoods"][k] for k in keys]
    pairs = [(out["x1_hat"][..., :size, :size], x1), (out["x2_hat"][..., :size, :size], x2)]
    nbytes = sum(l.numel() * 4 for l in liks) + sum(t.numel() * t.element_size() for p in pairs for t in p)
    tab = torch.empty((B, len(keys) + 4), dtype=torch.float64, device="cuda")
    ws = torch.empty(1 << 20, dtype=torch.uint8, device="cuda")            # B = 8 needs 2592 fp64 partials; the call checks the size
    acc = torch.zeros(len(keys) + 2, dtype=torch.float64, device="cuda")
    lo, so = [acc[i:i + 1] for i in range(len(keys))], [acc[len(keys) + i:len(keys) + i + 1] for i in range(2)]

    def zero_and_rd():
        z = Fn._zeros(len(keys) + 2, torch.float64, x1.device)
        Fn.rd_sums(liks, [z[i:i + 1] for i in range(len(keys))], pairs, [z[len(keys) + i:len(keys) + i + 1] for i in range(2)])

    src = torch.empty(nbytes // 8, dtype=torch.float32, device="cuda").normal_()              # a copy moves 2 x its size
    dst = torch.empty_like(src)
    graphs = {"pair_metrics": _graph_of(lambda: Fn.pair_metrics(liks, pairs, out=tab, ws=ws)),
              "rd_sums": _graph_of(lambda: Fn.rd_sums(liks, lo, pairs, so)),
              "rd_sums_with_zero_fill": _graph_of(zero_and_rd)}
    variants = {k: (lambda g=g: _event_us(g.replay, reps)) for k, g in graphs.items()}
    variants["copy_same_bytes"] = lambda: _event_us(lambda: dst.copy_(src), reps)
    t = {k: [] for k in variants}
    for _ in range(runs + 1):                        # run 0 is the warm-up of every variant
        for k, fn in variants.items():
            t[k].append(fn())
    rec = {"shape": {"B": B, "H": size, "W": size, "likelihood_elements": [l.numel() for l in liks],
                     "x_hat": str(pairs[0][0].dtype).replace("torch.", ""), "x_hat_channels_last": bool(pairs[0][0].stride(1) == 1)},
           "bytes_read": nbytes}
    for k in variants:
        rec[k + "_us"] = _med(t[k][1:])
    rec["pair_metrics_over_rd_sums"] = round(rec["pair_metrics_us"]["median"] / rec["rd_sums_us"]["median"], 2)
    rec["pair_metrics_over_rd_sums_with_zero_fill"] = round(rec["pair_metrics_us"]["median"] / rec["rd_sums_with_zero_fill_us"]["median"], 2)
    rec["pair_metrics_times_the_copy"] = round(rec["pair_metrics_us"]["median"] / rec["copy_same_bytes_us"]["median"], 2)
    # the two kernels describe the same sums
    torch.cuda.synchronize()
    acc.zero_()
    Fn.rd_sums(liks, lo, pairs, so)
    Fn.pair_metrics(liks, pairs, out=tab, ws=ws)
    torch.cuda.synchronize()
    cols = tab.sum(0)[:len(keys) + 2]
    rec["max_relative_difference_of_the_batch_sums"] = float(((cols - acc).abs() / acc.abs()).max())
    return rec


def folder(runs, n=16, size=512):
    from PIL import Image
    from hesic_amd import codec, eval_folder, synthetic
    rec = {"shape": {"pairs": n, "H": size, "W": size}}
    with tempfile.TemporaryDirectory() as tmp:
        x1, x2, Hm = synthetic.stereo_batch(100, n, size, size)
        for side, x in (("left", x1), ("right", x2)):
            d = Path(tmp) / "test" / side
            d.mkdir(parents=True)
            for i, img in enumerate(codec.quantise(x)):
                Image.fromarray(img).save(d / f"{i:03d}.png")
        (Path(tmp) / "test" / "H").mkdir()
        for i in range(n):
            np.save(Path(tmp) / "test" / "H" / f"{i:03d}.npy", Hm[i].double().numpy())
        net = codec.load_model(None, torch.float16)
        variants = {"batch8": (8, False), "batch1": (1, False), "batch8_coded": (8, True), "batch1_coded": (1, True)}
        t = {k: [] for k in variants}
        psnr = {}
        for _ in range(runs + 1):                    # run 0 is the warm-up of every variant
            for k, (batch, coded) in variants.items():
                _, summary = eval_folder.evaluate_folder(net, tmp, "test", batch, coded=coded, log=lambda s: None)
                t[k].append(summary["pairs_per_s"])
                psnr[k] = (summary["psnr"], summary["psnr_of_mean_mse"], summary["bpp"], summary.get("coded_bpp"))
    for k in variants:
        rec[k + "_pairs_per_s"] = _med(t[k][1:])
    rec["psnr_mean_over_pairs"], rec["psnr_of_mean_mse"], rec["bpp"], rec["coded_bpp"] = psnr["batch8_coded"]
    rec["batch1_equals_batch8"] = {"psnr": psnr["batch1"][0] == psnr["batch8"][0], "bpp": psnr["batch1"][2] == psnr["batch8"][2]}
    rec["batch8_over_batch1"] = round(rec["batch8_pairs_per_s"]["median"] / rec["batch1_pairs_per_s"]["median"], 2)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pair_metrics_bench.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("pair_metrics_bench: needs a ROCm device")
    from hesic_amd import codec
    net = codec.load_model(None, torch.float16)
    rec = {"device": torch.cuda.get_device_name(0), "runs": a.runs, "reps_per_run": a.reps,
           "kernel_B8": kernel(net, a.runs, a.reps, 8), "kernel_B1": kernel(net, a.runs, a.reps, 1), "folder": folder(a.runs)}
    with open(a.out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print(json.dumps(rec))


if __name__ == "__main__":
    main()

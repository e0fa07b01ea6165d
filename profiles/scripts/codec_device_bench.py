#!/usr/bin/env python3
"""HESIC bit-stream, wall time per stereo pair (512 x 512, float16 maps), one process on one box:

    host    HSIC.compress + HSIC.decompress (per-element tables to the host, one-threaded host range coder), B = 1
    device  HSIC.compress_batch + HSIC.decompress_batch (device range coder, csrc/codec.hip), B = 1 and B = 8

Warm runs (the first one of each configuration packs weights and loads kernels and is dropped), median of ``--runs`` (>= 6), min and max
beside it.  Writes profiles/codec_device_bench.json and prints it.  Run it under a time limit of its own:

    timeout -k 10 900 python profiles/scripts/codec_device_bench.py

``--trace`` instead runs the B = 8 device path three times and nothing else: the workload of
``rocprofv3 --kernel-trace --stats -- python profiles/scripts/codec_device_bench.py --trace`` (profiles/codec_device_kernel_stats.csv).
"""
import argparse
import json
import os
import sys
import tempfile
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)


def _stats(times, pairs):
    warm = sorted(times)
    per = [t / pairs * 1e3 for t in warm]
    return {"ms_per_pair": round(per[len(per) // 2], 3), "min": round(per[0], 3), "max": round(per[-1], 3), "runs": len(per)}


def _timed(fn, runs):
    out, times = None, []
    for rep in range(runs + 1):                      # run 0 is the cold one
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        if rep:
            times.append(time.perf_counter() - t0)
    return out, times


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--channels-per-stream", type=int, default=1)
    ap.add_argument("--trace", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "codec_device_bench.json"))
    a = ap.parse_args()
    if a.runs < 6:
        ap.error("--runs must be at least 6")
    import hesic_amd
    from hesic_amd import bitstream, models, synthetic
    hesic_amd.set_compute_dtype(torch.float16)
    net = models.HSIC()
    synthetic.fill_state_dict_(net.state_dict())
    net = net.cuda().eval()
    net.update(force=True)
    cps = a.channels_per_stream
    x1, x2, Hm = (t.cuda() for t in synthetic.stereo_batch(0, 8, a.size, a.size))
    if a.trace:
        for _ in range(3):
            enc = net.compress_batch(x1, x2, Hm, channels_per_stream=cps)
            dec = net.decompress_batch(enc["blobs"], Hm)
        torch.cuda.synchronize()
        assert torch.equal(dec["y2_hat"].float(), enc["y2_hat"].float())
        return
    rec = {"size": a.size, "dtype": "float16", "channels_per_stream": cps, "device": torch.cuda.get_device_name(0)}
    with tempfile.TemporaryDirectory() as td:
        enc, te = _timed(lambda: net.compress(x1[:1], x2[:1], Hm[:1], "p", td), a.runs)
        dec, td_ = _timed(lambda: net.decompress(None, None, Hm[:1], "p", td), a.runs)
        assert torch.equal(dec["y2_hat"].float().cpu(), enc["y2_hat"].float().cpu())
        rec["host_b1"] = {"compress": _stats(te, 1), "decompress": _stats(td_, 1), "total": _stats([p + q for p, q in zip(te, td_)], 1),
                          "bpp_real": round(enc["bpp_real"], 4)}
    for B in (1, 8):
        enc, te = _timed(lambda: net.compress_batch(x1[:B], x2[:B], Hm[:B], channels_per_stream=cps), a.runs)
        dec, td_ = _timed(lambda: net.decompress_batch(enc["blobs"], Hm[:B]), a.runs)
        assert torch.equal(dec["y2_hat"].float(), enc["y2_hat"].float()) and torch.equal(dec["y1_hat"].float(), enc["y1_hat"].float())
        rec[f"device_b{B}"] = {"compress": _stats(te, B), "decompress": _stats(td_, B), "total": _stats([p + q for p, q in zip(te, td_)], B),
                               "bpp_real": round(sum(enc["bpp_real"]) / B, 4)}
        if B == 8:          # what the row evaluation costs depends on the alphabets: minmax of (view 1, view 2) and coded channels, per pair
            heads = [bitstream.parse_pair(bl)["views"] for bl in enc["blobs"]]
            rec["minmax"] = [[v["minmax"] for v in h] for h in heads]
            rec["coded_channels"] = [[sum(v["flags"]) for v in h] for h in heads]
    rec["speedup_device_b8_over_host_b1"] = round(rec["host_b1"]["total"]["ms_per_pair"] / rec["device_b8"]["total"]["ms_per_pair"], 2)
    with open(a.out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print(json.dumps(rec))


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""HESIC+ bit-stream, wall time per stereo pair (512 x 512, float16 maps, synthetic weights), one process on one box, the two paths
alternating round by round:

    pair    HSICJoint.compress + decompress (per-pair: tables to a one-threaded host coder, 125 wavefront groups per view each with a
            host range-decode in the loop), B = 1 -- code the batched path does not touch
    batch   HSICJoint.compress_batch + decompress_batch (device range coder, one walk of the groups for the B images) at
            B = 1, 4, 8 and channels_per_stream = 1, 8

Round 0 of every configuration is cold (packs weights, captures graphs) and is dropped; then ``--runs`` (>= 7) rounds, each timing every
configuration once, wall time ending in a device synchronise.  Median, min and max per configuration.  Writes
profiles/codec_joint_device_bench.json and prints it.  Run it under a time limit of its own:

    timeout -k 10 900 python profiles/scripts/codec_joint_device_bench.py

``--trace`` instead runs the B = 8, cps = 1 batch path three times and nothing else: the workload of
``rocprofv3 --kernel-trace --stats -- python profiles/scripts/codec_joint_device_bench.py --trace``
(profiles/codec_joint_device_kernel_stats.csv).
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
    per = sorted(t / pairs * 1e3 for t in times)
    return {"ms_per_pair": round(per[len(per) // 2], 3), "min": round(per[0], 3), "max": round(per[-1], 3), "runs": len(per)}


def _wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return out, time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--trace", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "codec_joint_device_bench.json"))
    a = ap.parse_args()
    if a.runs < 7:
        ap.error("--runs must be at least 7")
    import hesic_amd
    from hesic_amd import bitstream, models, synthetic
    hesic_amd.set_compute_dtype(torch.float16)
    net = models.HSICJoint()
    synthetic.fill_state_dict_(net.state_dict())
    net = net.cuda().eval()
    net.update(force=True)
    x1, x2, Hm = (t.cuda() for t in synthetic.stereo_batch(0, 8, a.size, a.size))
    if a.trace:
        for _ in range(3):
            enc = net.compress_batch(x1, x2, Hm, channels_per_stream=1)
            dec = net.decompress_batch(enc["blobs"], Hm)
        torch.cuda.synchronize()
        assert torch.equal(dec["y2_hat"].float(), enc["y2_hat"].float())
        return
    configs = [(B, cps) for B in (1, 4, 8) for cps in (1, 8)]
    times = {"pair": ([], [])}
    times.update({c: ([], []) for c in configs})
    bpp, heads = {}, None
    with tempfile.TemporaryDirectory() as td:
        for rnd in range(a.runs + 1):
            enc, te = _wall(lambda: net.compress(x1[:1], x2[:1], Hm[:1], "p", td))
            dec, td_ = _wall(lambda: net.decompress(None, None, Hm[:1], "p", td))
            assert torch.equal(dec["y2_hat"].float().cpu(), enc["y2_hat"].float().cpu())
            bpp["pair"] = enc["bpp_real"]
            ref = dec
            if rnd:
                times["pair"][0].append(te)
                times["pair"][1].append(td_)
            for B, cps in configs:
                enc, te = _wall(lambda: net.compress_batch(x1[:B], x2[:B], Hm[:B], channels_per_stream=cps))
                dec, td_ = _wall(lambda: net.decompress_batch(enc["blobs"], Hm[:B]))
                assert torch.equal(dec["y2_hat"].float(), enc["y2_hat"].float()) and torch.equal(dec["y1_hat"].float(), enc["y1_hat"].float())
                assert torch.equal(dec["x2_hat"][:1].float(), ref["x2_hat"].float())          # pair 0 is the per-pair path's pair
                bpp[B, cps] = sum(enc["bpp_real"]) / B
                if (B, cps) == (8, 1):
                    heads = [bitstream.parse_pair(bl)["views"] for bl in enc["blobs"]]
                if rnd:
                    times[B, cps][0].append(te)
                    times[B, cps][1].append(td_)

    def entry(key, pairs):
        te, td_ = times[key]
        return {"compress": _stats(te, pairs), "decompress": _stats(td_, pairs), "total": _stats([p + q for p, q in zip(te, td_)], pairs),
                "bpp_real": round(bpp[key], 4)}

    rec = {"size": a.size, "dtype": "float16", "device": torch.cuda.get_device_name(0), "pair_b1": entry("pair", 1)}
    for B, cps in configs:
        rec[f"batch_b{B}_cps{cps}"] = entry((B, cps), B)
    rec["minmax"] = [[v["minmax"] for v in h] for h in heads]
    rec["coded_channels"] = [[sum(v["flags"]) for v in h] for h in heads]
    pd, bd = rec["pair_b1"]["decompress"], rec["batch_b8_cps1"]["decompress"]
    rec["decompress_pair_spread_ms"] = round(pd["max"] - pd["min"], 3)
    rec["decompress_gain_b8_cps1_ms_per_pair"] = round(pd["ms_per_pair"] - bd["ms_per_pair"], 3)
    rec["decompress_ratio_pair_over_b8_cps1"] = round(pd["ms_per_pair"] / bd["ms_per_pair"], 2)
    rec["acceptance_gain_exceeds_spread"] = rec["decompress_gain_b8_cps1_ms_per_pair"] > rec["decompress_pair_spread_ms"]
    with open(a.out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print(json.dumps(rec))


if __name__ == "__main__":
    main()

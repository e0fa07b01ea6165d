"""Throughput of the stereo homography estimator (hesic_amd.stereo_h): pairs/s at B = 1 and B = 8 for 512 x 512 and B = 4 for
860 x 1080 synthetic pairs (uint8 on the device), and the time of each entry point from HIP events recorded around its launches.
``--modes`` times the four descriptor modes (upright / oriented x 64 / 128-d) at each size instead of the default upright 64-d.

    python profiles/scripts/stereo_h_bench.py [--iters 20] [--modes] [--out FILE.json]
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from hesic_amd import _lib as L, stereo_h, synthetic  # noqa: E402


MODES = (("upright64", True, False), ("oriented64", False, False), ("upright128", True, True), ("oriented128", False, True))


def run(B, H, W, iters, upright=True, extended=False):
    x1, x2, _ = synthetic.stereo_batch(0, B, H, W)
    a = (x1 * 255).round().to(torch.uint8).cuda()
    b = (x2 * 255).round().to(torch.uint8).cuda()
    ws = stereo_h._Workspace()
    for _ in range(3):
        stereo_h.estimate_homography(a, b, upright=upright, extended=extended, _ws=ws)
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(iters):
        out = stereo_h.estimate_homography(a, b, upright=upright, extended=extended, _ws=ws)
    t1.record()
    torch.cuda.synchronize()
    ms = t0.elapsed_time(t1) / iters
    marks = []

    def hook(name, args):
        e = torch.cuda.Event(enable_timing=True)
        e.record()
        marks.append((name, e))
    stage = {}
    for _ in range(iters):
        marks.clear()
        with L.call_hook(hook):
            stereo_h.estimate_homography(a, b, upright=upright, extended=extended, _ws=ws)
        end = torch.cuda.Event(enable_timing=True)
        end.record()
        torch.cuda.synchronize()
        seq = marks + [("end", end)]
        for (n, e), (_, f) in zip(seq, seq[1:]):
            stage[n] = stage.get(n, 0.0) + e.elapsed_time(f) / iters
    return {"B": B, "H": H, "W": W, "upright": upright, "extended": extended, "ms_per_call": round(ms, 4), "ms_per_pair": round(ms / B, 4),
            "pairs_per_s": round(1000.0 * B / ms, 1), "valid": int(out[1].sum()), "inliers": out[2].tolist(),
            "stage_ms": {k.replace("hesic_stereo_h_", ""): round(v, 4) for k, v in stage.items()}}


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--iters", type=int, default=20)
    p.add_argument("--modes", action="store_true")
    p.add_argument("--out")
    a = p.parse_args()
    modes = MODES if a.modes else MODES[:1]
    res = [dict(run(B, H, W, a.iters, up, ext), mode=name) if a.modes else run(B, H, W, a.iters)
           for B, H, W in ((1, 512, 512), (8, 512, 512), (4, 860, 1080)) for name, up, ext in modes]
    for r in res:
        print(json.dumps(r))
    if a.out:
        with open(a.out, "w") as f:
            json.dump({"device": torch.cuda.get_device_name(0), "results": res}, f, indent=1)


if __name__ == "__main__":
    main()

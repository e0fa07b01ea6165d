#!/usr/bin/env python3
"""What photometric homography refinement costs, one process on one box, warm, median of ``--runs`` (7), variants alternating:

    call      B = 8 pairs of 3 x 512 x 512 (the right view is the left one shifted by (6, 3) px), the identity as the start, levels 3, iters 10:
              * refine:     ``homography.refine_h_matrix`` as the HIP-event time of ``--reps`` replays of a captured graph of the whole call;
              * normal_eq:  level 0's normal-equation launch alone (``hesic_hrefine_normal_eq``), the same way;
              * copy:       a plain device copy of the bytes that launch reads (level 0 of both views);
              * compress:   ``HSIC.compress_batch`` (float16, synthetic weights) on the same batch as host wall time with a synchronisation:
                            what the option adds to an encode.
              The corner error against the known shift before and after is recorded with the call.
    eval      ``python -m hesic_amd.homography_eval --checkpoint synthetic`` with and without ``--refine`` on a folder of 16 such pairs: the two
              summaries, whatever they show (the synthetic weights are an untrained net).

Writes profiles/homography_refine_bench.json and prints it.  Run it under a time limit of its own:

    timeout -k 10 600 python profiles/scripts/homography_refine_bench.py
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
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from homography_cache_bench import _write  # noqa: E402
from homography_prep_bench import _event_us, _graph_of, _med, _smooth_pairs  # noqa: E402


def _corner_error(Hm, Ht, h, w):
    c = torch.tensor([[0, 0, 1], [w - 1, 0, 1], [w - 1, h - 1, 1], [0, h - 1, 1]], dtype=torch.float64, device=Hm.device)
    p, q = c @ Hm.double().transpose(1, 2), c @ Ht.double().transpose(1, 2)
    return (p[..., :2] / p[..., 2:] - q[..., :2] / q[..., 2:]).square().sum(-1).sqrt().mean(-1)


def call(runs, reps, B=8, H=512, W=512, levels=3, iters=10):
    from hesic_amd import _lib as L
    from hesic_amd import codec, functional as Fn, homography
    a, b = _smooth_pairs(B, H, W, 0)
    x1, x2 = (torch.from_numpy(v).cuda().permute(0, 3, 1, 2).float().div(255.0).contiguous() for v in (a, b))
    eye = torch.eye(3, device="cuda").repeat(B, 1, 1)
    truth = eye.clone()
    truth[:, 0, 2], truth[:, 1, 2] = -6.0, -3.0                  # the right view shows the left one's pixel (x + 6, y + 3) at (x, y)
    out = {}

    def refine():
        out["h"], out["info"] = homography.refine_h_matrix(x1, x2, eye, levels=levels, iters=iters)

    refine()
    torch.cuda.synchronize()
    info = {k: v.cpu().tolist() for k, v in out["info"].items()}
    err0, err1 = _corner_error(eye, truth, H, W).cpu().tolist(), _corner_error(out["h"], truth, H, W).cpu().tolist()
    pyr, _ = Fn.homography_refine_pyramid(x1, x2, levels)
    A = torch.eye(3, dtype=torch.float64, device="cuda").repeat(B, 1, 1)
    partials = torch.empty((B, L.lib().hesic_hrefine_blocks(H, W), L.HREFINE_SUMS), dtype=torch.float64, device="cuda")

    def normal_eq():
        L.call("hesic_hrefine_normal_eq", L.ptr(pyr), B, H, W, levels, 0, L.ptr(A), 9, 0.0, L.ptr(partials), L.stream())

    read_bytes = 2 * B * H * W * 4
    src = torch.empty(read_bytes // 4, dtype=torch.float32, device="cuda").normal_()
    dst = torch.empty_like(src)
    net = codec.load_model(None, torch.float16)

    def compress_ms():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        net.compress_batch(x1, x2, eye)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    gr, gn = _graph_of(refine), _graph_of(normal_eq)
    variants = {"refine_graph_replay_us": lambda: _event_us(gr.replay, reps), "normal_eq_level0_graph_replay_us": lambda: _event_us(gn.replay, reps * 10),
                "copy_of_the_bytes_read_us": lambda: _event_us(lambda: dst.copy_(src), reps * 10), "compress_batch_ms": compress_ms}
    t = {k: [] for k in variants}
    for _ in range(runs + 1):                    # run 0 is the warm-up of every variant
        for k, fn in variants.items():
            t[k].append(fn())
    n_levels = Fn.homography_refine_levels(H, W, levels)
    rec = {"shape": {"B": B, "C": 3, "H": H, "W": W, "levels": levels, "iters": iters, "huber": None},
           "launches": 4 + n_levels * (1 + 2 * (iters + 1)) + (2 if n_levels > 1 else 0), "normal_eq_level0_bytes_read": read_bytes,
           "corner_error_px_before": [round(v, 4) for v in err0], "corner_error_px_after": [round(v, 5) for v in err1],
           "cost_before": info["cost_before"], "cost_after": info["cost_after"], "accepted": info["accepted"], "rejected": info["rejected"]}
    rec.update({k: _med(v[1:]) for k, v in t.items()})
    rec["normal_eq_times_the_copy"] = round(rec["normal_eq_level0_graph_replay_us"]["median"] / rec["copy_of_the_bytes_read_us"]["median"], 2)
    rec["refine_over_compress_batch"] = round(rec["refine_graph_replay_us"]["median"] / 1e3 / rec["compress_batch_ms"]["median"], 4)
    return rec


def evaluation(pairs=16, H=512, W=512):
    from hesic_amd import homography_eval
    with tempfile.TemporaryDirectory() as tmp:
        a, b = _smooth_pairs(pairs, H, W, 1)
        _write(tmp, "test", a, b)
        args = [tmp, "--checkpoint", "synthetic", "--batch", "8"]
        plain = homography_eval.main(args, log=lambda _: None)[-1]
        refined = homography_eval.main(args + ["--refine"], log=lambda _: None)[-1]
    return {"shape": {"pairs": pairs, "H": H, "W": W, "checkpoint": "synthetic", "rho": 45, "picsize": 256, "patchsize": 128},
            "without_refine": plain, "with_refine": refined}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "homography_refine_bench.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("homography_refine_bench: needs a ROCm device")
    rec = {"device": torch.cuda.get_device_name(0), "runs": a.runs, "reps_per_run": a.reps, "call": call(a.runs, a.reps), "eval": evaluation()}
    with open(a.out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print(json.dumps(rec))


if __name__ == "__main__":
    main()

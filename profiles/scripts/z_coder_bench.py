#!/usr/bin/env python3
"""The z strings of the batched bit-stream on the host rANS coder (``z_coder="host"``: the path the models had before csrc/rans.hip, the
yardstick) against the device rANS coder (``z_coder="device"``), 512 x 512, float16 maps, one process on one box, warm, the two settings
ALTERNATING run by run, median of ``--runs`` (7) with min and max:

    models    wall time per pair of compress_batch and decompress_batch, HSIC and HSICJoint, B = 1 and B = 8
    launches  the encode (+ compaction) and decode launches alone as HIP-graph replays for the 2 B z streams of such a batch (8192 symbols
              each, the symbols of the model's own z), next to the host coder's time for the same streams and to a device copy of the
              bytes those launches move
    folder    ``eval_folder --coded`` in pairs / s on a generated folder of 512 x 512 pairs

``--only-launches`` runs the second section alone (profiles/z_coder_plain_div.json is that run with libhesic_hip_f16.so built with
-DHESIC_RANS_PLAIN_DIV=1: the compiler's 64-bit division in the encoder's fold instead of the double reciprocal).

Writes profiles/z_coder_bench.json and prints it.  Run it under a time limit of its own:

    timeout -k 10 900 python profiles/scripts/z_coder_bench.py
"""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
SETTINGS = ("host", "device")


def _stats(values, digits=3):
    v = sorted(values)
    return {"median": round(v[len(v) // 2], digits), "min": round(v[0], digits), "max": round(v[-1], digits), "runs": len(v)}


def _wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return out, (time.perf_counter() - t0) * 1e3


def _alternating(fns, runs):
    """fns: {setting: callable}; one dropped warm-up each, then ``runs`` rounds host, device, host, ... -> {setting: [ms]}"""
    times = {k: [] for k in fns}
    for rep in range(runs + 1):
        for k, fn in fns.items():
            _, ms = _wall(fn)
            if rep:
                times[k].append(ms)
    return times


def _replay_us(graph, runs, inner=20):
    out = []
    for _ in range(runs + 1):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(inner):
            graph.replay()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b) * 1e3 / inner)
    return out[1:]


def _capture(fn):
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        fn()
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        keep = fn()
    return g, keep


def bench_models(rec, runs, size, timed=True):
    from hesic_amd import models, synthetic
    nets = {}
    for cls in ("HSIC", "HSICJoint") if timed else ("HSIC",):
        net = getattr(models, cls)()
        synthetic.fill_state_dict_(net.state_dict())
        nets[cls] = net.cuda().eval()
        nets[cls].update(force=True)
    x1, x2, Hm = (t.cuda() for t in synthetic.stereo_batch(0, 8, size, size))
    for cls, net in nets.items() if timed else ():
        for B in (1, 8):
            a1, a2, ah = x1[:B], x2[:B], Hm[:B]
            enc = {z: net.compress_batch(a1, a2, ah, z_coder=z) for z in SETTINGS}
            assert enc["host"]["blobs"] == enc["device"]["blobs"]
            blobs = enc["host"]["blobs"]
            tc = _alternating({z: (lambda z=z: net.compress_batch(a1, a2, ah, z_coder=z)) for z in SETTINGS}, runs)
            td = _alternating({z: (lambda z=z: net.decompress_batch(blobs, ah, z_coder=z)) for z in SETTINGS}, runs)
            rec[f"{cls}_b{B}"] = {z: {"compress_ms_per_pair": _stats([t / B for t in tc[z]]), "decompress_ms_per_pair": _stats([t / B for t in td[z]])}
                                  for z in SETTINGS}
    return nets["HSIC"], (x1, x2, Hm)


def bench_launches(rec, net, batch, runs):
    from hesic_amd import _host, bitstream
    from hesic_amd import functional as Fn
    x1, x2, Hm = batch
    eb = net.entropy_bottleneck1
    table, lengths, offsets, medians = eb._device_tables(x1.device)
    tn, ln, on = (t.cpu().numpy() for t in (table, lengths, offsets))
    blobs = net.compress_batch(x1, x2, Hm, z_coder="host")["blobs"]
    zs = (x1.shape[-2] // 64, x1.shape[-1] // 64)
    strings = [bitstream.parse_pair(bl)["views"][0]["z"] for bl in blobs]
    z_hat = torch.cat([eb.decompress([s_], zs) for s_ in strings])
    sym8 = torch.round(z_hat - eb._medians().detach().view(1, -1, 1, 1)).int().contiguous(memory_format=torch.channels_last)
    C, P = sym8.shape[1], zs[0] * zs[1]
    idx = np.repeat(np.arange(C, dtype=np.int32), P)
    for B in (1, 8):
        sym = torch.cat([sym8[:B], sym8[:B]]).contiguous(memory_format=torch.channels_last)            # the 2 B streams of a batch's two views
        n_streams, n = sym.shape[0], C * P
        flat = sym.cpu().numpy().reshape(n_streams, -1)
        host_enc, host_dec, hs = [], [], None
        for _ in range(runs + 1):
            t0 = time.perf_counter()
            hs = [_host.rans_encode_arrays(s_, idx, tn, ln, on) for s_ in flat]
            t1 = time.perf_counter()
            back = [_host.rans_decode_arrays(s_, idx, tn, ln, on) for s_ in hs]
            t2 = time.perf_counter()
            host_enc.append((t1 - t0) * 1e6)
            host_dec.append((t2 - t1) * 1e6)
        assert all(np.array_equal(b_, s_) for b_, s_ in zip(back, flat))
        g_enc, (data, counts, status, zq) = _capture(lambda: Fn.rans_encode_launch(sym, table, lengths, offsets, None, (medians, torch.float16)))
        g_enc.replay()
        torch.cuda.synchronize()
        total = int(counts.sum())
        assert int(status.abs().sum()) == 0 and data[:total].cpu().numpy().tobytes() == b"".join(hs)
        payload, cnt = data[:total].clone(), counts.clone()
        g_dec, (zd, st) = _capture(lambda: Fn.rans_decode(payload, cnt, (C,) + zs, table, lengths, offsets, None, (medians, torch.float16), check=False))
        g_dec.replay()
        torch.cuda.synchronize()
        assert int(st.abs().sum()) == 0 and torch.equal(zd, zq)
        src = torch.empty(sym.numel() * 4 + total + zq.numel() * 2, dtype=torch.uint8, device="cuda")
        dst = torch.empty_like(src)
        g_cp, _ = _capture(lambda: dst.copy_(src))
        rec[f"launches_{n_streams}_streams"] = {
            "symbols_per_stream": n, "payload_bytes": total,
            "device_encode_us": _stats(_replay_us(g_enc, runs), 1), "device_decode_us": _stats(_replay_us(g_dec, runs), 1),
            "host_encode_us": _stats(host_enc[1:], 1), "host_decode_us": _stats(host_dec[1:], 1),
            "device_copy_of_the_bytes_us": _stats(_replay_us(g_cp, runs), 1), "bytes_copied": src.numel()}


def bench_folder(rec, net, runs, size, pairs=16):
    from PIL import Image
    from hesic_amd import eval_folder, synthetic
    with tempfile.TemporaryDirectory() as td:
        for sub in ("left", "right", "H"):
            os.makedirs(os.path.join(td, "test", sub))
        for i in range(pairs):
            x1, x2, Hm = synthetic.stereo_batch(100 + i, 1, size, size)
            for side, x in (("left", x1), ("right", x2)):
                Image.fromarray((x[0].clamp(0, 1) * 255).round().to(torch.uint8).permute(1, 2, 0).numpy()).save(
                    os.path.join(td, "test", side, f"p{i:03d}.png"))
            np.save(os.path.join(td, "test", "H", f"p{i:03d}.npy"), Hm[0].double().numpy())
        quiet = lambda _line: None
        fns = {z: (lambda z=z: eval_folder.evaluate_folder(net, td, "test", 8, coded=True, log=quiet, z_coder=z)) for z in SETTINGS}
        times = _alternating(fns, max(3, runs // 2))
    rec["eval_folder_coded"] = {z: {"pairs_per_s": _stats([pairs / (t / 1e3) for t in times[z]], 2)} for z in SETTINGS}
    rec["eval_folder_coded"]["pairs"] = pairs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "z_coder_bench.json"))
    ap.add_argument("--only-launches", action="store_true",
                    help="the launches section alone (an A/B build of the library, e.g. -DHESIC_RANS_PLAIN_DIV=1 of csrc/rans.hip, against the normal one)")
    a = ap.parse_args()
    import hesic_amd
    hesic_amd.set_compute_dtype(torch.float16)
    rec = {"size": a.size, "dtype": "float16", "device": torch.cuda.get_device_name(0), "runs": a.runs,
           "protocol": "one process, warm, host and device settings alternating run by run, median (min, max); yardstick: z_coder='host'"}
    net, batch = bench_models(rec, a.runs, a.size, timed=not a.only_launches)
    bench_launches(rec, net, batch, a.runs)
    if not a.only_launches:
        bench_folder(rec, net, a.runs, a.size)
    with open(a.out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print(json.dumps(rec))


if __name__ == "__main__":
    main()

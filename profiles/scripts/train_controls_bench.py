#!/usr/bin/env python3
"""What the step controls cost: the ``GraphedTrainer`` step at B = 8, 512 x 512, bfloat16, HSIC with
``clip_max_norm=1.0, skip_nonfinite=True`` against the step of a BASELINE tree (the parent commit, built, given with ``--baseline``), one box,
both warm, alternating, median of ``--runs`` (7).

Two trees carry the same package name, so each runs in a worker process of its own (two processes hold the GPU); the driver hands them the
turn over a pipe: a turn is ``--steps`` replays inside a host clock that ends in a synchronise.  The worker of this tree also times a plain
device copy of the main group's flat gradient buffer (HIP events, same turn): the yardstick for "one extra read of that buffer".

    timeout -k 10 900 python profiles/scripts/train_controls_bench.py --baseline /path/to/parent/tree

writes profiles/train_controls_bench.json (without ``--baseline``: this tree with and without the controls).  ``--trace`` replays the step with
controls ten times and nothing else: the workload of

    rocprofv3 --kernel-trace --stats -d DIR -o t --output-format csv -- python profiles/scripts/train_controls_bench.py --trace

and ``--kernel-stats DIR/t_kernel_stats.csv [--kernel-trace DIR/t_kernel_trace.csv]`` merges that run's rows for the new kernels into the JSON.
"""
import argparse
import csv
import json
import os
import subprocess
import sys
import time

HERE = os.path.abspath(__file__)
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(HERE)))
KERNELS = ("grad_sumsq_partials_kernel", "grad_norm_decide_kernel", "adam_bump_steps_ctl_kernel", "adam_update_ctl_kernel", "adam_update_kernel")


def _med(v):
    s = sorted(v)
    return {"median": round(s[len(s) // 2], 4), "min": round(s[0], 4), "max": round(s[-1], 4), "runs": len(s)}


def _trainer(controls, B=8, size=512):
    import torch
    import hesic_amd
    from hesic_amd import models, synthetic
    from hesic_amd.train import GraphedTrainer
    hesic_amd.set_compute_dtype(torch.bfloat16)
    net = models.HSIC()
    synthetic.fill_state_dict_(net.state_dict())
    kw = dict(clip_max_norm=1.0, skip_nonfinite=True) if controls else {}
    tr = GraphedTrainer(net.cuda(), lr=1e-4, aux_lr=1e-3, lmbda=0.0067, **kw)
    batch = tuple(t.cuda() for t in synthetic.stereo_batch(0, B, size, size))
    for _ in range(tr.warmup + 4):                 # eager warm-up steps, the capture, three replays
        out = tr.step(*batch)
    torch.cuda.synchronize()
    assert tr.graph is not None
    return tr, batch, out


def worker(root, controls):
    """Serve turns: "run N" -> ms per step of N replays; "copy N" -> us per plain copy of the main flat gradient; "last" -> the loss dict."""
    sys.path.insert(0, root)
    import torch
    tr, batch, out = _trainer(controls)
    g = tr.main_group.flat_g
    dst = torch.empty_like(g)
    print(json.dumps({"ready": True, "main_numel": g.numel(), "aux_numel": tr.aux_group.numel, "package": os.path.dirname(sys.modules["hesic_amd"].__file__)}), flush=True)
    for line in sys.stdin:
        cmd, *arg = line.split()
        if cmd == "run":
            n = int(arg[0])
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(n):
                out = tr.step(*batch)
            torch.cuda.synchronize()
            print(json.dumps({"ms": (time.perf_counter() - t0) / n * 1e3}), flush=True)
        elif cmd == "copy":
            n = int(arg[0])
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(n):
                dst.copy_(g)
            e1.record()
            torch.cuda.synchronize()
            print(json.dumps({"us": e0.elapsed_time(e1) / n * 1e3}), flush=True)
        elif cmd == "last":
            print(json.dumps({k: float(v) for k, v in out.items()}), flush=True)
        else:
            break


class _Worker:
    def __init__(self, root, controls):
        self.p = subprocess.Popen([sys.executable, HERE, "--worker", "--root", root, "--controls", str(int(controls))], stdin=subprocess.PIPE,
                                  stdout=subprocess.PIPE, text=True, cwd=root)
        self.info = self._read()

    def _read(self):
        while True:
            line = self.p.stdout.readline()
            if not line:
                raise SystemExit(f"train_controls_bench: a worker ended early (exit {self.p.wait()})")
            if line.startswith("{"):
                return json.loads(line)

    def ask(self, cmd):
        self.p.stdin.write(cmd + "\n")
        self.p.stdin.flush()
        return self._read()

    def close(self):
        try:
            self.p.stdin.write("quit\n")
            self.p.stdin.flush()
        except OSError:
            pass
        self.p.wait(timeout=60)


def kernel_stats(path):
    """Rows of a rocprofv3 ``*_kernel_stats.csv`` for the kernels of the control path (and the plain Adam update for comparison)."""
    rows = {}
    with open(path) as f:
        for r in csv.DictReader(f):
            name = r.get("Name", "")
            for k in KERNELS:
                if k in name:
                    rows.setdefault(k, []).append({"name": name, "calls": int(r["Calls"]), "total_ns": int(float(r["TotalDurationNs"])),
                                                   "average_ns": round(float(r["AverageNs"]), 1), "min_ns": int(float(r["MinNs"])),
                                                   "max_ns": int(float(r["MaxNs"]))})
    return rows


def kernel_trace(path):
    """The same kernels from the run's ``*_kernel_trace.csv``, split by grid size (the main group's launches and the aux group's differ by
    three orders of magnitude, an average over both says nothing): median / min / max duration in ns."""
    d = {}
    with open(path) as f:
        for r in csv.DictReader(f):
            for k in KERNELS:
                if k in r["Kernel_Name"]:
                    d.setdefault((k, int(r["Grid_Size_X"])), []).append(int(r["End_Timestamp"]) - int(r["Start_Timestamp"]))
    return [{"kernel": k, "grid_threads": g, "launches": len(v), "median_ns": sorted(v)[len(v) // 2], "min_ns": min(v), "max_ns": max(v)}
            for (k, g), v in sorted(d.items())]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--baseline", default=None, help="root of a built tree of the parent commit (default: this tree without the controls)")
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--copies", type=int, default=50)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "train_controls_bench.json"))
    ap.add_argument("--trace", action="store_true")
    ap.add_argument("--kernel-stats", default=None)
    ap.add_argument("--kernel-trace", default=None)
    ap.add_argument("--worker", action="store_true")
    ap.add_argument("--root", default=ROOT)
    ap.add_argument("--controls", type=int, default=1)
    a = ap.parse_args()
    if a.worker:
        return worker(a.root, bool(a.controls))
    if a.kernel_stats:
        with open(a.out) as f:
            rec = json.load(f)
        rec["kernel_trace"] = {"source": "rocprofv3 --kernel-trace --stats, a run of its own: ten replays of the step with controls after the warm-up "
                                         "steps (the eager warm-up launches are in the counts)", "kernels": kernel_stats(a.kernel_stats)}
        if a.kernel_trace:
            rec["kernel_trace"]["by_launch_size"] = kernel_trace(a.kernel_trace)
        with open(a.out, "w") as f:
            json.dump(rec, f, indent=1)
            f.write("\n")
        print(json.dumps(rec["kernel_trace"]))
        return
    sys.path.insert(0, ROOT)
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("train_controls_bench: needs a ROCm device")
    if a.trace:
        tr, batch, _ = _trainer(True)
        for _ in range(10):
            tr.step(*batch)
        torch.cuda.synchronize()
        return
    base_root = os.path.abspath(a.baseline) if a.baseline else ROOT
    variants = {"baseline": _Worker(base_root, False), "controls": _Worker(ROOT, True)}
    try:
        if a.baseline:
            assert variants["baseline"].info["package"].startswith(base_root), variants["baseline"].info
        t = {k: [] for k in variants}
        copies = []
        for rep in range(a.runs + 1):                  # run 0 is dropped
            for k, w in variants.items():
                ms = w.ask(f"run {a.steps}")["ms"]
                if rep:
                    t[k].append(ms)
            us = variants["controls"].ask(f"copy {a.copies}")["us"]
            if rep:
                copies.append(us)
        rec = {"device": torch.cuda.get_device_name(0), "workload": "GraphedTrainer step, HSIC, B = 8, 512 x 512, bfloat16, lmbda 0.0067",
               "controls": "clip_max_norm=1.0, skip_nonfinite=True",
               "baseline": "the parent commit's tree" if a.baseline else "this tree without step controls",
               "runs": a.runs, "steps_per_run": a.steps, "main_numel": variants["controls"].info["main_numel"],
               "aux_numel": variants["controls"].info["aux_numel"]}
        for k, w in variants.items():
            rec[k + "_step_ms"] = _med(t[k])
            rec[k + "_last"] = {n: round(v, 6) for n, v in w.ask("last").items()}
        rec["difference_ms"] = round(rec["controls_step_ms"]["median"] - rec["baseline_step_ms"]["median"], 4)
        rec["spread_ms"] = {k: round(rec[k + "_step_ms"]["max"] - rec[k + "_step_ms"]["min"], 4) for k in variants}
        rec["copy_main_flat_g_us"] = _med(copies)
        rec["copy_main_flat_g_gb_per_s"] = round(2 * 4 * rec["main_numel"] / rec["copy_main_flat_g_us"]["median"] / 1e3, 1)
        rec["bar_ms"] = round(max(rec["spread_ms"].values()) + 2 * rec["copy_main_flat_g_us"]["median"] / 1e3, 4)
        rec["difference_exceeds_spread_plus_two_copies"] = bool(rec["difference_ms"] > rec["bar_ms"])
    finally:
        for w in variants.values():
            w.close()
    with open(a.out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print(json.dumps(rec))


if __name__ == "__main__":
    main()

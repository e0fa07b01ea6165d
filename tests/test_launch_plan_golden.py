"""The launch plans of the convolution entry points are host logic: tile, K step and kernel family (hesic_conv2d_variant), the split-K
workspace sizes (hesic_conv2d_ws_bytes / _f32out_ws_bytes / _hilo_ws_bytes) and the weight gradient's K-slice counts and workspace
(hesic_conv2d_wgrad_nsplit / _ws_bytes).  tests/golden/launch_plans.json holds what the commit named inside it answered for a fixed grid
of descriptors; this test asserts that the library still answers the same, entry for entry.  No GPU: the queries launch nothing.

Run as a script (python tests/test_launch_plan_golden.py) to record the file from the library that is built."""
import ctypes as C
import json
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "launch_plans.json")
ENV = "HESIC_IGEMM_S1_PATCH"

BATCHES = (1, 4, 8)
MAPS = ((8, 8), (16, 16), (32, 32), (64, 64), (56, 68), (128, 128))
# name: Cin, Cout, k, stride, transposed, then the descriptor fields that differ from a plain 16-bit layer
LAYERS = {
    "128-128k5s2": (128, 128, 5, 2, 0, {}),
    "128-128k5s2t": (128, 128, 5, 2, 1, {}),
    "128-192k5s2": (128, 192, 5, 2, 0, {}),
    "192-128k5s1": (192, 128, 5, 1, 0, {}),
    "128-960k5s1": (128, 960, 5, 1, 0, {}),
    "128-2048k5s1_xps256": (128, 2048, 5, 1, 0, {"x_pix_stride": 256}),
    "192-192k3s1": (192, 192, 3, 1, 0, {}),
    "384-192k1s1": (384, 192, 1, 1, 0, {}),
    "960-128k5s1t": (960, 128, 5, 1, 1, {}),
    "32-32k3s1": (32, 32, 3, 1, 0, {}),
    "128-256k5s1_masked12": (128, 256, 5, 1, 0, {"tap_mask_lo": (1 << 12) - 1}),      # MaskedConv2d: a raster-order prefix of the taps
    "128-128k5s2_f32": (128, 128, 5, 2, 0, {"dtype": "F32"}),
    "128-128k5s2_wrongHo": (128, 128, 5, 2, 0, {"Ho": "+1"}),                          # refused: output size does not match
    "48-128k3s1_badCin": (48, 128, 3, 1, 0, {}),                                       # refused: Cin is no multiple of the K step
}


def _lib():
    from hesic_amd import _lib as L
    if not os.path.exists(L.LIB_PATH):
        import __graft_entry__ as ge
        ge.build()
    return L


def descriptors():
    L = _lib()
    for B in BATCHES:
        for H, W in MAPS:
            for name, (Cin, Cout, k, s, tr, extra) in LAYERS.items():
                if tr:
                    Ho, Wo = H * s, W * s
                else:
                    Ho, Wo = (H + 2 * (k // 2) - k) // s + 1, (W + 2 * (k // 2) - k) // s + 1
                d = L.ConvDesc(B, H, W, Cin, Ho, Wo, Cout, k, k, s, k // 2, tr, L.H16, 0, 0, Cin, 0, Cout, 0, 0)
                for f, v in extra.items():
                    if f == "dtype":
                        d.dtype = L.F32
                    elif f == "Ho":
                        d.Ho = Ho + 1
                    else:
                        setattr(d, f, v)
                yield f"B{B}_{H}x{W}_{name}", d


def _variant(l, d):
    v = (C.c_int32 * 4)(-1, -1, -1, -1)
    rc = l.hesic_conv2d_variant(C.byref(d), v)
    return [rc] + list(v) if rc == 0 else [rc, l.hesic_last_error().decode()]


def compute():
    """{descriptor name: {column: value}} from the library that is built, with the process's two planner settings put back afterwards."""
    l = _lib().lib()
    prev_env = os.environ.pop(ENV, None)
    prev_mode = l.hesic_conv2d_set_phase_fusion(1)
    out = {}
    try:
        for name, d in descriptors():
            e = {"variant": _variant(l, d)}
            for q in ("hesic_conv2d_ws_bytes", "hesic_conv2d_f32out_ws_bytes", "hesic_conv2d_hilo_ws_bytes", "hesic_conv2d_wgrad_ws_bytes"):
                e[q[len("hesic_conv2d_"):]] = int(getattr(l, q)(C.byref(d)))
                if e["variant"][0] != 0 and not q.startswith("hesic_conv2d_wgrad"):
                    e[q[len("hesic_conv2d_"):] + "_error"] = l.hesic_last_error().decode()
            e["wgrad_nsplit"] = [l.hesic_conv2d_wgrad_nsplit(C.byref(d), 0), l.hesic_conv2d_wgrad_nsplit(C.byref(d), 1)]
            for m in (0, 1, 2):
                os.environ[ENV] = str(m)
                e[f"variant_s1_patch{m}"] = _variant(l, d)
            os.environ.pop(ENV)
            for m in (0, 1, 2):
                l.hesic_conv2d_set_phase_fusion(m)
                e[f"variant_phase_fusion{m}"] = _variant(l, d)
            l.hesic_conv2d_set_phase_fusion(1)
            out[name] = e
    finally:
        l.hesic_conv2d_set_phase_fusion(prev_mode)
        if prev_env is not None:
            os.environ[ENV] = prev_env
    return out


def test_launch_plans_match_the_recorded_ones():
    with open(GOLDEN) as f:
        gold = json.load(f)["plans"]
    now = compute()
    assert sorted(now) == sorted(gold)
    assert len(now) == len(BATCHES) * len(MAPS) * len(LAYERS)
    bad = [f"{name}.{col}: recorded {gold[name].get(col)!r}, now {now[name].get(col)!r}"
           for name in gold for col in sorted(set(gold[name]) | set(now[name])) if gold[name].get(col) != now[name].get(col)]
    assert not bad, f"{len(bad)} plan entries changed:\n" + "\n".join(bad[:40])


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(HERE))
    commit = subprocess.check_output(["git", "-C", HERE, "rev-parse", "HEAD"], text=True).strip()
    plans = compute()
    with open(GOLDEN, "w") as f:
        f.write('{"recorded_from_commit": "%s",\n "plans": {\n' % commit)
        f.write(",\n".join(f"  {json.dumps(k)}: {json.dumps(v, separators=(',', ':'))}" for k, v in plans.items()))
        f.write("\n }}\n")
    print(f"{len(plans)} descriptors recorded from {commit} -> {GOLDEN}")

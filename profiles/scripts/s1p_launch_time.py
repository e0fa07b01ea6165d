"""The stride-1 5 x 5 128 -> 960 launches of the entropy-parameter nets (grouped 2 x (128 -> 960) fp32-only, plain 128 -> 960), float16 build:
igemm_glds_kernel's staged x tiles (HESIC_IGEMM_S1_PATCH=0) against the resident input patch (igemm_s1p_kernel, =2), alternating in one
process, 3 x 100 launches each between HIP events, on the shapes the auto rule of hesic_conv2d_forward was set from.  Prints one line per
shape: the variant each mode selects, us per launch of every repeat, and whether the outputs are bit-identical.
usage: python profiles/scripts/s1p_launch_time.py [<float16 library> [<tag> [<modes, e.g. 0,2>]]]   (from the repository root;
writes profiles/s1p_launch_time_<tag>.json)"""
import ctypes as C
import json
import os
import sys

import torch

sys.path.insert(0, os.getcwd())
from hesic_amd import _lib as L  # noqa: E402

if len(sys.argv) > 1:
    L.LIB_PATH_F16 = os.path.abspath(sys.argv[1])
tag = sys.argv[2] if len(sys.argv) > 2 else "run"
modes = [int(m) for m in (sys.argv[3] if len(sys.argv) > 3 else "0,2").split(",")]
import hesic_amd  # noqa: E402

hesic_amd.set_compute_dtype(torch.float16)
dev = "cuda"
ENV = "HESIC_IGEMM_S1_PATCH"

SHAPES = [
    # name, B, H, W, grouped
    ("grouped_b8_32x32", 8, 32, 32, True),
    ("plain_b8_32x32", 8, 32, 32, False),
    ("grouped_b4_56x68", 4, 56, 68, True),
    ("plain_b4_56x68", 4, 56, 68, False),
    ("grouped_b4_32x32", 4, 32, 32, True),
    ("plain_b4_32x32", 4, 32, 32, False),
    ("grouped_b1_32x32", 1, 32, 32, True),
    ("plain_b1_32x32", 1, 32, 32, False),
    ("grouped_b2_32x32", 2, 32, 32, True),
    ("grouped_b8_16x16", 8, 16, 16, True),
    ("plain_b16_32x32", 16, 32, 32, False),
]
N, REPS = 100, 3
res = {}
for name, B, H, W, grouped in SHAPES:
    xc = 256 if grouped else 128
    cout = 2048 if grouped else 960
    x = (torch.randn(B, H, W, xc, device=dev) * 0.5).half()
    wp = (torch.randn(25 * cout * 128, device=dev) * 0.03).half()
    bias = torch.randn(cout, device=dev) * 0.1
    y32 = torch.empty(B, H, W, cout, device=dev, dtype=torch.float32)
    y16 = torch.empty(B, H, W, cout, device=dev, dtype=torch.float16)
    d = L.ConvDesc(B, H, W, 128, H, W, cout, 5, 5, 1, 2, 0, L.H16, 0, 0, xc, 0, cout, 0, 0)
    st = L.stream()

    def launch():
        if grouped:
            L.call("hesic_conv2d_forward_grouped", C.byref(d), 2, 128, L.ACT_NONE, 1024, L.ptr(x), L.ptr(wp), L.ptr(bias), None, L.ptr(y32), cout, 0, st)
        else:
            L.call("hesic_conv2d_forward", C.byref(d), L.ptr(x), L.ptr(wp), L.ptr(bias), L.ptr(y16), st)
    times = {m: [] for m in modes}
    var = {}
    outs = {}
    for rep in range(REPS):
        for m in modes:
            os.environ[ENV] = str(m)
            v = (C.c_int32 * 4)()
            L.call("hesic_conv2d_variant", C.byref(d), v)
            var[m] = list(v)
            for _ in range(10):
                launch()
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(N):
                launch()
            e1.record()
            torch.cuda.synchronize()
            times[m].append(e0.elapsed_time(e1) * 1000.0 / N)
            outs[m] = (y32 if grouped else y16).clone()
    same = all(torch.equal(outs[modes[0]], outs[m]) for m in modes[1:])
    res[name] = {"variant": {str(m): var[m] for m in modes}, "us": {str(m): [round(t, 2) for t in times[m]] for m in modes}, "equal": same}
    print(tag, name, json.dumps(res[name]), flush=True)
json.dump(res, open(os.path.join("profiles", f"s1p_launch_time_{tag}.json"), "w"), indent=1)

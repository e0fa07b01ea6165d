"""The weight-gradient launchers' host decisions: K-slice counts (hesic_conv2d_wgrad_nsplit), workspace sizes (hesic_conv2d_wgrad_ws_bytes /
_ws_bytes_n, hesic_gdn_backward_ws_bytes, hesic_sconv2d_wgrad_ws_bytes), hesic_gdn_backward_partial_ok, and the return code and error text of
the calls the entry points refuse before they launch anything.  tests/golden/wgrad_plans.json holds what the commit named inside it answered;
this test asserts that the library still answers the same, entry for entry.  No GPU: queries and refused calls only.

Run as a script (python tests/test_wgrad_plan_golden.py) to record the file from the library that is built."""
import ctypes as C
import json
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "wgrad_plans.json")
ENVS = {"default": {}, "row0": {"HESIC_WGRAD_ROW": "0"}, "row1_minq0": {"HESIC_WGRAD_ROW": "1", "HESIC_WGRAD_ROW_MINQ": "0"}}
ENV_NAMES = ("HESIC_WGRAD_ROW", "HESIC_WGRAD_ROW_MINQ")

GDN_P = (1, 64, 85, 86, 128, 129, 4096, 32768, (1 << 22) - 1, 1 << 22)      # 85 | 86: the largest of the three size terms changes


def _L():
    sys.path.insert(0, HERE)
    import test_launch_plan_golden as G
    return G, G._lib()


def _conv(L, B, H, W, Cin, Cout, k, s, tr, dtype=None, **extra):
    if tr:
        Ho, Wo = H * s, W * s
    else:
        Ho, Wo = (H + 2 * (k // 2) - k) // s + 1, (W + 2 * (k // 2) - k) // s + 1
    d = L.ConvDesc(B, H, W, Cin, Ho, Wo, Cout, k, k, s, k // 2, tr, L.H16 if dtype is None else dtype, 0, 0, Cin, 0, Cout, 0, 0)
    for f, v in extra.items():
        setattr(d, f, v)
    return d


def descriptors():
    G, L = _L()
    yield from G.descriptors()
    # wgrad_row_kernel candidates (5x5, stride 2, QW % 64 == 0) on both sides of its 100 000-pixel threshold: Q = 65536 | 131072
    for B in (4, 8):
        yield f"row_B{B}_256x256_128-128k5s2", _conv(L, B, 256, 256, 128, 128, 5, 2, 0)
        yield f"row_B{B}_128x128_128-128k5s2t", _conv(L, B, 128, 128, 128, 128, 5, 2, 1)
    for P in (64, 4096, 9216, 32768, 1 << 20):                         # the GDN parameter gradient: a 1x1 layer over P pixels
        yield f"gdn_P{P}_128-128k1", _conv(L, 1, 1, P, 128, 128, 1, 1, 0)
    for B, H in ((1, 16), (8, 64)):
        yield f"B{B}_{H}x{H}_128-128k5s1_mask_no_prefix", _conv(L, B, H, H, 128, 128, 5, 1, 0, tap_mask_lo=0x155555)
        yield f"B{B}_{H}x{H}_128-128k7s1", _conv(L, B, H, H, 128, 128, 7, 1, 0)                      # 49 taps: more than the 25 a launch takes
        yield f"B{B}_{H}x{H}_128-128k5s2_coff", _conv(L, B, H, H, 128, 128, 5, 2, 0, x_pix_stride=256, x_c_off=64, y_pix_stride=192, y_c_off=64)
        yield f"B{B}_{H}x{H}_128-192k3s1_f32", _conv(L, B, H, H, 128, 192, 3, 1, 0, dtype=L.F32)
        yield f"B{B}_{H}x{H}_192-128k5s2t_f32", _conv(L, B, H, H, 192, 128, 5, 2, 1, dtype=L.F32)
        yield f"B{B}_{H}x{H}_128-128k5s1_f32_masked12", _conv(L, B, H, H, 128, 128, 5, 1, 0, dtype=L.F32, tap_mask_lo=(1 << 12) - 1)


def _sconv(L, B, H, W, Cin, Cout, s, tr, x_dtype, y_dtype, x_nhwc, y_nhwc):
    Ho, Wo = (H * s, W * s) if tr else (H // s, W // s)

    def strides(C_, h, w, nhwc):
        return (h * w * C_, 1, w * C_, C_) if nhwc else (C_ * h * w, h * w, w, 1)
    return L.SConvDesc(B, H, W, Cin, Ho, Wo, Cout, 5, 5, s, 2, tr, x_dtype, y_dtype, 0, 0, *strides(Cin, H, W, x_nhwc), *strides(Cout, Ho, Wo, y_nhwc))


def sconv_descriptors():
    _, L = _L()
    for B, H in ((1, 64), (8, 256)):
        yield f"conv1_B{B}_{H}", _sconv(L, B, H, H, 3, 128, 2, 0, L.F32, L.H16, False, True)
        yield f"deconv4_B{B}_{H // 2}", _sconv(L, B, H // 2, H // 2, 128, 3, 2, 1, L.H16, L.F32, True, False)
        yield f"6-3s1_B{B}_{H}", _sconv(L, B, H, H, 6, 3, 1, 0, L.F32, L.F32, False, False)
    yield "3-64s2_B1_64_no_fast_case", _sconv(L, 1, 64, 64, 3, 64, 2, 0, L.F32, L.H16, False, True)


def _refusals(l, L):
    """name -> [return code, hesic_last_error text].  Every call here is refused by an argument check that runs before the first launch; the
    pointers are host buffers that nothing dereferences."""
    buf = (C.c_char * 256)()
    p = C.cast(buf, C.c_void_p)
    big = 1 << 40
    ok = _conv(L, 1, 16, 16, 128, 128, 5, 2, 0)
    cin36 = _conv(L, 1, 16, 16, 36, 128, 5, 2, 0)
    k7 = _conv(L, 1, 16, 16, 128, 128, 7, 1, 0)
    out = {}

    def rec(name, rc):
        out[name] = [int(rc), l.hesic_last_error().decode()]

    def arr(ty, *v):
        return (ty * len(v))(*v)

    def batched(d, x, ws_bytes, nsplit=None):
        return l.hesic_conv2d_wgrad_partial_batched(1, C.byref(d), arr(C.c_void_p, x), arr(C.c_void_p, p.value), arr(C.c_void_p, p.value),
                                                    arr(C.c_int64, ws_bytes), nsplit, None)
    need_packed = int(l.hesic_conv2d_wgrad_ws_bytes(C.byref(ok))) - int(l.hesic_conv2d_wgrad_nsplit(C.byref(ok), 0)) * 4 * 128 * 4
    need = int(l.hesic_conv2d_wgrad_ws_bytes(C.byref(ok)))
    need_b = int(l.hesic_conv2d_wgrad_ws_bytes_n(C.byref(ok), l.hesic_conv2d_wgrad_nsplit(C.byref(ok), 1)))
    for case, d, x, small in (("cin36", cin36, p, False), ("taps49", k7, p, False), ("null", ok, None, False), ("ws_short", ok, p, True)):
        rec(f"wgrad.{case}", l.hesic_conv2d_wgrad(C.byref(d), x, p, p, None, p, need_packed - 1 if small else big, None))
        rec(f"wgrad_direct.{case}", l.hesic_conv2d_wgrad_direct(C.byref(d), x, p, p, None, 0, p, need - 1 if small else big, None))
        rec(f"wgrad_partial.{case}", l.hesic_conv2d_wgrad_partial(C.byref(d), x, p, p, need - 1 if small else big, None))
        rec(f"wgrad_partial_batched.{case}", batched(d, x.value if x else None, need - 1 if small else big))
    rec("wgrad_partial_batched.ws_short_named_count",
        batched(ok, p.value, need_b - 1, arr(C.c_int32, l.hesic_conv2d_wgrad_nsplit(C.byref(ok), 1))))
    row = _conv(L, 8, 256, 256, 128, 128, 5, 2, 0)
    rec("wgrad_partial_batched.row_layer_named_count_disagrees", batched(row, p.value, big, arr(C.c_int32, l.hesic_conv2d_wgrad_nsplit(C.byref(row), 0) + 1)))
    two = (L.ConvDesc * 2)(ok, ok)
    pp, nul = arr(C.c_void_p, p.value, p.value), arr(C.c_void_p, None, None)
    rec("wgrad_finish_batched_n.shared_dw", l.hesic_conv2d_wgrad_finish_batched_n(2, two, pp, pp, pp, nul, 1, None, None))
    mixed = (L.ConvDesc * 2)(ok, _conv(L, 1, 16, 16, 128, 128, 5, 2, 0, dtype=L.F32))
    dws = arr(C.c_void_p, p.value, p.value + 64)
    rec("wgrad_finish_batched_n.mixed_dtypes", l.hesic_conv2d_wgrad_finish_batched_n(2, mixed, pp, pp, dws, nul, 1, None, None))
    rec("gdn_backward_partial.C3", l.hesic_gdn_backward_partial(p, p, p, p, p, p, 4096, 3, 0, 1e-6, L.H16, None))
    rec("gdn_param_finish_batched.repeated_dgamma",
        l.hesic_gdn_param_finish_batched(2, pp, arr(C.c_int64, 4096, 4096), pp, pp, pp, dws, arr(C.c_float, 1e-6, 1e-6), 0, None))
    return out


def compute():
    """{section: {name: value}} from the library that is built; the two environment switches are put back afterwards."""
    _, L = _L()
    l = L.lib()
    prev = {k: os.environ.pop(k, None) for k in ENV_NAMES}
    out = {"conv": {}, "gdn": {}, "sconv": {}, "refused": {}}
    try:
        for name, d in descriptors():
            e = {}
            for env, vals in ENVS.items():
                os.environ.update(vals)
                ns = [l.hesic_conv2d_wgrad_nsplit(C.byref(d), 0), l.hesic_conv2d_wgrad_nsplit(C.byref(d), 1)]
                e[env] = {"nsplit": ns, "ws_bytes": int(l.hesic_conv2d_wgrad_ws_bytes(C.byref(d))),
                          "ws_bytes_n": {str(n): int(l.hesic_conv2d_wgrad_ws_bytes_n(C.byref(d), n)) for n in (1, 3, ns[1], 300)}}
                for k in vals:
                    os.environ.pop(k)
            out["conv"][name] = e
        for P in GDN_P:
            out["gdn"][f"P{P}"] = {"ws_bytes": {str(c): int(l.hesic_gdn_backward_ws_bytes(P, c)) for c in (3, 128, 192)},
                                   "partial_ok": {f"C{c}_{n}": l.hesic_gdn_backward_partial_ok(P, c, dt)
                                                  for c in (3, 128) for n, dt in (("h16", L.H16), ("f32", L.F32))}}
        for name, d in sconv_descriptors():
            out["sconv"][name] = int(l.hesic_sconv2d_wgrad_ws_bytes(C.byref(d)))
        out["refused"] = _refusals(l, L)
    finally:
        for k in ENV_NAMES:
            os.environ.pop(k, None)
            if prev[k] is not None:
                os.environ[k] = prev[k]
    return out


def test_wgrad_plans_match_the_recorded_ones():
    with open(GOLDEN) as f:
        gold = json.load(f)["plans"]
    now = compute()
    assert sorted(now) == sorted(gold)
    bad = []
    for sec in gold:
        assert sorted(now[sec]) == sorted(gold[sec]), sec
        bad += [f"{sec}.{name}: recorded {gold[sec][name]!r}, now {now[sec][name]!r}" for name in gold[sec] if gold[sec][name] != now[sec][name]]
    assert not bad, f"{len(bad)} entries changed:\n" + "\n".join(bad[:40])
    # the grid is the one that was asked for, and the refused calls were refused
    assert len(now["gdn"]) == len(GDN_P) and len(now["sconv"]) == 7 and len(now["refused"]) == 22
    assert all(rc != 0 and text for rc, text in now["refused"].values())


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(HERE))
    commit = subprocess.check_output(["git", "-C", HERE, "rev-parse", "HEAD"], text=True).strip()
    plans = compute()
    with open(GOLDEN, "w") as f:
        f.write('{"recorded_from_commit": "%s",\n "plans": {\n' % commit)
        secs = []
        for sec, entries in plans.items():
            secs.append('  %s: {\n' % json.dumps(sec) + ",\n".join(f"   {json.dumps(k)}: {json.dumps(v, separators=(',', ':'))}" for k, v in entries.items()) + "\n  }")
        f.write(",\n".join(secs))
        f.write("\n }}\n")
    print(f"{sum(len(v) for v in plans.values())} entries recorded from {commit} -> {GOLDEN}")

"""Per-pair rate-distortion metrics, the parts that need no GPU: the fp64 restatement the GPU tests hold the kernel to (tests/pair_metrics_ref.py)
against the reference's definitions -- the criterion of ywz/mywork/test3real.py:90-122 at batch 1 (``nn.MSELoss``, ``mse2psnr``, the
``log(...).sum() / (-ln 2 * num_pixels)`` bits), ``codec.quantise``'s uint8 images, ``AverageMeter`` --, the C ABI of
include/hesic_pair_metrics.h with its refusals, and the host logic of ``python -m hesic_amd.eval_folder``."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest
import torch

import pair_metrics_ref as R
from hesic_amd import codec, synthetic

KEYS = ("y1", "y2", "z1", "z2")


def _lib():
    from hesic_amd import _lib as L
    if not (os.path.exists(L.LIB_PATH) and os.path.exists(L.LIB_PATH_F16)):
        import __graft_entry__ as ge
        ge.build()
    return L


def _batch(B=3, h=20, w=28):
    """A small random forward: reconstructions around the originals (some values outside [0, 1]) and four likelihood maps."""
    x1 = synthetic._uniform("pm.cpu.x1", (B, 3, h, w), 0, 1)
    x2 = synthetic._uniform("pm.cpu.x2", (B, 3, h, w), 0, 1)
    x1_hat = x1 + synthetic._uniform("pm.cpu.e1", (B, 3, h, w), -0.1, 0.1)
    x2_hat = x2 + synthetic._uniform("pm.cpu.e2", (B, 3, h, w), -0.05, 0.05)
    shapes = {"y1": (B, 12, 5, 7), "y2": (B, 12, 5, 7), "z1": (B, 8, 2, 2), "z2": (B, 8, 2, 2)}
    liks = {k: (1e-9 + synthetic._uniform("pm.cpu.l" + k, s, 0, 1) ** 2).clamp(max=1.0).float() for k, s in shapes.items()}
    return x1.float(), x2.float(), x1_hat.float(), x2_hat.float(), liks


# ------------------------------------------------------------------------------------------- the restatement against the reference
def test_restatement_equals_the_reference_criterion_at_batch_one():
    x1, x2, x1_hat, x2_hat, liks = _batch()
    B, _, h, w = x1.shape
    tab = R.table([liks[k] for k in KEYS], [(x1_hat, x1), (x2_hat, x2)])
    fig = R.figures(tab, KEYS, h, w)
    mse = torch.nn.MSELoss()
    for b in range(B):
        t1, t2, o1, o2 = (t[b:b + 1].double() for t in (x1, x2, x1_hat, x2_hat))
        N, _, H, W = t1.size()
        num_pixels = N * H * W                                      # test3real.py:91-93 with N = 1
        bpp_loss = sum(float(torch.log(liks[k][b:b + 1].double()).sum() / (-math.log(2) * num_pixels)) for k in KEYS)       # :115-117
        m1, m2 = float(mse(o1, t1)), float(mse(o2, t2))
        p1, p2 = 10 * math.log10(1 / m1), 10 * math.log10(1 / m2)   # mse2psnr, :69-72, 110-111
        for name, want in (("bpp_loss", bpp_loss), ("bpp", bpp_loss / 2), ("mse1", m1), ("mse2", m2), ("psnr1", p1), ("psnr2", p2),
                           ("psnr", (p1 + p2) / 2)):
            assert abs(fig[name][b] - want) <= 1e-12 * abs(want), (name, b, fig[name][b], want)
        for k in KEYS:
            want = float(torch.log(liks[k][b].double()).sum() / -math.log(2))
            assert abs(fig["bits"][k][b] - want) <= 1e-12 * abs(want)


def test_sse8_is_the_squared_error_of_the_quantised_images():
    x1, x2, x1_hat, x2_hat, liks = _batch()
    x1_hat = x1_hat.clone()
    x1_hat[0, 0, 0, :10] = torch.tensor([-0.2, 1.3, 0.5 / 255, 1.5 / 255, 2.5 / 255, 254.5 / 255, 0.0, 1.0, -0.0, 127.5 / 255])
    tab = R.table([], [(x1_hat, x1), (x2_hat, x2)])
    for col, (a, b) in ((2, (x1_hat, x1)), (3, (x2_hat, x2))):
        qa, qb = codec.quantise(a).astype(np.int64), codec.quantise(b).astype(np.int64)
        want = ((qa - qb) ** 2).reshape(qa.shape[0], -1).sum(1)
        assert np.array_equal(tab[:, col], want.astype(np.float64))
    fig = R.figures(tab, (), 20, 28)
    mse8 = tab[:, 2] / (20 * 28 * 3)
    assert np.allclose(fig["psnr8_1"], 10 * np.log10(255.0 ** 2 / mse8), rtol=1e-14)


def test_zero_error_is_100_db_and_nan_stays_in_its_row():
    x1, x2, x1_hat, x2_hat, liks = _batch()
    x1_hat = x1_hat.clone()
    x1_hat[0] = x1[0]
    x1_hat[2, 1, 3, 4] = float("nan")
    tab = R.table([liks["y1"]], [(x1_hat, x1), (x2_hat, x2)])
    fig = R.figures(tab, ("y1",), 20, 28)
    assert tab[0, 1] == 0 and tab[0, 3] == 0 and fig["psnr1"][0] == 100.0 and fig["psnr8_1"][0] == 100.0
    assert np.isnan(tab[2, 1]) and np.isnan(tab[2, 3]) and np.isnan(fig["psnr"][2]) and np.isnan(fig["psnr8"][2])
    assert np.isfinite(tab[1]).all() and np.isfinite(tab[:, [0, 2, 4]]).all()


def test_pair_metrics_from_equals_the_restatement_on_host_tensors():
    from hesic_amd import models
    x1, x2, x1_hat, x2_hat, liks = _batch()
    x1_hat = x1_hat.clone()
    x1_hat[1] = x1[1]
    tab = R.table([liks[k] for k in KEYS], [(x1_hat, x1), (x2_hat, x2)])
    t = torch.from_numpy(tab)
    pm = {"bits_" + k: -t[:, i] for i, k in enumerate(KEYS)}
    pm.update(sse1=t[:, 4], sse2=t[:, 5], sse8_1=t[:, 6], sse8_2=t[:, 7], num_pixels=20 * 28)
    got, want = models.pair_metrics_from(pm), R.figures(tab, KEYS, 20, 28)
    assert set(got) == set(want) and list(got["bits"]) == list(KEYS)
    for k, v in want.items():
        if k == "bits":
            for kk in KEYS:
                assert np.array_equal(got["bits"][kk].numpy(), v[kk])
        else:
            assert got[k].dtype == torch.float64 and np.allclose(got[k].numpy(), v, rtol=1e-12, atol=0), k
    assert float(got["psnr1"][1]) == 100.0 and float(got["psnr8_1"][1]) == 100.0


class AverageMeter:
    """test3real.py:127-139, restated."""

    def __init__(self):
        self.val, self.avg, self.sum, self.count = 0, 0, 0, 0

    def update(self, val, n=1):
        self.val = val
        self.sum += val * n
        self.count += n
        self.avg = self.sum / self.count


def _records(n=5):
    from hesic_amd import eval_folder
    g = np.random.Generator(np.random.PCG64(7))
    recs = []
    for i in range(n):
        r = {"stem": f"p{i}", "height": 64, "width": 70}
        r.update({k: float(g.uniform(0.1, 40)) for k in eval_folder.FIGURES})
        r["mse1"], r["mse2"] = float(g.uniform(1e-4, 1e-2)), float(g.uniform(1e-4, 1e-2))
        r["bits"] = {k: float(g.uniform(10, 1e4)) for k in KEYS}
        big = i % 2 == 0
        r.update({k: (float(g.uniform(0.9, 1)) if big else None) for k in eval_folder.MS_SSIM_FIELDS})
        r["coded_bpp"] = float(g.uniform(0.1, 1))
        recs.append(r)
    return recs


def test_summarise_reproduces_average_meter_over_batch_one_updates():
    from hesic_amd import eval_folder
    recs = _records()
    s = eval_folder.summarise(recs)
    assert s["pairs"] == 5
    for k in eval_folder.FIGURES + ("coded_bpp",):
        m = AverageMeter()
        for r in recs:
            m.update(r[k])
        assert s[k] == m.avg, k
    for k in KEYS:
        m = AverageMeter()
        for r in recs:
            m.update(r["bits"][k])
        assert s["bits"][k] == m.avg
    for k in eval_folder.MS_SSIM_FIELDS:
        m = AverageMeter()
        for r in recs:
            if r[k] is not None:
                m.update(r[k])
        assert m.count == 3 and s[k] == m.avg
    want = (10 * math.log10(1 / s["mse1"]) + 10 * math.log10(1 / s["mse2"])) / 2
    assert s["psnr_of_mean_mse"] == want and s["psnr_of_mean_mse"] != s["psnr"]
    for r in recs:
        r.update({k: None for k in eval_folder.MS_SSIM_FIELDS})
        del r["coded_bpp"]
    s = eval_folder.summarise(recs)
    assert all(s[k] is None for k in eval_folder.MS_SSIM_FIELDS) and "coded_bpp" not in s
    assert eval_folder.summarise([])["pairs"] == 0


# ------------------------------------------------------------------------------------------------------------------------ ABI
@pytest.mark.parametrize("fmt", ["bf16", "f16"])
def test_abi_header_bindings_exports(fmt):
    L = _lib()
    declared = L.declared_symbols("hesic_pair_metrics.h")
    assert declared == ["hesic_pair_metrics", "hesic_pair_metrics_ws_bytes"]
    assert set(declared) == set(L._PAIR_METRICS_SIGS)
    assert not set(declared) & set(L.declared_symbols())                # a header of its own: include/hesic_hip.h does not list it
    assert "hesic_pair_metrics.h" not in open(L.header_path("hesic_hip.h")).read()
    assert "#define HESIC_PAIR_METRICS_MAX_LIK 8" in open(L.header_path("hesic_pair_metrics.h")).read() and L.PAIR_METRICS_MAX_LIK == 8
    exported = subprocess.check_output(["nm", "-D", "--defined-only", L.LIB_PATH_F16 if fmt == "f16" else L.LIB_PATH], text=True)
    for s in declared:
        assert f" T {s}\n" in exported, s
    L.lib(torch.float16 if fmt == "f16" else torch.bfloat16)            # binds every signature, the new ones included


def _call_raw(lib, **kw):
    """hesic_pair_metrics with host dummies for pointers: every case below is refused before anything is launched or dereferenced on the device."""
    buf = (C.c_double * 16)()
    p = C.cast(buf, C.c_void_p)
    two = (C.c_void_p * 2)(p, p)
    a = dict(B=2, n_lik=2, lik=(C.c_void_p * 8)(*([p] * 8)), numel=(C.c_int64 * 8)(*([64] * 8)), a=two, a_dtype=(C.c_int32 * 2)(0, 0),
             a_strides=(C.c_int64 * 8)(48, 16, 4, 1, 48, 16, 4, 1), b=two, b_dtype=(C.c_int32 * 2)(0, 1),
             b_strides=(C.c_int64 * 8)(48, 16, 4, 1, 48, 16, 4, 1), C=3, H=4, W=4, out=p, ws=p, ws_bytes=1 << 20)
    a.update(kw)
    return lib.hesic_pair_metrics(a["B"], a["n_lik"], a["lik"], a["numel"], a["a"], a["a_dtype"], a["a_strides"], a["b"], a["b_dtype"],
                                  a["b_strides"], a["C"], a["H"], a["W"], a["out"], a["ws"], a["ws_bytes"], None)


def _numel(*v):
    return (C.c_int64 * 8)(*(list(v) + [64] * (8 - len(v))))


def _ptrs(n_null):
    buf = (C.c_double * 16)()
    p = C.cast(buf, C.c_void_p).value
    return (C.c_void_p * 2)(*[None if i == n_null else p for i in range(2)])


@pytest.mark.parametrize("bad, word", [
    (dict(out=None), "null"), (dict(ws=None), "null"), (dict(a=None), "null"), (dict(b_strides=None), "null"), (dict(lik=None), "null"),
    (dict(numel=None), "null"), (dict(a=_ptrs(1)), "null"), (dict(b=_ptrs(0)), "null"),
    (dict(lik=(C.c_void_p * 8)()), "null"),
    (dict(n_lik=9), "outside 0..8"), (dict(n_lik=-1), "outside 0..8"),
    (dict(numel=_numel(64, 63)), "multiple of B"), (dict(B=3), "multiple of B"), (dict(numel=_numel(0)), "non-positive"),
    (dict(B=0), "non-positive"), (dict(C=0), "non-positive"), (dict(H=0), "non-positive"), (dict(W=-4), "non-positive"),
    (dict(H=1 << 16, W=1 << 15), "2^31"), (dict(H=46341, W=46341), "2^31"),
    (dict(ws_bytes=0), "workspace too small"), (dict(ws_bytes=2 * (1 + 1 + 2 + 2) * 8 - 1), "workspace too small"),
    (dict(a_dtype=(C.c_int32 * 2)(0, 7)), "dtype"),
], ids=lambda v: "-".join(f"{k}" for k in v) if isinstance(v, dict) else str(v).replace(" ", "_"))
def test_bad_arguments_return_einval_with_a_message(bad, word):
    lib = _lib().lib()
    assert _call_raw(lib, **bad) == -1
    msg = lib.hesic_last_error().decode()
    assert msg.startswith("pair_metrics:") and word in msg, msg


def test_ws_bytes_counts_the_partials_and_refuses_what_the_call_refuses():
    lib = _lib().lib()
    ws = lib.hesic_pair_metrics_ws_bytes
    one = (C.c_int64 * 1)
    assert ws(2, 0, None, 4, 4) == 2 * 2 * 2 * 8                        # two image pairs, one block an image, two sums a block
    assert ws(2, 1, one(2 * 4096), 4, 4) == (2 * 1 + 8) * 8 and ws(2, 1, one(2 * 4097), 4, 4) == (2 * 2 + 8) * 8
    assert ws(1, 1, one(10 ** 9), 4, 4) == (32 + 4) * 8                 # the cap on a likelihood map's blocks
    assert ws(1, 0, None, 32, 32) == 4 * 8 and ws(1, 0, None, 32, 33) == 8 * 8 and ws(1, 0, None, 4096, 4096) == 64 * 4 * 8
    # the block count of an image never depends on B: B images need B times the partials of one
    assert ws(8, 2, (C.c_int64 * 2)(8 * 196608, 8 * 8192), 512, 512) == 8 * ws(1, 2, (C.c_int64 * 2)(196608, 8192), 512, 512)
    for args, word in (((2, 1, one(7), 4, 4), "multiple of B"), ((0, 0, None, 4, 4), "non-positive"), ((1, 9, one(4), 4, 4), "outside 0..8"),
                       ((1, 1, None, 4, 4), "null"), ((1, 0, None, 65536, 32768), "2^31")):
        assert ws(*args) == -1
        msg = lib.hesic_last_error().decode()
        assert msg.startswith("pair_metrics_ws_bytes:") and word in msg, msg


def test_wrapper_refuses_cpu_tensors_and_bad_shapes():
    from hesic_amd import functional as Fn
    x = torch.zeros(2, 3, 4, 4)
    with pytest.raises(ValueError, match="two image pairs"):
        Fn.pair_metrics([], [(x, x)])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        Fn.pair_metrics([], [(x, x), (x, x)])


# ------------------------------------------------------------------------------------------------------------- the command's host logic
def _write_pair(root, split, stem, h, w, H=None, seed=0):
    from PIL import Image
    g = np.random.Generator(np.random.PCG64([9, seed]))
    for side in ("left", "right"):
        d = root / split / side
        d.mkdir(parents=True, exist_ok=True)
        Image.fromarray(g.integers(0, 256, size=(h, w, 3), dtype=np.uint8)).save(d / f"{stem}.png")
    if H is not None:
        (root / split / "H").mkdir(exist_ok=True)
        np.save(root / split / "H" / f"{stem}.npy", H)


def test_parser_defaults():
    from hesic_amd import eval_folder
    a = eval_folder.parser().parse_args(["root"])
    assert (a.root, a.split, a.batch, a.model, a.checkpoint, a.dtype, a.homography, a.homography_checkpoint, a.enhancer, a.coded,
            a.channels_per_stream, a.out) == ("root", "test", 8, "hesic", None, "f16", "sidecar", None, None, False, 1, None)
    a = eval_folder.parser().parse_args(["r", "--coded", "--enhancer", "synthetic", "--homography", "net", "--model", "joint", "--dtype", "bf16"])
    assert a.coded and a.enhancer == "synthetic" and a.homography == "net" and a.model == "joint" and a.dtype == "bf16"
    for bad in (["r", "--dtype", "f64"], ["r", "--model", "x"], ["r", "--homography", "surf"], []):
        with pytest.raises(SystemExit):
            eval_folder.parser().parse_args(bad)


def test_plan_groups_by_size_cuts_chunks_and_skips_pairs_without_a_sidecar(tmp_path):
    from hesic_amd import eval_folder
    eye = np.eye(3)
    for i, (h, w, H) in enumerate([(20, 24, eye), (16, 40, eye), (20, 24, None), (20, 24, eye), (16, 40, eye), (20, 24, eye)]):
        _write_pair(tmp_path, "test", f"p{i}", h, w, H, seed=i)
    chunks, skipped = eval_folder.plan(tmp_path, "test", 2)
    assert skipped == 1
    assert [(size, [it[0] for it in items]) for size, items in chunks] == [((24, 20), ["p0", "p3"]), ((24, 20), ["p5"]), ((40, 16), ["p1", "p4"])]
    assert all(it[3] is not None for _, items in chunks for it in items)
    chunks, skipped = eval_folder.plan(tmp_path, "test", 8, sidecars=False)
    assert skipped == 0 and [[it[0] for it in items] for _, items in chunks] == [["p0", "p2", "p3", "p5"], ["p1", "p4"]]
    assert chunks[0][1][1][3] is None
    with pytest.raises(RuntimeError, match="0 left"):
        eval_folder.plan(tmp_path, "valid", 2)


def test_main_refuses_bad_flags_and_returns_2_without_a_device(tmp_path, capsys):
    from hesic_amd import eval_folder
    _write_pair(tmp_path, "test", "a", 20, 24, np.eye(3))
    for bad in (["--batch", "0"], ["--homography-checkpoint", "x.pth.tar"], ["--channels-per-stream", "0"]):
        with pytest.raises(SystemExit) as e:
            eval_folder.main([str(tmp_path), *bad], log=lambda s: None)
        assert e.value.code == 2
    capsys.readouterr()
    if not torch.cuda.is_available():
        assert eval_folder.main([str(tmp_path)], log=lambda s: None) == 2
        assert "needs a ROCm device" in capsys.readouterr().err

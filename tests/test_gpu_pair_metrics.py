"""``hesic_pair_metrics`` (csrc/pair_metrics.hip), ``models.pair_metrics*`` and ``python -m hesic_amd.eval_folder`` on a real MI355X.

Kernel cases: every tensor the call sees, the workspace included, is ``memguard.guarded``; the output table and the workspace start as NaN and
the guards are checked after the call.  The values are held to the fp64 restatement of tests/pair_metrics_ref.py with the units of
tests/glue_ref.py applied per image (``sum_log2_ref`` for the bits, c = 1; images on the 1/16 grid, where every fp64 partial is exact, must
match bit for bit; the 8-bit sums are integers and must be equal).  Each case prints  "pair_metrics <case> <column> <ratio>"  before it asserts."""
import ctypes as C
import json
import math

import numpy as np
import pytest
import torch

import glue_ref as G
import memguard
import pair_metrics_ref as R
from hesic_amd import synthetic

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF, F16, F32 = torch.bfloat16, torch.float16, torch.float32
CL = torch.channels_last


@pytest.fixture(autouse=True)
def _bf16_library():
    import hesic_amd
    hesic_amd.set_compute_dtype(BF)
    yield
    hesic_amd.set_compute_dtype(BF)
    hesic_amd.set_compute_dtype(F32)


def _imp():
    from hesic_amd import functional as Fn
    from hesic_amd import _lib as L
    return Fn, L


def _name(dt):
    return {BF: "bf16", F16: "f16", F32: "f32"}[dt]


def _g(t, name):
    return memguard.guarded(t.to(DEV) if not t.is_cuda else t, name=name)


def _guard(t, name):
    """``t`` guarded on the device; a tensor that is guarded already, or a device view of one (a window), is passed as it is."""
    if hasattr(t, "_memguard") or (t.is_cuda and t._base is not None):
        return t
    return _g(t, name)


def _run(liks, pairs):
    """The table of ``Fn.pair_metrics`` on guarded copies of everything, with a NaN-filled guarded table and workspace; (B, n_lik + 4) fp64
    on the host.  Every guard is checked after the call."""
    Fn, L = _imp()
    liks = [_guard(l, f"lik{i}") for i, l in enumerate(liks)]
    pairs = [tuple(_guard(t, f"img{s}") for t in p) for s, p in enumerate(pairs)]
    B, _, H, W = pairs[0][0].shape
    numel = (C.c_int64 * max(len(liks), 1))(*[l.numel() for l in liks])
    need = L.lib().hesic_pair_metrics_ws_bytes(B, len(liks), numel, H, W)
    assert need > 0
    ws = memguard.guarded(torch.full((need,), 0xFF, dtype=torch.uint8, device=DEV), name="workspace")
    out = memguard.guarded(torch.full((B, len(liks) + 4), float("nan"), dtype=torch.float64, device=DEV), name="table")
    got = Fn.pair_metrics(liks, pairs, out=out, ws=ws)
    torch.cuda.synchronize()
    assert got is out
    memguard.check_all(liks + [t for p in pairs for t in p] + [ws, out])
    return out.cpu().clone()


def _bar(case, col, R_, got):
    ok, ratio, msg = G.check(R_, got, c=1.0, name=f"{case} {col}")
    print(f"pair_metrics {case} {col} {ratio:.4f}")
    assert ok, msg
    assert ratio <= 1.0, msg


def _same(case, col, got, want):
    same = G.same_bits(got, want)
    print(f"pair_metrics {case} {col} {0.0 if same else math.inf:.4f}")
    assert same, f"{case} {col}: {got.tolist()} != {want.tolist()}"


def _liks(B, per, salt=0):
    """(B, per) likelihoods in [1e-9, 1] from the reduction tests' pool (tests/glue_ref.py)."""
    big = G.likelihoods("n300000")
    pool = torch.cat((big, big * 0.5 + 0.25, (big * 0.25 + 0.125)))
    n = B * per
    assert salt + n <= pool.numel()
    return pool[salt:salt + n].clone().reshape(B, per)


def _tiny_pairs(B, tag="t"):
    return [(G.grid16(f"pm.{tag}.a{s}", (B, 3, 2, 2)), G.grid16(f"pm.{tag}.b{s}", (B, 3, 2, 2))) for s in range(2)]


def _images(name, shape):
    """Image-like fp32 values in [-0.2, 1.2] that are on no grid: their sums depend on the order of the additions."""
    return synthetic._uniform("pm." + name, shape, -0.2, 1.2).float()


# ----------------------------------------------------------------------------------------------------------------------- bits
@pytest.mark.parametrize("B,per", [(3, 1), (3, 3), (3, 1027), (2, 300000)], ids=lambda v: str(v))
def test_bits_per_image(B, per):
    """per = 1, 3: the scalar tail alone; 1027: 256 four-element groups + a tail of 3, and image 1's slice starts 4-byte but not 16-byte
    aligned; 300000: more groups than one trip of the 32 blocks an image gets."""
    lik = _liks(B, per)
    Fn, L = _imp()
    ld = _g(lik, "lik")
    if per == 1027:
        assert ld.data_ptr() % 16 == 0 and (ld.data_ptr() + 4 * per) % 16 == 12
    got = _run([ld], _tiny_pairs(B))
    for b in range(B):
        _bar(f"bits_{B}x{per}", f"image{b}", G.sum_log2_ref(lik[b]), got[b, 0:1])
    assert np.array_equal(got[:, 1:].numpy(), R.table([], _tiny_pairs(B)))


# ------------------------------------------------------------------------------------------------------------- squared error
SSE_SHAPES = {"50x100_in_64x128": (3, 3, 50, 100), "2x2": (3, 3, 2, 2), "c5_9x7": (3, 5, 9, 7)}


def _hat(tag, s, shape, form, h16):
    """x_hat of pair s on the 1/16 grid: for the windowed shape a [..., :50, :100] view of a guarded (B, 3, 64, 128) tensor whose padding is NaN;
    ``form`` "h16_cl": 16-bit channels-last in the active format, "f32": dense fp32."""
    a = G.grid16(f"pm.sse.{tag}.a{s}", shape)
    B, Cc, H, W = shape
    if tag == "50x100_in_64x128":
        full = torch.full((B, Cc, 64, 128), float("nan"))
        full[..., :H, :W] = a
    else:
        full = a
    d = full.to(DEV, h16 if form == "h16_cl" else F32)
    if form == "h16_cl":
        d = d.contiguous(memory_format=CL)
    gd = memguard.guarded(d, name=f"x{s}_hat")
    return a, gd, gd[..., :H, :W]


@pytest.mark.parametrize("form,h16", [("h16_cl", BF), ("h16_cl", F16), ("f32", None)], ids=["h16cl-bf16", "h16cl-f16", "f32"])
@pytest.mark.parametrize("tag", list(SSE_SHAPES))
def test_sse_is_exact_on_the_grid(tag, form, h16):
    """Both squared-error columns bit for bit against fp64 (every partial sum is exact on the 1/16 grid, so the order cannot matter), for
    16-bit channels-last reconstructions against fp32 NCHW originals and for fp32 against fp32; the NaN padding around the 50 x 100 window
    would turn a read outside it into a NaN sum.  50 x 100: five blocks an image (one trip of the 4-pixel loop for 1160 lanes, the rest one by
    one); 2 x 2: the pixel loop alone; C = 5: the generic channel loop."""
    import hesic_amd
    if h16 is not None:
        hesic_amd.set_compute_dtype(h16)
    shape = SSE_SHAPES[tag]
    B = shape[0]
    hats = [_hat(tag, s, shape, form, h16) for s in range(2)]
    xs = [G.grid16(f"pm.sse.{tag}.b{s}", shape) for s in range(2)]
    lik = _liks(B, 5)
    got = _run([lik], [(hats[s][2], xs[s]) for s in range(2)])
    memguard.check_all([h[1] for h in hats])
    want = R.table([lik], [(hats[s][0], xs[s]) for s in range(2)])
    case = f"sse_{tag}_{form}" + (f"_{_name(h16)}" if h16 else "")
    for col, name in ((1, "sse1"), (2, "sse2"), (3, "sse8_1"), (4, "sse8_2")):
        _same(case, name, got[:, col], torch.from_numpy(want[:, col]))
    for s in range(2):
        for b in range(B):
            ok, ratio, msg = G.check(G.sum_sq_diff_ref(hats[s][0][b:b + 1], xs[s][b:b + 1]), got[b, 1 + s:2 + s], c=1.0, name=case)
            assert ok and ratio == 0.0, msg


def test_sse8_clamps_rounds_half_to_even_and_is_an_integer():
    """Values below 0, above 1 and every tie (k + 0.5) / 255 of the rounding: equal to the restatement's integers, which
    tests/test_pair_metrics_cpu.py holds to ``codec.quantise``'s uint8 images."""
    B, Cc, H, W = 3, 3, 9, 37
    a = synthetic._uniform("pm.q8.a", (B, Cc, H, W), -0.3, 1.3).float()
    b = synthetic._uniform("pm.q8.b", (B, Cc, H, W), -0.3, 1.3).float()
    ties = ((torch.arange(255, dtype=torch.float32) + 0.5) / 255.0)
    a.reshape(B, -1)[0, :255] = ties
    b.reshape(B, -1)[1, 100:355] = ties
    a.reshape(B, -1)[2, :6] = torch.tensor([0.0, -0.0, 1.0, 1.0 + 2 ** -20, -1e-30, 0.5])
    a2, b2 = a.flip(0).contiguous(), b.roll(1, 0).contiguous()
    got = _run([], [(a, b), (a2, b2)])
    want = R.table([], [(a, b), (a2, b2)])
    assert (want[:, 2:] == np.rint(want[:, 2:])).all() and (want[:, 2:] > 0).all()
    for col, name in ((2, "sse8_1"), (3, "sse8_2")):
        _same("sse8", name, got[:, col], torch.from_numpy(want[:, col]))
    for s, (p, q) in enumerate(((a, b), (a2, b2))):
        for i in range(B):
            _bar("sse8", f"sse{s + 1}_image{i}", G.sum_sq_diff_ref(p[i:i + 1], q[i:i + 1]), got[i, s:s + 1])


# ------------------------------------------------------------------------------------------------- the same bits in every batch
def _order_sensitive_job(B=3):
    liks = [_liks(B, 1027), _liks(B, 4100, salt=5000), _liks(B, 70000, salt=30000)]       # unaligned slices; two blocks; several trips
    pairs = [(_images(f"inv.a{s}", (B, 3, 50, 100)), _images(f"inv.b{s}", (B, 3, 50, 100))) for s in range(2)]
    return liks, pairs


def test_a_row_does_not_depend_on_the_batch_or_the_position_and_repeats():
    liks, pairs = _order_sensitive_job()
    whole = _run(liks, pairs)
    _same("invariance", "second_call", _run(liks, pairs), whole)
    for b in range(3):
        alone = _run([l[b:b + 1].clone() for l in liks], [tuple(t[b:b + 1].clone() for t in p) for p in pairs])
        _same("invariance", f"image{b}_alone", alone[0], whole[b])
    rev = _run([l.flip(0).contiguous() for l in liks], [tuple(t.flip(0).contiguous() for t in p) for p in pairs])
    _same("invariance", "reversed_batch", rev.flip(0), whole)
    want = R.table(liks, pairs)
    for b in range(3):
        for i, l in enumerate(liks):
            _bar("invariance", f"bits{i}_image{b}", G.sum_log2_ref(l[b]), whole[b, i:i + 1])
        for s, (p, q) in enumerate(pairs):
            _bar("invariance", f"sse{s + 1}_image{b}", G.sum_sq_diff_ref(p[b:b + 1], q[b:b + 1]), whole[b, 3 + s:4 + s])
    assert np.array_equal(whole[:, 5:].numpy(), want[:, 5:])


def test_a_nan_stays_in_its_row_and_its_pair():
    liks, pairs = _order_sensitive_job()
    clean = _run(liks, pairs)
    bad = pairs[0][0].clone()
    bad[1, 2, 17, 33] = float("nan")
    got = _run(liks, [(bad, pairs[0][1]), pairs[1]])
    n = len(liks)
    assert math.isnan(got[1, n]) and math.isnan(got[1, n + 2])
    keep = torch.ones_like(got, dtype=torch.bool)
    keep[1, n] = keep[1, n + 2] = False
    _same("nan", "every_other_cell", got[keep], clean[keep])
    assert bool(torch.isfinite(clean).all())


# ------------------------------------------------------------------------------------------------------------- limits, old kernel
def test_eight_likelihood_maps_and_none():
    B = 2
    sizes = [1027, 3, 1, 700, 64, 2044, 513, 8200]
    liks = [_liks(B, n, salt=9000 * i) for i, n in enumerate(sizes)]
    pairs = [(G.grid16(f"pm.lim.a{s}", (B, 3, 50, 100)), G.grid16(f"pm.lim.b{s}", (B, 3, 50, 100))) for s in range(2)]
    got = _run(liks, pairs)
    want = R.table(liks, pairs)
    for i, l in enumerate(liks):
        for b in range(B):
            _bar("n_lik8", f"bits{i}_image{b}", G.sum_log2_ref(l[b]), got[b, i:i + 1])
    _same("n_lik8", "sse", got[:, 8:], torch.from_numpy(want[:, 8:]))
    none = _run([], pairs)
    assert none.shape == (B, 4)
    _same("n_lik0", "sse", none, torch.from_numpy(want[:, 8:]))


def test_column_sums_describe_what_rd_sums_describes():
    """Summed over the batch, every column is the quantity ``Fn.rd_sums`` (the existing batch-level kernel) adds up on the same tensors: they
    agree within the sum of both results' units."""
    Fn, L = _imp()
    B = 3
    liks = [_liks(B, 1027), _liks(B, 70000, salt=30000)]
    pairs = [(_images(f"rd.a{s}", (B, 3, 50, 100)), _images(f"rd.b{s}", (B, 3, 50, 100))) for s in range(2)]
    ld = [_g(l, f"lik{i}") for i, l in enumerate(liks)]
    pd = [tuple(_g(t, f"img{s}") for t in p) for s, p in enumerate(pairs)]
    got = _run(ld, pd)
    z = lambda: torch.zeros(1, dtype=torch.float64, device=DEV)
    lo, so = [z() for _ in liks], [z() for _ in pairs]
    Fn.rd_sums(ld, lo, pd, so)
    torch.cuda.synchronize()
    for i, l in enumerate(liks):
        unit = sum(float(G.sum_log2_ref(l[b])["unit"]) for b in range(B)) + float(G.sum_log2_ref(l.reshape(-1))["unit"])
        err = abs(float(got[:, i].sum()) - float(lo[i]))
        print(f"pair_metrics rd_sums bits{i} {err / unit:.4f}")
        assert err <= unit
    for s, (p, q) in enumerate(pairs):
        unit = sum(float(G.sum_sq_diff_ref(p[b:b + 1], q[b:b + 1])["unit"]) for b in range(B)) + float(G.sum_sq_diff_ref(p, q)["unit"])
        err = abs(float(got[:, 2 + s].sum()) - float(so[s]))
        print(f"pair_metrics rd_sums sse{s + 1} {err / unit:.4f}")
        assert err <= unit


def test_the_call_replays_from_a_graph_with_the_same_bits():
    Fn, L = _imp()
    liks, pairs = _order_sensitive_job()
    ld = [l.to(DEV) for l in liks]
    pd = [tuple(t.to(DEV) for t in p) for p in pairs]
    eager = Fn.pair_metrics(ld, pd).clone()
    torch.cuda.synchronize()
    out = torch.full_like(eager, float("nan"))
    st = torch.cuda.Stream()
    st.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(st):
        Fn.pair_metrics(ld, pd, out=out)                     # warm-up on the capture stream
    torch.cuda.current_stream().wait_stream(st)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=st):
        Fn.pair_metrics(ld, pd, out=out)
    out.fill_(float("nan"))
    graph.replay()
    torch.cuda.synchronize()
    _same("graph", "replay", out, eager)


# -------------------------------------------------------------------------------------------------------------- model and folder
def _hsic(dtype=F16):
    from hesic_amd import codec
    return codec.load_model(None, dtype)


def _close(got, want, name, rel=1e-12):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape and np.all(np.abs(got - want) <= rel * np.abs(want)), (name, got, want)


def test_model_pair_metrics_on_a_padded_forward():
    """HSIC f16, B = 2 at 3 x 64 x 128 whose originals are 50 x 100: ``models.pair_metrics`` on the forward's own outputs against the restatement
    applied to the outputs read back -- the glue units on the sums, 1e-12 relative on the derived figures (a handful of fp64 roundings)."""
    from hesic_amd import models
    net = _hsic(F16)
    x1, x2, Hm = (t.to(DEV) for t in synthetic.stereo_batch(40, 2, 50, 100))
    x1p, x2p = models.pad_to_multiple(x1), models.pad_to_multiple(x2)
    assert tuple(x1p.shape) == (2, 3, 64, 128)
    with torch.no_grad():
        out = net(x1p, x2p, Hm)
        pm = models.pair_metrics(out, x1, x2)
        fig = models.pair_metrics_from(pm)
    torch.cuda.synchronize()
    keys = list(out["likelihoods"])
    assert len(keys) == 4
    assert pm["num_pixels"] == 50 * 100 and set(pm) == {"bits_" + k for k in keys} | {"sse1", "sse2", "sse8_1", "sse8_2", "num_pixels"}
    liks = [out["likelihoods"][k].float().cpu() for k in keys]
    hats = [out[k][..., :50, :100].cpu() for k in ("x1_hat", "x2_hat")]
    xs = [x1.cpu(), x2.cpu()]
    want = R.table(liks, [(hats[0], xs[0]), (hats[1], xs[1])])
    for b in range(2):
        for i, k in enumerate(keys):
            ref = G.sum_log2_ref(liks[i][b])
            _bar("model", f"bits_{k}_image{b}", {"ref": -ref["ref"], "unit": ref["unit"]}, pm["bits_" + k][b:b + 1])
        for s in range(2):
            _bar("model", f"sse{s + 1}_image{b}", G.sum_sq_diff_ref(hats[s][b:b + 1].float(), xs[s][b:b + 1]), pm[f"sse{s + 1}"][b:b + 1])
    assert np.array_equal(torch.stack([pm["sse8_1"], pm["sse8_2"]], 1).cpu().numpy(), want[:, 6:])
    tab = torch.stack([-pm["bits_" + k] for k in keys] + [pm["sse1"], pm["sse2"], pm["sse8_1"], pm["sse8_2"]], 1).cpu().numpy()
    rf = R.figures(tab, keys, 50, 100)
    for k, v in rf.items():
        if k == "bits":
            for kk in keys:
                _close(fig["bits"][kk].cpu().numpy(), v[kk], kk)
        else:
            assert fig[k].dtype == torch.float64 and tuple(fig[k].shape) == (2,)
            _close(fig[k].cpu().numpy(), v, k)
    assert bool((fig["psnr8"] > 5).all()) and bool((fig["bpp"] > 0).all())


def _write_folder(root):
    """test/: big0, big1 (170 x 200; big1 without a sidecar) and small (64 x 70)."""
    from PIL import Image
    from hesic_amd import codec
    pairs = {}
    for stems, seed, (h, w) in ((("big0", "big1"), 60, (170, 200)), (("small",), 70, (64, 70))):
        x1, x2, Hm = synthetic.stereo_batch(seed, len(stems), h, w)
        q1, q2 = codec.quantise(x1), codec.quantise(x2)
        for i, stem in enumerate(stems):
            for side, q in (("left", q1), ("right", q2)):
                d = root / "test" / side
                d.mkdir(parents=True, exist_ok=True)
                Image.fromarray(q[i]).save(d / f"{stem}.png")
            if stem != "big1":
                (root / "test" / "H").mkdir(exist_ok=True)
                np.save(root / "test" / "H" / f"{stem}.npy", Hm[i].double().numpy())
            pairs[stem] = (q1[i], q2[i], Hm[i].double().numpy())
    return pairs


def _recompute(net, pair, coded=True, enhancer=None):
    """One pair's figures by the public calls, alone (B = 1): rows are the same bits in any batch."""
    from hesic_amd import models
    q1, q2, H = pair
    x1 = torch.from_numpy(q1).permute(2, 0, 1).float().div(255.0)[None]
    x2 = torch.from_numpy(q2).permute(2, 0, 1).float().div(255.0)[None]
    h, w = x1.shape[-2:]
    x1p, x2p = models.pad_to_multiple(x1).to(DEV), models.pad_to_multiple(x2).to(DEV)
    x1, x2 = x1p[..., :h, :w], x2p[..., :h, :w]
    Hm = torch.from_numpy(H.astype(np.float64).reshape(1, 3, 3)).float().to(DEV)
    with torch.no_grad():
        out = net(x1p, x2p, Hm)
        if enhancer is not None:
            en = enhancer(out["x1_hat"], out["x2_hat"], Hm)
            out = {"x1_hat": en["x1_hat"], "x2_hat": en["x2_hat"], "likelihoods": out["likelihoods"]}
        fig = models.pair_metrics_from(models.pair_metrics(out, x1, x2))
        rec = {k: float(v) for k, v in fig.items() if k != "bits"}
        rec["bits"] = {k: float(v) for k, v in fig["bits"].items()}
        if min(h, w) > 160:
            s1, s2 = models.ms_ssim(out["x1_hat"][..., :h, :w], x1), models.ms_ssim(out["x2_hat"][..., :h, :w], x2)
            s = (s1 + s2) / 2
            rec.update(ms_ssim1=float(s1), ms_ssim2=float(s2), ms_ssim=float(s), ms_ssim_db=float(models.ms_ssim_db(s)))
        else:
            rec.update(ms_ssim1=None, ms_ssim2=None, ms_ssim=None, ms_ssim_db=None)
        if coded:
            enc = net.compress_batch(x1p, x2p, Hm, channels_per_stream=1)
            Hp, Wp = x1p.shape[-2:]
            rec["coded_bpp"] = enc["bpp_real"][0] * (Hp * Wp) / (h * w)          # bpp_real counts the padded pixels
            assert abs(rec["coded_bpp"] - len(enc["blobs"][0]) * 8 / (2 * h * w)) <= 1e-12 * rec["coded_bpp"]
    return rec


def _assert_record(rec, want, stem):
    for k, v in want.items():
        if k == "bits":
            assert rec["bits"] == v, (stem, rec["bits"], v)
        elif k == "coded_bpp":
            assert abs(rec[k] - v) <= 1e-12 * v, (stem, k)
        else:
            assert rec[k] == v or (isinstance(v, float) and math.isnan(v) and math.isnan(rec[k])), (stem, k, rec[k], v)


def test_eval_folder_records_and_summary(tmp_path):
    from hesic_amd import eval_folder
    pairs = _write_folder(tmp_path)
    lines = []
    out_file = tmp_path / "summary.json"
    records = eval_folder.main([str(tmp_path), "--batch", "2", "--coded", "--out", str(out_file)], log=lines.append)
    assert [r["stem"] for r in records] == ["big0", "small"] and len(lines) == 3
    assert [json.loads(l) for l in lines[:2]] == json.loads(json.dumps(records))
    summary = json.loads(lines[2])
    assert summary["pairs"] == 2 and summary["skipped_no_sidecar"] == 1 and summary["seconds"] > 0 and summary["pairs_per_s"] > 0
    assert json.loads(out_file.read_text()) == summary
    big, small = records
    assert (big["height"], big["width"], small["height"], small["width"]) == (170, 200, 64, 70)
    assert all(0 < big[k] <= 1 for k in ("ms_ssim1", "ms_ssim2", "ms_ssim")) and big["ms_ssim_db"] > 0
    assert all(small[k] is None for k in eval_folder.MS_SSIM_FIELDS)
    net = _hsic(F16)
    for rec in records:
        _assert_record(rec, _recompute(net, pairs[rec["stem"]]), rec["stem"])
    want = json.loads(json.dumps(eval_folder.summarise(records)))
    assert {k: summary[k] for k in want} == want
    assert summary["psnr"] == (big["psnr"] + small["psnr"]) / 2 and summary["ms_ssim"] == big["ms_ssim"]


def test_eval_folder_with_the_net_homography_skips_nobody(tmp_path):
    from hesic_amd import eval_folder
    _write_folder(tmp_path)
    lines = []
    with_net = eval_folder.main([str(tmp_path), "--batch", "2", "--homography", "net"], log=lines.append)      # big0 / big1 share one batch
    assert [r["stem"] for r in with_net] == ["big0", "big1", "small"] and json.loads(lines[-1])["skipped_no_sidecar"] == 0
    assert json.loads(lines[-1])["pairs"] == 3 and all(math.isfinite(r["psnr"]) and r["bpp"] > 0 for r in with_net)
    assert all("coded_bpp" not in r for r in with_net) and "coded_bpp" not in json.loads(lines[-1])


def test_eval_folder_enhancer_changes_the_distortion_and_leaves_the_bits(tmp_path):
    from hesic_amd import eval_folder
    pairs = _write_folder(tmp_path)
    enhanced = eval_folder.main([str(tmp_path), "--batch", "2", "--enhancer", "synthetic"], log=lambda s: None)
    assert [r["stem"] for r in enhanced] == ["big0", "small"]
    net, en = _hsic(F16), eval_folder.load_enhancer("synthetic")
    for e in enhanced:
        r = _recompute(net, pairs[e["stem"]], coded=False)               # the first model alone
        assert e["bits"] == r["bits"] and e["bpp"] == r["bpp"]
        assert e["mse1"] != r["mse1"] and e["mse2"] != r["mse2"] and e["psnr"] != r["psnr"] and e["psnr8"] != r["psnr8"]
        _assert_record(e, _recompute(net, pairs[e["stem"]], coded=False, enhancer=en), e["stem"])

"""The photometric homography refiner on the GPU (include/hesic_homography_refine.h, csrc/homography_refine.hip; homography.refine_h_matrix,
``codec encode --refine-homography``) against the numpy fp64 restatement of tests/homography_refine_ref.py.

Bars.  One pass: each of the 46 sums within (n + 16) 2^-52 S_abs of the restatement's (n pixels, S_abs the restatement's sum of the absolute
per-pixel terms: the fp64 summation bound plus a few roundings per term), the valid count exact.  Pyramid: bit-equal.  Known warps: <= 0.25 px
at the corners against the truth, <= 1e-4 px against the restatement's corners.  Huber (delta 0.05): <= 0.1 px and strictly better than L2.
Every case prints its figures before it asserts."""
import json

import numpy as np
import pytest
import torch

import homography_refine_ref as R
import memguard
from hesic_amd import functional as Fn
from hesic_amd import geometry, homography

pytestmark = pytest.mark.gpu

H, W = 96, 128
_CACHE = {}


def _known():
    """The six known-warp cases (seeds 0 - 5) with the restatement's answer from the identity, computed once and shared."""
    if "known" not in _CACHE:
        cases = [R.known_case(seed, H, W, sigma=2.0, rho=8.0) for seed in range(6)]
        eye = np.eye(3, dtype=np.float32)
        _CACHE["known"] = (cases, [R.refine(x1, x2, eye, levels=3, iters=10) for x1, x2, _ in cases])
    return _CACHE["known"]


def _batch(cases):
    x1 = torch.from_numpy(np.stack([c[0] for c in cases])).cuda()
    x2 = torch.from_numpy(np.stack([c[1] for c in cases])).cuda()
    return x1, x2


def _eye(B=1):
    return torch.eye(3, device="cuda").repeat(B, 1, 1)


def _guarded_crop(t, name):
    """``t`` (B,C,H,W) as a strided crop of a larger guarded tensor whose other elements are NaN.  Returns (crop, guarded tensor)."""
    B, C, h, w = t.shape
    big = torch.full((B, C, h + 5, w + 7), float("nan"), dtype=t.dtype, device=t.device)
    big[..., 2:2 + h, 3:3 + w] = t
    g = memguard.guarded(big, name=name)
    crop = g[..., 2:2 + h, 3:3 + w]
    assert not crop.is_contiguous()
    return crop, g


def _texture_batch(B, C, h, w, seed0):
    return np.stack([np.stack([R.texture(seed0 + 10 * b + c, h, w, 2.0) for c in range(C)]) for b in range(B)])


def _bits(t):
    return t.detach().cpu().numpy().tobytes()


def _info_bits(info):
    return b"".join(_bits(info[k]) for k in sorted(info))


# --------------------------------------------------------------------------------------------------------------------------- pyramid
@pytest.mark.parametrize("shape", [(1, 96, 128, 3), (3, 75, 101, 6), (3, 128, 192, 6), (1, 33, 47, 3)], ids=["c1_96x128", "c3_75x101", "c3_128x192_l6", "c1_33x47"])
def test_pyramid_is_bit_equal(shape):
    C, h, w, levels = shape
    B = 3
    a, b = _texture_batch(B, C, h, w, 40), _texture_batch(B, C, h, w, 70)
    x1, g1 = _guarded_crop(torch.from_numpy(a).cuda(), "x1")
    x2, g2 = _guarded_crop(torch.from_numpy(b).cuda(), "x2")
    pyr, views = Fn.homography_refine_pyramid(x1, x2, levels)
    sizes = R.level_sizes(h, w, levels)
    assert Fn.homography_refine_levels(h, w, levels) == len(sizes) == len(views) and pyr.numel() == sum(2 * B * hl * wl for hl, wl in sizes)
    for v, src in enumerate((a, b)):
        for i in range(B):
            for l, want in enumerate(R.pyramid(src[i], levels)):
                got = views[l][v, i].cpu().numpy()
                assert got.shape == want.shape and got.tobytes() == want.tobytes(), (v, i, l, np.abs(got - want).max())
    memguard.check_all([g1, g2])


# -------------------------------------------------------------------------------------------------------------------------- one pass
@pytest.mark.parametrize("shape", [(96, 128, 1), (75, 101, 3)], ids=["96x128", "75x101"])
def test_one_pass_sums(shape):
    h, w, C = shape
    B = 3
    a, b = _texture_batch(B, C, h, w, 11), _texture_batch(B, C, h, w, 12)
    b = (0.5 * a + 0.5 * b).astype(np.float32)                   # correlated with x1: residuals and gradients of comparable size
    x1, g1 = _guarded_crop(torch.from_numpy(a).cuda(), "x1")
    x2, g2 = _guarded_crop(torch.from_numpy(b).cuda(), "x2")
    generic = R.norm22(R.inv3(R.known_warp(7, h, w, 6.0)))
    mats = [np.eye(3), generic, R.norm22(R.inv3(R.known_warp(8, h, w, 3.0)))]
    pyr, views = Fn.homography_refine_pyramid(x1, x2, 3)
    worst = 0.0
    for level in (0, 1):
        for huber in (None, 0.05):
            A = [R.to_level(m, 0, level) for m in mats]
            part = Fn.homography_refine_normal_eq(pyr, (B, h, w), 3, level, torch.from_numpy(np.stack(A)).cuda(), huber)
            hl, wl = h >> level, w >> level
            assert part.shape == (B, min(64, -(-hl * wl // 256)), 46) and part.dtype == torch.float64
            part = part.cpu().numpy()
            for i in range(B):
                got = np.zeros(46)
                for j in range(part.shape[1]):                    # the update launch's order: blocks in index order
                    got = got + part[i, j]
                want, sabs = R.normal_equations(R.pyramid(a[i], 3)[level], R.pyramid(b[i], 3)[level], A[i], huber, with_abs=True)
                n = hl * wl
                bar = (n + 16) * 2.0 ** -52 * sabs
                ratio = float((np.abs(got - want)[:45] / np.maximum(bar[:45], 1e-300)).max())
                worst = max(worst, ratio)
                print(f"one_pass {h}x{w} level {level} huber {huber} pair {i}: n_valid {got[45]:.0f} (ref {want[45]:.0f}), worst |diff| / bar {ratio:.3e}")
                assert got[45] == want[45] and want[45] > 0.5 * n
                assert (np.abs(got - want)[:45] <= bar[:45]).all(), (level, huber, i, np.abs(got - want) / np.maximum(bar, 1e-300))
    print(f"one_pass {h}x{w}: worst |diff| / bar {worst:.3e}")
    memguard.check_all([g1, g2])


# ----------------------------------------------------------------------------------------------------------------------- known warps
def test_known_warps():
    cases, refs = _known()
    x1, x2 = _batch(cases)
    h, info = homography.refine_h_matrix(x1, x2, _eye(), levels=3, iters=10)
    assert h.shape == (6, 3, 3) and h.dtype == torch.float32
    assert info["cost_before"].dtype == torch.float64 and info["accepted"].dtype == torch.int32 and all(v.is_cuda and v.shape == (6,) for v in info.values())
    hc = h.cpu().numpy()
    rec = {k: v.cpu().numpy() for k, v in info.items()}
    for i, ((_, _, Ht), (hr, ir)) in enumerate(zip(cases, refs)):
        err, to_ref = R.corner_error(hc[i], Ht, H, W), R.corner_error(hc[i], hr, H, W)
        print(f"known seed {i}: corner error {err:.6f} px (ref {R.corner_error(hr, Ht, H, W):.6f}), to ref {to_ref:.3e} px, cost {rec['cost_before'][i]:.4e} -> "
              f"{rec['cost_after'][i]:.4e} (ref {ir['cost_before']:.4e} -> {ir['cost_after']:.4e}), accepted {rec['accepted'][i]}/{ir['accepted']}, "
              f"rejected {rec['rejected'][i]}/{ir['rejected']}, valid {rec['valid_share'][i]:.4f}")
    for i, ((_, _, Ht), (hr, ir)) in enumerate(zip(cases, refs)):
        assert R.corner_error(hc[i], Ht, H, W) <= 0.25, i
        assert R.corner_error(hc[i], hr, H, W) <= 1e-4, i
        assert rec["cost_after"][i] <= rec["cost_before"][i] and rec["levels_used"][i] == 3
        assert abs(rec["cost_before"][i] - ir["cost_before"]) <= 1e-12 * ir["cost_before"]
        assert rec["accepted"][i] > 0 and 0.5 < rec["valid_share"][i] <= 1.0


def test_huber():
    cases = [R.huber_case(seed, H, W) for seed in range(6)]
    x1, x2 = _batch(cases)
    hh, _ = homography.refine_h_matrix(x1, x2, _eye(), huber=0.05)
    hl, _ = homography.refine_h_matrix(x1, x2, _eye())
    hh, hl = hh.cpu().numpy(), hl.cpu().numpy()
    errs = [(R.corner_error(hh[i], c[2], H, W), R.corner_error(hl[i], c[2], H, W)) for i, c in enumerate(cases)]
    for i, (eh, el) in enumerate(errs):
        print(f"huber seed {i}: huber {eh:.4f} px, L2 {el:.4f} px")
    for eh, el in errs:
        assert eh <= 0.1 and eh < el


# ------------------------------------------------------------------------------------------------------------------------ never worse
@pytest.mark.parametrize("case", ["zero_overlap", "x2_zeros", "x2_constant", "iters0", "singular"])
def test_never_worse(case):
    """Each case returns the input bits, has finite info and reports accepted == 0.  ``x2_zeros`` / ``x2_constant``: a view without contrast
    says nothing about geometry (descent would only drag x1's window towards the parts of x1 nearest that constant), so such a level does
    nothing, like a level without a valid pixel; the start of these two cases overlaps well, so the overlap test is not what stops them."""
    cases, _ = _known()
    x1, x2 = _batch(cases[:2])
    h0 = torch.tensor([[1.01, 0.002, 1.5], [-0.003, 0.99, -2.25], [1e-5, -2e-5, 1.0]], device="cuda").repeat(2, 1, 1)      # a plain, well-overlapping start
    kw = {}
    if case == "zero_overlap":
        h0 = torch.tensor([[1, 0, 2.0 * W], [0, 1, 0], [0, 0, 1]], device="cuda").repeat(2, 1, 1)
    elif case == "x2_zeros":
        x2 = torch.zeros_like(x2)
    elif case == "x2_constant":
        x2 = torch.full_like(x2, 0.4375)
    elif case == "iters0":
        kw["iters"] = 0
    else:
        h0 = torch.tensor([[1, 2, 3], [2, 4, 6], [0, 0, 1.0]], device="cuda").repeat(2, 1, 1)
    h, info = homography.refine_h_matrix(x1, x2, h0, **kw)
    rec = {k: v.cpu().numpy() for k, v in info.items()}
    print(f"never_worse {case}: " + ", ".join(f"{k} {v.tolist()}" for k, v in rec.items()))
    assert all(np.isfinite(v).all() for v in rec.values())
    assert (rec["cost_after"] <= rec["cost_before"]).all()
    assert _bits(h) == _bits(h0)
    assert (rec["accepted"] == 0).all()
    if case.startswith("x2_"):
        assert (rec["rejected"] == 0).all() and (rec["cost_before"] > 0).all() and (rec["cost_after"] == rec["cost_before"]).all()


# ------------------------------------------------------------------------------------------------------------------------ determinism
def test_two_calls_and_a_graph_replay_are_bit_identical():
    cases, _ = _known()
    x1, x2 = _batch(cases)
    h0 = _eye(6)
    ha, ia = homography.refine_h_matrix(x1, x2, h0, huber=0.1)
    hb, ib = homography.refine_h_matrix(x1, x2, h0, huber=0.1)
    assert _bits(ha) == _bits(hb) and _info_bits(ia) == _info_bits(ib)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        homography.refine_h_matrix(x1, x2, h0, huber=0.1)         # warm on a side stream, as captures want
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        hg, ig = homography.refine_h_matrix(x1, x2, h0, huber=0.1)
    hg.fill_(float("nan"))
    graph.replay()
    torch.cuda.synchronize()
    assert _bits(hg) == _bits(ha) and _info_bits(ig) == _info_bits(ia)


def test_a_pair_gives_the_same_bits_alone_and_at_any_position():
    cases, _ = _known()
    x1, x2 = _batch(cases)
    full, info = homography.refine_h_matrix(x1, x2, _eye())
    for i in (0, 5):
        alone, ia = homography.refine_h_matrix(x1[i:i + 1], x2[i:i + 1], _eye())
        assert _bits(alone[0]) == _bits(full[i]) and all(_bits(ia[k][0]) == _bits(info[k][i]) for k in info), i
    for k in range(1, 6):                                         # seed 0's pair at every other position of the batch
        rolled, ir = homography.refine_h_matrix(torch.roll(x1, k, 0), torch.roll(x2, k, 0), _eye())
        assert _bits(rolled) == _bits(torch.roll(full, k, 0)), k
        assert _bits(ir["cost_after"]) == _bits(torch.roll(info["cost_after"], k, 0)), k


# ------------------------------------------------------------------------------------------------------------------------ allocations
def test_poisoned_allocations():
    cases, _ = _known()
    a = np.stack([np.repeat(c[0], 3, 0) for c in cases[:3]])
    b = np.stack([np.repeat(c[1], 3, 0) for c in cases[:3]])
    x1, g1 = _guarded_crop(torch.from_numpy(a).cuda(), "x1")
    x2, g2 = _guarded_crop(torch.from_numpy(b).cuda(), "x2")
    want, winfo = Fn.homography_refine(x1, x2, _eye(3).contiguous())
    with memguard.poisoned_allocations([Fn]) as rec:
        got, info = Fn.homography_refine(x1, x2, _eye(3).contiguous())
        assert len(rec) == 3                                      # the workspace, the matrices, the report
    assert torch.isfinite(got).all() and torch.isfinite(info).all()
    assert _bits(got) == _bits(want) and _bits(info) == _bits(winfo)
    assert (info[:, 6] == 1).all() and (info[:, 2] > 0).all()
    memguard.check_all([g1, g2])
    # three equal channels are the grey image itself ((v + v + v) / 3 is v exactly in fp64): the one-channel batch's bits
    one, _ = Fn.homography_refine(torch.from_numpy(np.stack([c[0] for c in cases[:3]])).cuda(),
                                  torch.from_numpy(np.stack([c[1] for c in cases[:3]])).cuda(), _eye(3).contiguous())
    assert _bits(one) == _bits(got)


# -------------------------------------------------------------------------------------------------------------------------------- CLI
def test_cli_encode_with_refinement(tmp_path, capsys):
    """Two 128 x 192 PNG pairs cut from the textures, sidecars 3 px off at the corners: ``encode --refine-homography`` writes the matrices
    ``refine_h_matrix`` returns for the same inputs, with a lower photometric figure; ``decode`` writes both views; without the flag the JSON
    is today's."""
    from PIL import Image
    from hesic_amd import codec
    from hesic_amd.models import pad_to_multiple
    h, w = 128, 192
    root = tmp_path / "data"
    for sub in ("left", "right", "H"):
        (root / "test" / sub).mkdir(parents=True)
    off = np.array([[3, -3], [-3, 3], [3, 3], [-3, -3]], np.float64)
    truth, side = {}, {}
    for i, stem in enumerate(("a", "b")):
        x1, x2, Ht = R.known_case(20 + i, h, w, sigma=2.0, rho=4.0)
        for name, x in (("left", x1), ("right", x2)):
            Image.fromarray(np.repeat((x[0] * 255).round().astype(np.uint8)[..., None], 3, -1)).save(root / "test" / name / (stem + ".png"))
        c = R.corners_of(h, w)
        truth[stem], side[stem] = Ht, R.dlt4(c, R.corner_points(Ht, h, w) + off)
        np.save(root / "test" / "H" / (stem + ".npy"), side[stem])
    plain, refined, recon = tmp_path / "plain", tmp_path / "refined", tmp_path / "recon"
    assert codec.main(["encode", str(root), str(plain), "--batch", "2"]) == 0
    assert codec.main(["encode", str(root), str(refined), "--batch", "2", "--refine-homography", "--refine-huber", "0.1"]) == 0
    capsys.readouterr()
    x1 = pad_to_multiple(torch.stack([codec.read_image(root / "test" / "left" / f"{s}.png") for s in ("a", "b")])).cuda()
    x2 = pad_to_multiple(torch.stack([codec.read_image(root / "test" / "right" / f"{s}.png") for s in ("a", "b")])).cuda()
    Hm = torch.from_numpy(np.stack([side["a"], side["b"]])).float().cuda()
    want, info = homography.refine_h_matrix(x1[..., :h, :w], x2[..., :h, :w], Hm, levels=3, iters=10, huber=0.1)
    for i, stem in enumerate(("a", "b")):
        p, r = json.loads((plain / f"{stem}.json").read_text()), json.loads((refined / f"{stem}.json").read_text())
        assert set(p) == {"height", "width", "h_matrix"} and p["h_matrix"] == side[stem].reshape(-1).tolist()
        assert set(r) == {"height", "width", "h_matrix", "h_refined", "photometric_before", "photometric_after"} and r["h_refined"] is True
        assert np.asarray(r["h_matrix"], np.float64).astype(np.float32).tobytes() == _bits(want[i])
        assert r["photometric_before"] == float(info["cost_before"][i]) and r["photometric_after"] == float(info["cost_after"][i])
        e0, e1 = R.corner_error(side[stem], truth[stem], h, w), R.corner_error(np.asarray(r["h_matrix"]).reshape(3, 3), truth[stem], h, w)
        print(f"cli {stem}: corner error {e0:.3f} -> {e1:.4f} px, photometric {r['photometric_before']:.4e} -> {r['photometric_after']:.4e}")
        assert r["photometric_after"] < r["photometric_before"] and e1 < 0.5 < e0
    assert codec.main(["decode", str(refined), str(recon), "--batch", "2"]) == 0
    assert sorted(f.name for f in recon.glob("*.png")) == ["a_left.png", "a_right.png", "b_left.png", "b_right.png"]
    assert np.array(Image.open(recon / "a_right.png")).shape == (h, w, 3)


# -------------------------------------------------------------------------------------------------------------------------- refusals
def test_refusals():
    x = torch.zeros(2, 3, 32, 48, device="cuda")
    with pytest.raises(NotImplementedError, match="align_corners"):
        homography.refine_h_matrix(x, x, _eye(), align_corners=False)
    with pytest.MonkeyPatch.context() as mp:
        mp.setattr(geometry, "DEFAULT_ALIGN_CORNERS", False)
        with pytest.raises(NotImplementedError, match="align_corners"):
            homography.refine_h_matrix(x, x, _eye())
        homography.refine_h_matrix(x, x, _eye(), align_corners=True)
    with pytest.raises(TypeError, match="float32"):
        homography.refine_h_matrix(x.half(), x.half(), _eye())
    with pytest.raises(TypeError, match="float32"):
        homography.refine_h_matrix(x, x, _eye().double())
    with pytest.raises(RuntimeError, match="one shape"):
        homography.refine_h_matrix(x, x[..., :40], _eye())
    with pytest.raises(RuntimeError, match="one shape"):
        homography.refine_h_matrix(x[:, :2], x[:, :2], _eye())
    with pytest.raises(RuntimeError, match=r"\(B, 3, 3\)"):
        homography.refine_h_matrix(x, x, _eye(3))
    with pytest.raises(RuntimeError, match="at least 16"):
        homography.refine_h_matrix(x[..., :15, :], x[..., :15, :], _eye())
    with pytest.raises(ValueError, match="levels"):
        homography.refine_h_matrix(x, x, _eye(), levels=0)
    with pytest.raises(ValueError, match="huber"):
        homography.refine_h_matrix(x, x, _eye(), huber=0.0)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        homography.refine_h_matrix(x.cpu(), x.cpu(), torch.eye(3)[None])
    h, info = homography.refine_h_matrix(x, x, _eye(), levels=6)           # 32 x 48: two levels exist
    assert (info["levels_used"] == 2).all() and _bits(h) == _bits(_eye(2))

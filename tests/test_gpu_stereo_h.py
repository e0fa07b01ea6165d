"""The stereo homography estimator (hesic_amd.stereo_h) on the GPU: every stage against the NumPy restatement (tests/stereo_h_ref.py),
the result against the ground-truth H of synthetic pairs, determinism, batch independence, degenerate inputs, memory bounds, the loader
callable, the sidecar writer and the codec end to end."""
import os
import random
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import stereo_h_ref as R                                      # noqa: E402
from hesic_amd import synthetic                               # noqa: E402

pytestmark = pytest.mark.gpu


def _est(x1, x2, **kw):
    from hesic_amd import stereo_h
    return stereo_h.estimate_homography(torch.as_tensor(x1).cuda(), torch.as_tensor(x2).cuda(), **kw)


def _pair(kind, seed, h=512, w=512):
    return getattr(synthetic, kind)(seed, h, w)


@pytest.fixture(scope="module")
def stage_case():
    x1, x2, Ht = _pair("stereo_pair", 1)
    ref = R.estimate(x1, x2, pair=0)
    H, valid, inl, det = _est(x1[None], x2[None], return_details=True)
    return x1, x2, Ht, ref, H, valid, inl, det


def test_integral_is_bit_exact(stage_case):
    _, _, _, ref, _, _, _, det = stage_case
    assert np.array_equal(det["integral"][0].cpu().numpy(), ref["I1"])
    assert np.array_equal(det["integral"][1].cpu().numpy(), ref["I2"])


def test_hessian_responses(stage_case):
    _, _, _, ref, _, _, _, det = stage_case
    for v in (0, 1):
        g = det["hessian"][v].cpu().numpy()
        r = np.concatenate([d.reshape(-1) for d in ref["dets%d" % (v + 1)]])
        assert g.shape == r.shape
        scale = np.maximum(np.abs(r), 1.0)
        assert float(np.max(np.abs(g - r) / scale)) <= 1e-5


def _found(g, r, tol=0.01):
    """Fraction of the rows of r (x, y, size) with a row of g within tol px in x, y and equal size."""
    if len(r) == 0:
        return 1.0
    d = np.abs(g[None, :, :2] - r[:, None, :2]).max(-1)
    ok = (d <= tol) & (g[None, :, 2] == r[:, None, 2])
    return float(ok.any(1).mean())


def test_keypoints_and_descriptors(stage_case):
    _, _, _, ref, _, _, _, det = stage_case
    for v in (0, 1):
        g = det["keypoints"][v].cpu().numpy()
        r = ref["kps%d" % (v + 1)]
        assert _found(g, r) >= 0.99, (len(g), len(r))
        if len(g) == len(r) and np.array_equal(g, r):
            gd = det["descriptors"][v].cpu().numpy()
            assert float(np.abs(gd - ref["desc%d" % (v + 1)]).max()) <= 1e-5
        else:                                                            # descriptors of the keypoints both found
            gd = det["descriptors"][v].cpu().numpy()
            for i in range(0, len(r), max(1, len(r) // 64)):
                j = np.where((np.abs(g[:, :2] - r[i, :2]).max(1) == 0) & (g[:, 2] == r[i, 2]))[0]
                if len(j):
                    assert float(np.abs(gd[j[0]] - ref["desc%d" % (v + 1)][i]).max()) <= 1e-5


def test_matches_and_result_follow_the_restatement(stage_case):
    x1, x2, Ht, ref, H, valid, inl, det = stage_case
    gm = {tuple(m) for m in det["matches"][0].cpu().numpy().tolist()}
    rm = {tuple(m) for m in ref["matches"].tolist()}
    assert len(gm & rm) >= 0.99 * max(len(gm), len(rm))
    assert bool(valid[0]) and ref["H"] is not None
    assert R.corner_error(H[0].cpu().numpy(), ref["H"], 512, 512) <= 0.05
    assert abs(int(inl[0]) - ref["inliers"]) <= 0.01 * ref["inliers"]


def test_keypoint_cap_follows_the_restatement():
    """max_keypoints below the candidate count: the radix-select path keeps the same strongest keypoints as the restatement, and the
    later stages follow."""
    x1, x2, _ = _pair("stereo_pair", 1)
    ref = R.estimate(x1, x2, max_keypoints=512, pair=0)
    assert len(R.detect(ref["I1"], ref["dets1"])) > 512 and len(R.detect(ref["I2"], ref["dets2"])) > 512
    H, valid, inl, det = _est(x1[None], x2[None], max_keypoints=512, return_details=True)
    for v in (0, 1):
        g = det["keypoints"][v].cpu().numpy()
        r = ref["kps%d" % (v + 1)]
        assert len(g) == len(r) == 512 and _found(g, r) >= 0.99
    gm = {tuple(m) for m in det["matches"][0].cpu().numpy().tolist()}
    rm = {tuple(m) for m in ref["matches"].tolist()}
    assert len(gm & rm) >= 0.99 * max(len(gm), len(rm))
    assert bool(valid[0]) and R.corner_error(H[0].cpu().numpy(), ref["H"], 512, 512) <= 0.05
    assert abs(int(inl[0]) - ref["inliers"]) <= 0.01 * ref["inliers"]


def test_pair_ids_key_the_sampling():
    """pair_ids gives each pair its own RANSAC draws: a pair estimated alone under its number equals the same pair inside a batch."""
    x1, x2, _ = synthetic.stereo_batch(0, 3, 256, 256)
    a = _est(x1, x2, pair_ids=[7, 3, 11], return_details=True)
    for j, i in enumerate((7, 3, 11)):
        s = _est(x1[j:j + 1], x2[j:j + 1], pair_ids=[i], return_details=True)
        assert torch.equal(s[0][0], a[0][j]) and int(s[3]["best"][0]) == int(a[3]["best"][j])


@pytest.mark.parametrize("seed", range(8))
def test_recovers_ground_truth(seed):
    x1, x2, Ht = _pair("stereo_pair", seed)
    H, valid, _ = _est(x1[None], x2[None], first_pair=seed)
    assert bool(valid[0])
    assert R.corner_error(H[0].cpu().numpy(), Ht, 512, 512) <= 0.5


@pytest.mark.parametrize("seed", range(8))
def test_smooth_pairs_follow_the_restatement(seed):
    """smooth_stereo_pair at 512^2 leaves 14-26 ratio-test matches at hessianThreshold 100 (see test_stereo_h_cpu.py): the 0.5 px bar
    does not apply there; the expected result is the restatement's."""
    x1, x2, Ht = _pair("smooth_stereo_pair", seed)
    ref = R.estimate(x1, x2, pair=seed)
    H, valid, _ = _est(x1[None], x2[None], first_pair=seed)
    assert bool(valid[0]) == (ref["H"] is not None)
    if ref["H"] is not None:
        assert R.corner_error(H[0].cpu().numpy(), ref["H"], 512, 512) <= 0.05


def test_large_pair_and_outliers():
    x1, x2, Ht = synthetic.stereo_pair(3, 860, 1080)
    H, valid, _ = _est(x1[None], x2[None])
    assert bool(valid[0]) and R.corner_error(H[0].cpu().numpy(), Ht, 860, 1080) <= 0.5
    xs1, xs2, hs = [], [], []
    for seed in range(8):
        a, b, Hm = _pair("stereo_pair", seed)
        b = b.copy()
        b[:, 200:328, 300:428] = np.random.default_rng(100 + seed).uniform(0, 1, (3, 128, 128)).astype(np.float32)
        xs1.append(a); xs2.append(b); hs.append(Hm)
    H, valid, _ = _est(np.stack(xs1), np.stack(xs2))
    for i in range(8):
        assert bool(valid[i]) and R.corner_error(H[i].cpu().numpy(), hs[i], 512, 512) <= 1.0


def test_deterministic_and_batch_independent():
    x1, x2, _ = synthetic.stereo_batch(0, 8, 256, 256)
    a = _est(x1, x2, return_details=True)
    b = _est(x1, x2, return_details=True)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and torch.equal(a[2], b[2])
    for k in ("keypoints", "descriptors", "matches", "inlier_mask"):
        assert all(torch.equal(u, v) for u, v in zip(a[3][k], b[3][k])), k
    for i in range(8):
        s = _est(x1[i:i + 1], x2[i:i + 1], first_pair=i)
        assert torch.equal(s[0][0], a[0][i]) and bool(s[1][0]) == bool(a[1][i]) and int(s[2][0]) == int(a[2][i])


def test_degenerate_inputs_are_invalid():
    c = torch.full((1, 3, 128, 128), 0.5)
    H, valid, _ = _est(c, c)
    assert not bool(valid[0]) and torch.equal(H.cpu(), torch.zeros(1, 3, 3))
    x1, x2, _ = synthetic.stereo_batch(0, 1, 32, 32)
    _, valid, _ = _est(x1, x2)
    assert not bool(valid[0])
    # a single blob: a handful of keypoints, fewer than 4 matches
    y, x = np.mgrid[0:128, 0:128]
    blob = (0.2 + 0.6 * np.exp(-((x - 64.0) ** 2 + (y - 64.0) ** 2) / 50.0)).astype(np.float32)
    img = torch.from_numpy(np.stack([blob] * 3))[None]
    _, valid, _, det = _est(img, img, return_details=True)
    assert len(det["matches"][0]) < 4 and not bool(valid[0])
    torch.cuda.synchronize()


def test_memory_bounds():
    """Every entry point of include/hesic_stereo_h.h, with guarded inputs and poisoned allocations: results equal a plain run, guards intact."""
    import memguard as MG
    from hesic_amd import stereo_h
    x1, x2, _ = synthetic.stereo_batch(0, 2, 200, 232)
    u1 = (x1 * 255).round().to(torch.uint8).cuda()
    u2 = (x2 * 255).round().to(torch.uint8).cuda()
    plain = stereo_h.estimate_homography(u1, u2, return_details=True, max_keypoints=512, hypotheses=300)
    for fill in (MG.NAN_FILL, MG.BIG_FILL):
        g1, g2 = MG.guarded(u1, fill=fill, name="img1"), MG.guarded(u2, fill=fill, name="img2")
        with MG.poisoned_allocations([stereo_h], fill=fill):
            got = stereo_h.estimate_homography(g1, g2, return_details=True, max_keypoints=512, hypotheses=300)
            torch.cuda.synchronize()
        g1.check()
        g2.check()
        assert torch.equal(got[0], plain[0]) and torch.equal(got[1], plain[1]) and torch.equal(got[2], plain[2])
        for k in ("keypoints", "descriptors", "matches", "inlier_mask"):
            assert all(torch.equal(u, v) for u, v in zip(got[3][k], plain[3][k])), k
        assert torch.equal(got[3]["integral"], plain[3]["integral"]) and torch.equal(got[3]["hessian"], plain[3]["hessian"])


def _folder(root, n=3, h=384, w=448):
    from PIL import Image
    hs = []
    for side in ("left", "right"):
        os.makedirs(os.path.join(root, "train", side), exist_ok=True)
    for i in range(n):
        a, b, Hm = synthetic.stereo_pair(i, h, w)
        Image.fromarray((a.transpose(1, 2, 0) * 255).round().astype(np.uint8)).save(os.path.join(root, "train", "left", f"{i:04d}.png"))
        Image.fromarray((b.transpose(1, 2, 0) * 255).round().astype(np.uint8)).save(os.path.join(root, "train", "right", f"{i:04d}.png"))
        hs.append(Hm)
    return hs


def _crop_H(Hfull, x0, y0):
    t_in = np.array([[1, 0, x0], [0, 1, y0], [0, 0, 1]], dtype=np.float64)
    t_out = np.array([[1, 0, -x0], [0, 1, -y0], [0, 0, 1]], dtype=np.float64)
    Hc = t_out @ np.asarray(Hfull, np.float64) @ t_in
    return Hc / Hc[2, 2]


def test_loader_callable_and_cli(tmp_path):
    from compressai.datasets import ImageFolder, to_tensor
    from hesic_amd import stereo_h
    root = str(tmp_path)
    hs = _folder(root)
    ds = ImageFolder(root, transform=to_tensor, patch_size=(256, 256), split="train", homography=stereo_h.HipHomography())
    offsets = []
    for i in range(len(ds)):
        random.seed(7 + i)
        item = ds[i]
        random.seed(7 + i)
        y0, x0 = random.randint(0, 384 - 256 - 1), random.randint(0, 448 - 256 - 1)
        offsets.append((x0, y0))
        assert len(item) == 6
        assert R.corner_error(item[2].numpy(), _crop_H(hs[i], x0, y0), 256, 256) <= 0.5
    assert stereo_h.main([root, "--split", "train", "--batch", "2"]) == 0
    for i in range(3):
        assert os.path.isfile(os.path.join(root, "train", "H", f"{i:04d}.npy"))
    ds2 = ImageFolder(root, transform=to_tensor, patch_size=(256, 256), split="train")
    for i in range(len(ds2)):
        random.seed(7 + i)
        item = ds2[i]
        x0, y0 = offsets[i]
        assert len(item) == 6
        assert R.corner_error(item[2].numpy(), _crop_H(hs[i], x0, y0), 256, 256) <= 0.5


def test_codec_bpp_with_estimated_h():
    """HSIC.forward (float16 maps, x3 analysis) on 4 stereo_pair 256^2 pairs: every pair is valid, its corners within 0.5 px, and the bpp
    with the estimated H within 1 % of the bpp with H_true.

    smooth_stereo_pair at 256^2 is not used: it leaves 0-4 matches per pair (two pairs invalid, the other two 307 px and 4993 px off).
    The 1 % bpp bar alone does NOT discriminate the quality of H with these synthetic weights.  Measured bpp on this batch: H_true
    6.02685, estimated 6.02526, H_true with its translation moved by +1 / +4 / +16 / +64 px 6.01678 / 6.00323 / 6.02278 / 5.99533,
    identity 5.62679.  Only a missing warp (identity, -6.6 %) leaves the bar; the corner-error assertion carries the accuracy check."""
    import hesic_amd
    from hesic_amd import models
    x1, x2, Ht = synthetic.stereo_batch(0, 4, 256, 256)
    H, valid, _ = _est(x1, x2)
    assert bool(valid.all())
    errs = [R.corner_error(H[i].cpu().numpy(), Ht[i].numpy(), 256, 256) for i in range(4)]
    assert max(errs) <= 0.5, errs
    hesic_amd.set_compute_dtype(torch.float16)
    try:
        net = models.HSIC()
        synthetic.fill_state_dict_(net.state_dict())
        net = net.cuda().eval()
        bpp = {}
        with torch.no_grad():
            for name, Hm in (("true", Ht), ("estimated", H.cpu()), ("identity", torch.eye(3).expand(4, 3, 3).contiguous())):
                out = net(x1.cuda(), x2.cuda(), Hm.cuda())
                bpp[name] = models.metrics_from(models.rate_distortion(out, x1.cuda(), x2.cuda()))["bpp"]
    finally:
        hesic_amd.set_compute_dtype(torch.float32)
    print(f"codec bpp: H_true {bpp['true']:.6f}, estimated H {bpp['estimated']:.6f}, identity {bpp['identity']:.6f}; corner errors "
          f"{[round(e, 3) for e in errs]} px")
    assert abs(bpp["estimated"] - bpp["true"]) <= 0.01 * bpp["true"], (bpp, errs)
    assert abs(bpp["identity"] - bpp["true"]) > 0.01 * bpp["true"], bpp          # the bar does see a missing warp

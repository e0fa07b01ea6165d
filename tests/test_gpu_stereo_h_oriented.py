"""Oriented and extended SURF of the stereo homography estimator on the GPU: orientations, descriptors, matches and H against the NumPy
restatement (tests/stereo_h_oriented_ref.py), the identity frame against the upright entry point, ground truth under in-plane rotation,
an exact 90-degree rotation, determinism, batch independence, memory bounds, the loader callable and the sidecar command."""
import os
import random
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import stereo_h_ref as R                                      # noqa: E402
import stereo_h_oriented_ref as O                             # noqa: E402
from hesic_amd import synthetic                               # noqa: E402

pytestmark = pytest.mark.gpu

THETAS = (0, 30, 60, 90, 135, 180, 270)
MODES = {"oriented64": (False, False), "upright128": (True, True), "oriented128": (False, True)}


def _est(x1, x2, **kw):
    from hesic_amd import stereo_h
    return stereo_h.estimate_homography(torch.as_tensor(x1).cuda(), torch.as_tensor(x2).cuda(), **kw)


@pytest.fixture(scope="module")
def cases():
    return {}


def _case(cases, mode):
    """One 512^2 pair, rotated by 30 degrees for the oriented modes (0 for upright): the restatement and the GPU with
    return_details, in the given descriptor mode."""
    if mode not in cases:
        up, ext = MODES[mode]
        x1, x2, Ht = synthetic.rotated_stereo_pair(1, 0 if up else 30, 512, 512)
        ref = O.estimate(x1, x2, upright=up, extended=ext)
        got = _est(x1[None], x2[None], upright=up, extended=ext, return_details=True)
        cases[mode] = (Ht, ref, got)
    return cases[mode]


def _common(g, r):
    """Index pairs (i in g, j in r) of keypoints with identical (x, y, size)."""
    key = {tuple(row): j for j, row in enumerate(r[:, :3].tolist())}
    gi, rj = [], []
    for i, row in enumerate(g[:, :3].tolist()):
        j = key.get(tuple(row))
        if j is not None:
            gi.append(i)
            rj.append(j)
    return np.array(gi, np.int64), np.array(rj, np.int64)


def test_orientations_are_exact(cases):
    """(cos, sin) equal the restatement's bit for bit on every keypoint both found (fp32 fastAtan2, correctly rounded / and sqrt)."""
    _, ref, got = _case(cases, "oriented64")
    det = got[3]
    assert len(det["orientations"]) == 2
    for v in (0, 1):
        g = det["keypoints"][v].cpu().numpy()
        r = ref["kps%d" % (v + 1)]
        gi, rj = _common(g, r)
        assert len(gi) >= 0.99 * len(r)
        go = det["orientations"][v].cpu().numpy()[gi]
        ro = ref["ori%d" % (v + 1)][rj]
        assert go.shape == ro.shape and np.array_equal(go, ro), int((go != ro).any(1).sum())
    print(f"orientation fallbacks of the restatement on this pair: {ref['fallbacks']}")


def test_identity_frame_equals_upright_describe():
    """describe_ex with (1, 0) for every keypoint and dim = 64 gives hesic_stereo_h_describe's bits; with ori = NULL too."""
    from hesic_amd import _lib as L
    x1, x2, _ = synthetic.rotated_stereo_pair(2, 45, 384, 448)
    det = _est(x1[None], x2[None], upright=False, return_details=True)[3]
    I = det["integral"]
    nk = [len(k) for k in det["keypoints"]]
    N, K = 2, max(nk)
    kp = torch.zeros((N, K, 4), dtype=torch.float32, device="cuda")
    for n in range(N):
        kp[n, :nk[n]] = det["keypoints"][n]
    n_kp = torch.tensor(nk, dtype=torch.int32, device="cuda")
    ori = torch.zeros((N, K, 2), dtype=torch.float32, device="cuda")
    ori[..., 0] = 1
    outs = []
    for name, o in (("plain", None), ("identity", ori), ("null", None)):
        desc = torch.zeros((N, K, 64), dtype=torch.float32, device="cuda")
        nrm = torch.zeros((N, K), dtype=torch.float32, device="cuda")
        if name == "plain":
            L.call("hesic_stereo_h_describe", L.ptr(I), L.ptr(kp), L.ptr(n_kp), N, 384, 448, K, L.ptr(desc), L.ptr(nrm), L.stream())
        else:
            L.call("hesic_stereo_h_describe_ex", L.ptr(I), L.ptr(kp), L.ptr(o), L.ptr(n_kp), N, 384, 448, K, 64, L.ptr(desc), L.ptr(nrm),
                   L.stream())
        outs.append((desc, nrm))
    for desc, nrm in outs[1:]:
        assert torch.equal(desc, outs[0][0]) and torch.equal(nrm, outs[0][1])


@pytest.mark.parametrize("mode", list(MODES))
def test_descriptors_follow_the_restatement(cases, mode):
    _, ref, got = _case(cases, mode)
    det = got[3]
    D = 128 if MODES[mode][1] else 64
    for v in (0, 1):
        g = det["keypoints"][v].cpu().numpy()
        r = ref["kps%d" % (v + 1)]
        gi, rj = _common(g, r)
        assert len(gi) >= 0.99 * len(r)
        gd = det["descriptors"][v].cpu().numpy()
        assert gd.shape[1] == D
        assert float(np.abs(gd[gi] - ref["desc%d" % (v + 1)][rj]).max()) <= 1e-5


@pytest.mark.parametrize("mode", list(MODES))
def test_matches_and_result_follow_the_restatement(cases, mode):
    _, ref, (H, valid, inl, det) = _case(cases, mode)
    gm = {tuple(m) for m in det["matches"][0].cpu().numpy().tolist()}
    rm = {tuple(m) for m in ref["matches"].tolist()}
    assert len(gm & rm) >= 0.99 * max(len(gm), len(rm))
    assert bool(valid[0]) and ref["H"] is not None
    assert R.corner_error(H[0].cpu().numpy(), ref["H"], 512, 512) <= 0.05
    assert abs(int(inl[0]) - ref["inliers"]) <= 0.01 * ref["inliers"]


def test_ground_truth_under_rotation():
    """Oriented SURF: every rotated pair valid, corners within 1 px.  Upright SURF: invalid or > 5 px off from 60 degrees on."""
    pairs = [synthetic.rotated_stereo_pair(0, t, 512, 512) for t in THETAS]
    x1 = np.stack([p[0] for p in pairs])
    x2 = np.stack([p[1] for p in pairs])
    ids = [0] * len(THETAS)                                     # each pair under the number the CPU test uses
    Ho, vo, _ = _est(x1, x2, pair_ids=ids, upright=False)
    Hu, vu, _ = _est(x1, x2, pair_ids=ids, upright=True)
    errs = []
    for k, (t, (_, _, Ht)) in enumerate(zip(THETAS, pairs)):
        assert bool(vo[k]), t
        e = R.corner_error(Ho[k].cpu().numpy(), Ht, 512, 512)
        errs.append(round(e, 3))
        assert e <= 1.0, (t, e)
        if t >= 60:
            assert not bool(vu[k]) or R.corner_error(Hu[k].cpu().numpy(), Ht, 512, 512) > 5.0, t
    print(f"oriented corner errors (px) at {THETAS} degrees: {errs}")


def test_exact_quarter_turn():
    """View 2 = torch.rot90 of view 1: a view-1 pixel (x, y) is (y, 511 - x) in view 2, and a direction turns by -90 degrees (x
    right, y down).  The restatement pairs 100 % of these keypoints with a turn within 10 degrees of -90 (seeds 0 and 1); the bar is 99 %."""
    x1 = torch.from_numpy(synthetic.rotated_stereo_pair(0, 0, 512, 512)[0])[None]
    x2 = torch.rot90(x1, 1, dims=(2, 3)).contiguous()
    det = _est(x1, x2, upright=False, return_details=True)[3]
    k1, k2 = (det["keypoints"][v].cpu().numpy() for v in (0, 1))
    o1, o2 = (det["orientations"][v].cpu().numpy() for v in (0, 1))
    p = np.stack([k1[:, 1], 511 - k1[:, 0]], -1)
    d = np.abs(p[:, None] - k2[None, :, :2]).max(-1)
    i, j = np.where((d <= 0.5) & (k1[:, None, 2] == k2[None, :, 2]))
    assert len(i) >= 0.9 * len(k1)
    turn = np.degrees(np.arctan2(o2[j, 1], o2[j, 0]) - np.arctan2(o1[i, 1], o1[i, 0]))
    dev = (turn + 90 + 180) % 360 - 180
    assert float((np.abs(dev) < 10).mean()) >= 0.99


def test_oriented_extended_is_deterministic_and_batch_independent():
    pairs = [synthetic.rotated_stereo_pair(s, t, 256, 256) for s, t in ((4, 30), (5, 90), (6, 180))]
    x1 = torch.from_numpy(np.stack([p[0] for p in pairs]))
    x2 = torch.from_numpy(np.stack([p[1] for p in pairs]))
    kw = dict(upright=False, extended=True, return_details=True)
    a = _est(x1, x2, pair_ids=[7, 3, 11], **kw)
    b = _est(x1, x2, pair_ids=[7, 3, 11], **kw)
    keys = ("keypoints", "orientations", "descriptors", "matches", "inlier_mask")
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and torch.equal(a[2], b[2])
    for k in keys:
        assert all(torch.equal(u, v) for u, v in zip(a[3][k], b[3][k])), k
    for j, i in enumerate((7, 3, 11)):
        s = _est(x1[j:j + 1], x2[j:j + 1], pair_ids=[i], **kw)
        assert torch.equal(s[0][0], a[0][j]) and bool(s[1][0]) == bool(a[1][j]) and int(s[2][0]) == int(a[2][j])
        assert int(s[3]["best"][0]) == int(a[3]["best"][j])
        for k in keys:
            per_image = k in ("keypoints", "orientations", "descriptors")
            got = (s[3][k][0], s[3][k][1]) if per_image else (s[3][k][0],)
            want = (a[3][k][j], a[3][k][3 + j]) if per_image else (a[3][k][j],)
            assert all(torch.equal(u, v) for u, v in zip(got, want)), (k, j)


@pytest.mark.parametrize("upright", [False, True])
def test_memory_bounds(upright):
    """orient / describe_ex / match_ex with guarded inputs and poisoned allocations: results equal a plain run, guards intact."""
    import memguard as MG
    from hesic_amd import stereo_h
    x1, x2, _ = synthetic.stereo_batch(0, 2, 200, 232)
    u1 = (x1 * 255).round().to(torch.uint8).cuda()
    u2 = (x2 * 255).round().to(torch.uint8).cuda()
    kw = dict(return_details=True, max_keypoints=512, hypotheses=300, upright=upright, extended=True)
    plain = stereo_h.estimate_homography(u1, u2, **kw)
    keys = ("keypoints", "descriptors", "matches", "inlier_mask") + (() if upright else ("orientations",))
    for fill in (MG.NAN_FILL, MG.BIG_FILL):
        g1, g2 = MG.guarded(u1, fill=fill, name="img1"), MG.guarded(u2, fill=fill, name="img2")
        with MG.poisoned_allocations([stereo_h], fill=fill):
            got = stereo_h.estimate_homography(g1, g2, **kw)
            torch.cuda.synchronize()
        g1.check()
        g2.check()
        assert torch.equal(got[0], plain[0]) and torch.equal(got[1], plain[1]) and torch.equal(got[2], plain[2])
        for k in keys:
            assert all(torch.equal(u, v) for u, v in zip(got[3][k], plain[3][k])), k


def test_loader_callable_and_cli(tmp_path):
    """HipHomography(upright=False) as ImageFolder's homography=, and `python -m hesic_amd.stereo_h ROOT --oriented --extended`."""
    from PIL import Image
    from compressai.datasets import ImageFolder, to_tensor
    from hesic_amd import stereo_h
    root = str(tmp_path)
    for side in ("left", "right"):
        os.makedirs(os.path.join(root, "train", side))
    hs = []
    for i in range(3):
        a, b, Hm = synthetic.rotated_stereo_pair(i, 0, 384, 448)
        Image.fromarray((a.transpose(1, 2, 0) * 255).round().astype(np.uint8)).save(os.path.join(root, "train", "left", f"{i:04d}.png"))
        Image.fromarray((b.transpose(1, 2, 0) * 255).round().astype(np.uint8)).save(os.path.join(root, "train", "right", f"{i:04d}.png"))
        hs.append(Hm.astype(np.float64))
    ds = ImageFolder(root, transform=to_tensor, patch_size=(256, 256), split="train", homography=stereo_h.HipHomography(upright=False))
    for i in range(len(ds)):
        random.seed(7 + i)
        item = ds[i]
        random.seed(7 + i)
        y0, x0 = random.randint(0, 384 - 256 - 1), random.randint(0, 448 - 256 - 1)
        want = np.array([[1, 0, -x0], [0, 1, -y0], [0, 0, 1.0]]) @ hs[i] @ np.array([[1, 0, x0], [0, 1, y0], [0, 0, 1.0]])
        assert len(item) == 6
        assert R.corner_error(item[2].numpy(), want / want[2, 2], 256, 256) <= 1.0
    assert stereo_h.main([root, "--split", "train", "--batch", "2", "--oriented", "--extended"]) == 0
    for i in range(3):
        Hs = np.load(os.path.join(root, "train", "H", f"{i:04d}.npy"))
        assert R.corner_error(Hs, hs[i], 384, 448) <= 1.0

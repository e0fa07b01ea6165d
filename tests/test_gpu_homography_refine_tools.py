"""Where users meet the photometric refiner besides the codec: ``stereo_h.write_sidecars(refine=...)`` and ``homography_eval --refine``
(tests/test_gpu_homography_refine.py holds the kernels to the numpy restatement and covers ``codec encode --refine-homography``)."""
import numpy as np
import pytest
import torch

import homography_refine_ref as R
from hesic_amd import homography, homography_eval, stereo_h

pytestmark = pytest.mark.gpu

H, W = 128, 192


@pytest.fixture(scope="module")
def folder(tmp_path_factory):
    """ROOT/test/{left,right}/p{0,1,2}.png: 128 x 192 textures and their known warps (rho 4), as grey RGB PNGs.  Returns (root, truths)."""
    from PIL import Image
    root = tmp_path_factory.mktemp("refine_tools")
    for sub in ("left", "right"):
        (root / "test" / sub).mkdir(parents=True)
    truths = []
    for i in range(3):
        x1, x2, Ht = R.known_case(30 + i, H, W, sigma=2.0, rho=4.0)
        truths.append(Ht)
        for name, x in (("left", x1), ("right", x2)):
            Image.fromarray(np.repeat((x[0] * 255).round().astype(np.uint8)[..., None], 3, -1)).save(root / "test" / name / f"p{i}.png")
    return root, truths


def test_write_sidecars_refines_once(folder):
    """An estimator 3 px off at the corners: with ``refine={}`` the sidecars are within 0.25 px of the truth, without it they are the
    estimator's matrices, as before."""
    root, truths = folder
    off = np.array([[3, -3], [-3, 3], [3, 3], [-3, -3]], np.float64)
    rough = [R.dlt4(R.corners_of(H, W), R.corner_points(Ht, H, W) + off) for Ht in truths]

    def estimator(x1, x2, ids):
        assert x1.dtype == torch.uint8 and tuple(x1.shape[1:]) == (3, H, W)
        return np.stack([rough[i] for i in ids]), [True] * len(ids)

    assert stereo_h.write_sidecars(root, ["test"], batch=2, estimator=estimator, log=lambda m: None) == (3, 0, 0)
    for i in range(3):
        assert np.array_equal(np.load(root / "test" / "H" / f"p{i}.npy"), rough[i] / rough[i][2, 2])
    assert stereo_h.write_sidecars(root, ["test"], batch=2, overwrite=True, estimator=estimator, log=lambda m: None, refine={}) == (3, 0, 0)
    for i in range(3):
        Hm = np.load(root / "test" / "H" / f"p{i}.npy")
        e0, e1 = R.corner_error(rough[i], truths[i], H, W), R.corner_error(Hm, truths[i], H, W)
        print(f"sidecar p{i}: corner error {e0:.3f} -> {e1:.4f} px")
        assert Hm.dtype == np.float64 and Hm[2, 2] == 1.0 and e1 <= 0.25 < e0


def test_homography_eval_refine(folder, monkeypatch):
    """A net that answers zero (the identity) on known warps of rho 3 of a 64-pixel window: ``--refine`` brings every pair below half a pixel,
    the lines and the summary gain their ``refined_*`` entries, and without the flag the records are today's."""
    root, _ = folder
    monkeypatch.setattr(homography.Net, "forward", lambda self, a, b: torch.zeros(a.shape[0], 4, 2, device=a.device))
    args = [str(root), "--checkpoint", "synthetic", "--rho", "3", "--picsize", "128", "--patchsize", "64", "--batch", "2"]
    plain = homography_eval.main(args, log=lambda _: None)
    recs = homography_eval.main(args + ["--refine"], log=lambda _: None)
    assert all(set(r) == {"stem", "corner_error", "identity_corner_error"} for r in plain[:-1])
    assert not any(k.startswith("refined") for k in plain[-1])
    lines, summary = recs[:-1], recs[-1]
    assert len(lines) == 3 and all(set(r) == {"stem", "corner_error", "identity_corner_error", "refined_corner_error"} for r in lines)
    for r, p in zip(lines, plain[:-1]):
        print(f"eval {r['stem']}: corner error {r['corner_error']:.3f} -> {r['refined_corner_error']:.4f} px")
        assert {k: r[k] for k in p} == p and r["corner_error"] == r["identity_corner_error"] > 0.5
        assert r["refined_corner_error"] < 0.5
    ref = np.array([r["refined_corner_error"] for r in lines])
    assert {k: summary[k] for k in plain[-1]} == plain[-1]
    assert summary["refined_mean_corner_error"] == float(ref.mean()) and summary["refined_median_corner_error"] == float(np.median(ref))
    assert summary["refined_under_1px"] == 1.0 and summary["refined_under_3px"] == 1.0

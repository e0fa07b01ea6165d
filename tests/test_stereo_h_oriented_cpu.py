"""Oriented and extended SURF of the stereo homography estimator without a GPU: the NumPy restatement
(tests/stereo_h_oriented_ref.py) on pairs with in-plane rotation, its identity frame, the fastAtan2 polynomial, the options of the
command line and the C ABI of the new entry points."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import stereo_h_ref as R                                      # noqa: E402
import stereo_h_oriented_ref as O                             # noqa: E402
from hesic_amd import synthetic                               # noqa: E402

THETAS = (0, 30, 60, 90, 135, 180, 270)


@pytest.mark.parametrize("theta", THETAS)
def test_oriented_restatement_recovers_rotation(theta):
    """Oriented SURF recovers H within 1 px at every rotation; upright SURF does not from 60 degrees on (invalid or > 5 px off)."""
    x1, x2, Ht = synthetic.rotated_stereo_pair(0, theta, 512, 512)
    o = O.estimate(x1, x2, upright=False)
    assert o["H"] is not None and R.corner_error(o["H"], Ht, 512, 512) <= 1.0
    assert o["fallbacks"] == 0                                  # every keypoint got a direction
    if theta >= 60:
        u = O.estimate(x1, x2, upright=True)
        assert u["H"] is None or R.corner_error(u["H"], Ht, 512, 512) > 5.0


def test_rotated_pair_ground_truth():
    """View 2 is view 1 warped by H: pixels of view 1 land on the same values in view 2 (up to the added noise and interpolation)."""
    x1, x2, Ht = synthetic.rotated_stereo_pair(3, 135, 256, 256)
    ys, xs = np.mgrid[64:192:8, 64:192:8]
    p = np.stack([xs.ravel(), ys.ravel(), np.ones(xs.size)]) .astype(np.float64)
    q = Ht.astype(np.float64) @ p
    u, v = q[0] / q[2], q[1] / q[2]
    got = x2[:, np.rint(v).astype(int), np.rint(u).astype(int)]
    want = x1[:, ys.ravel(), xs.ravel()]
    assert float(np.abs(got - want).mean()) < 0.05


def test_identity_frame_is_upright():
    """describe_ex with (1, 0) everywhere (or no orientation) reproduces describe bit for bit; 128-d has unit norm."""
    x1, _, _ = synthetic.stereo_pair(2, 256, 256)
    I = R.integral(R.grey(x1))
    kps = R.select(R.detect(I), 4096)
    d, n = R.describe(I, kps)
    one = np.tile(np.array([[1, 0]], np.float32), (len(kps), 1))
    for ori in (one, None):
        de, ne = O.describe_ex(I, kps, ori, 64)
        assert np.array_equal(de, d) and np.array_equal(ne, n)
    d128, n128 = O.describe_ex(I, kps, one, 128)
    assert d128.shape == (len(kps), 128) and np.allclose(n128, 1, atol=1e-5)
    s = d128.reshape(-1, 16, 8).astype(np.float64)               # the two halves of each split sum add up to the 64-d sum
    v = np.stack([s[..., 0] + s[..., 2], s[..., 1] + s[..., 3], s[..., 4] + s[..., 6], s[..., 5] + s[..., 7]], -1).reshape(-1, 64)
    assert np.abs(v / np.linalg.norm(v, axis=1, keepdims=True) - d).max() < 1e-5
    assert (s[..., 1] >= 0).all() and (s[..., 7] >= 0).all() and (s[..., 2] <= s[..., 3]).all()


def test_fast_atan2_polynomial():
    """Within 0.01 degrees of atan2 everywhere, in [0, 360]; the quadrant rules give 0 / 90 / 180 / 270 on the axes."""
    t = np.linspace(0, 2 * np.pi, 100001)
    for r in (1e-3, 1.0, 3e5):
        x, y = (r * np.cos(t)).astype(np.float32), (r * np.sin(t)).astype(np.float32)
        a = O.fast_atan2(y, x)
        ref = np.degrees(np.arctan2(y.astype(np.float64), x.astype(np.float64))) % 360
        err = np.abs((a - ref + 180) % 360 - 180)
        assert float(err.max()) < 0.01 and float(a.min()) >= 0 and float(a.max()) <= 360
    ax = O.fast_atan2(np.float32([0, 1, 0, -1]), np.float32([1, 0, -1, 0]))
    assert ax.tolist() == [0.0, 90.0, 180.0, 270.0]


def test_orientation_table():
    i, j, w = O.ori_table()
    assert len(w) == 109 and w.dtype == np.float32 and (i * i + j * j < 36).all()
    assert list(zip(i[:3], j[:3])) == [(-5, -3), (-5, -2), (-5, -1)]          # row-major, i outer
    c = int(np.argmax(w))
    assert (i[c], j[c]) == (0, 0) and c == 54 and 0.8 < float(w.sum()) < 1.0


def test_cli_passes_the_descriptor_options(monkeypatch):
    from hesic_amd import stereo_h
    seen = []
    monkeypatch.setattr(stereo_h, "write_sidecars", lambda *a, **kw: seen.append(kw))
    monkeypatch.setattr(torch.cuda, "is_available", lambda: True)
    assert stereo_h.main(["root", "--oriented", "--extended"]) == 0
    assert stereo_h.main(["root"]) == 0
    assert (seen[0]["upright"], seen[0]["extended"]) == (False, True) and (seen[1]["upright"], seen[1]["extended"]) == (True, False)


@pytest.mark.parametrize("fmt", ["bf16", "f16"])
def test_oriented_abi(fmt):
    """The three new entry points are declared in include/hesic_stereo_h.h, bound in _STEREO_H_SIGS and exported by both libraries;
    each rejects a null pointer, a bad dim and a max_kp above the cap with HESIC_EINVAL."""
    from hesic_amd import _lib as L
    if not os.path.exists(L.LIB_PATH):
        import __graft_entry__ as ge
        ge.build()
    new = ("hesic_stereo_h_orient", "hesic_stereo_h_describe_ex", "hesic_stereo_h_match_ex")
    declared = L.declared_symbols("hesic_stereo_h.h")
    assert all(s in declared and s in L._STEREO_H_SIGS for s in new)
    assert not set(new) & set(L.declared_symbols())
    path = L.LIB_PATH_F16 if fmt == "f16" else L.LIB_PATH
    exported = subprocess.check_output(["nm", "-D", "--defined-only", path], text=True)
    assert all(f" T {s}\n" in exported for s in new)
    l = L.lib(torch.float16 if fmt == "f16" else torch.bfloat16)
    p = L._vp(4096)                                             # never dereferenced: the arguments are refused first
    assert l.hesic_stereo_h_orient(None, p, p, 2, 64, 64, 16, p, None) == -1 and b"orient" in l.hesic_last_error()
    assert l.hesic_stereo_h_orient(p, p, p, 2, 64, 64, 4097, p, None) == -1
    assert l.hesic_stereo_h_describe_ex(p, p, None, p, 2, 64, 64, 16, 96, p, p, None) == -1 and b"dim 96" in l.hesic_last_error()
    assert l.hesic_stereo_h_describe_ex(p, None, p, p, 2, 64, 64, 16, 64, p, p, None) == -1
    assert l.hesic_stereo_h_match_ex(p, p, p, 1, 64, 64, 16, 16, 32, p, 1 << 20, p, p, None) == -1 and b"dim 32" in l.hesic_last_error()
    assert l.hesic_stereo_h_match_ex(p, p, None, 1, 64, 64, 16, 16, 128, p, 1 << 20, p, p, None) == -1
    assert l.hesic_stereo_h_match_ex(p, p, p, 1, 64, 64, 16, 16, 128, p, 16, p, p, None) == -1 and b"workspace" in l.hesic_last_error()

"""The numpy restatement of the photometric homography refiner (tests/homography_refine_ref.py) against known answers: it is the reference
of tests/test_gpu_homography_refine.py, so it is checked by itself first."""
import numpy as np
import pytest

import homography_refine_ref as R

H, W = 96, 128
EYE = np.eye(3, dtype=np.float32)


@pytest.fixture(scope="module")
def cases():
    return [R.known_case(seed, H, W, sigma=2.0, rho=8.0) for seed in range(6)]


def test_known_warps_are_recovered(cases):
    """sigma = 2, rho = 8, 96 x 128, seeds 0 - 5, identity start, 3 levels x 10 iterations: every warp to <= 0.25 px at the corners."""
    for seed, (x1, x2, Ht) in enumerate(cases):
        start = R.corner_error(EYE, Ht, H, W)
        h, info = R.refine(x1, x2, EYE, levels=3, iters=10)
        err = R.corner_error(h, Ht, H, W)
        print(f"seed {seed}: corner error {start:.3f} -> {err:.5f} px, cost {info['cost_before']:.3e} -> {info['cost_after']:.3e}")
        assert start > 4.0                                  # the start is far from the answer
        assert err <= 0.25, (seed, err)
        assert info["refined"] and info["levels_used"] == 3 and info["cost_after"] < info["cost_before"]
        assert h.dtype == np.float32 and h[2, 2] == 1.0


def test_cost_never_increases(cases):
    """Within a level every accepted cost is below the one before it, and the reported pair is ordered."""
    for x1, x2, _ in cases[:3]:
        for huber in (None, 0.05):
            trace = []
            _, info = R.refine(x1, x2, EYE, levels=3, iters=10, huber=huber, trace=trace)
            assert info["cost_after"] <= info["cost_before"]
            for l in range(3):
                costs = [c for lv, c in trace if lv == l]
                assert len(costs) >= 1 and all(b < a for a, b in zip(costs, costs[1:])), (l, costs)


def test_three_levels_do_no_worse_than_one(cases):
    """One level with the same number of candidates does no better than three levels (the pyramid is part of the feature)."""
    for x1, x2, Ht in cases[:3]:
        e1 = R.corner_error(R.refine(x1, x2, EYE, levels=1, iters=30)[0], Ht, H, W)
        e3 = R.corner_error(R.refine(x1, x2, EYE, levels=3, iters=10)[0], Ht, H, W)
        assert e3 <= max(e1, 0.25)


def test_iters_zero_and_zero_overlap_return_the_input(cases):
    x1, x2, _ = cases[0]
    h0 = (EYE + np.float32(0.001) * np.arange(9, dtype=np.float32).reshape(3, 3)).astype(np.float32)
    h, info = R.refine(x1, x2, h0, iters=0)
    assert h.tobytes() == h0.tobytes() and info["accepted"] == 0 and info["cost_after"] == info["cost_before"] > 0
    far = np.array([[1, 0, 2 * W], [0, 1, 0], [0, 0, 1]], np.float32)
    h, info = R.refine(x1, x2, far)
    assert h.tobytes() == far.tobytes() and info["accepted"] == 0 and info["rejected"] == 0 and info["valid_share"] == 0.0
    assert all(np.isfinite(float(v)) for v in info.values())
    sing = np.zeros((3, 3), np.float32)
    h, info = R.refine(x1, x2, sing)
    assert h.tobytes() == sing.tobytes() and info["accepted"] == 0 and all(np.isfinite(float(v)) for v in info.values())


def test_a_view_without_contrast_is_left_alone(cases):
    """x2 constant (zero or not): every level does nothing and the input comes back, although the start overlaps well; one textured pixel is
    enough for the walk to run (the rule is about no contrast at all, not about little)."""
    x1, x2, _ = cases[0]
    h0 = np.array([[1.01, 0.002, 1.5], [-0.003, 0.99, -2.25], [1e-5, -2e-5, 1.0]], np.float32)
    for value in (0.0, 0.4375):
        h, info = R.refine(x1, np.full_like(x2, value), h0)
        assert h.tobytes() == h0.tobytes() and info["accepted"] == 0 and info["rejected"] == 0
        assert info["cost_after"] == info["cost_before"] > 0 and all(np.isfinite(float(v)) for v in info.values())
    dot = np.zeros_like(x2)
    dot[0, 40, 60] = 1.0
    assert R.refine(x1, dot, h0)[1]["accepted"] + R.refine(x1, dot, h0)[1]["rejected"] > 0


def test_huber_beats_l2_on_an_occluded_patch():
    for seed in range(6):
        x1, x2, Ht = R.huber_case(seed, H, W)
        eh = R.corner_error(R.refine(x1, x2, EYE, huber=0.05)[0], Ht, H, W)
        el = R.corner_error(R.refine(x1, x2, EYE)[0], Ht, H, W)
        print(f"seed {seed}: huber {eh:.4f} px, L2 {el:.4f} px")
        assert eh <= 0.1 and eh < el, (seed, eh, el)


@pytest.mark.parametrize("shape", [(96, 128), (75, 101), (33, 47), (16, 16), (15, 40), (129, 257)])
def test_pyramid_sizes(shape):
    h, w = shape
    sizes = R.level_sizes(h, w, 6)
    assert len(sizes) == (0 if min(h, w) < 16 else sum(1 for l in range(6) if min(h >> l, w >> l) >= 16))
    for l, (hl, wl) in enumerate(sizes):
        assert (hl, wl) == (h >> l, w >> l) and min(hl, wl) >= 16
    assert R.level_sizes(h, w, 2) == sizes[:2]
    if sizes:
        rng = np.random.default_rng(1)
        x = rng.random((3, h, w), dtype=np.float32)
        pyr = R.pyramid(x, 6)
        assert [p.shape for p in pyr] == sizes and all(p.dtype == np.float32 for p in pyr)
        g = x.astype(np.float64).mean(0)
        assert np.abs(pyr[0] - g).max() <= 2.0 ** -24
        for l in range(1, len(pyr)):                         # a level is the block mean of level 0 over the part it keeps, to fp32 rounding
            hl, wl = sizes[l]
            s = 2 ** l
            blk = g[:hl * s, :wl * s].reshape(hl, s, wl, s).mean((1, 3))
            assert np.abs(pyr[l] - blk).max() <= (l + 1) * 2.0 ** -24


def test_level_transition_round_trip_and_meaning():
    """A_l maps level-l pixel centres as A maps the level-0 positions they stand for; there and back is the identity to rounding."""
    A = R.norm22(R.inv3(R.known_warp(3, H, W, 8.0)))
    for l in (1, 2, 3):
        Al = R.to_level(A, 0, l)
        T, Ti = R.level_T(l)
        p = np.array([5.0, 7.0, 1.0])
        q0 = A @ (T @ p)
        ql = T @ (Al @ p)
        assert np.allclose(q0[:2] / q0[2], ql[:2] / ql[2], rtol=0, atol=1e-9)
        assert np.allclose(R.to_level(Al, l, 0), A, rtol=1e-12, atol=1e-12) and Al[2, 2] == 1.0


def test_normal_equations_are_the_gradient_and_gauss_newton_hessian():
    """J^T r is half the derivative of sum r^2 in the eight entries of A (central differences, away from cell borders in the mean)."""
    x1, x2, Ht = R.known_case(1, 48, 64, sigma=3.0, rho=2.0)
    I1, I2 = R.grey(x1), R.grey(x2)
    A = R.norm22(R.inv3(R.known_warp(2, 48, 64, 2.0)))           # another seed's warp: a small residual, not a zero one
    s = R.normal_equations(I1, I2, A)
    assert s[45] > 0.8 * 48 * 64
    for k in range(8):
        e = np.zeros(9)
        e[k] = 1e-7 * max(1.0, abs(A.reshape(9)[k]))
        up = R.normal_equations(I1, I2, (A.reshape(9) + e).reshape(3, 3))
        dn = R.normal_equations(I1, I2, (A.reshape(9) - e).reshape(3, 3))
        if up[45] != s[45] or dn[45] != s[45]:
            continue
        num = (up[44] - dn[44]) / (2 * e[k]) / 2
        assert abs(num - s[36 + k]) <= 2e-3 * max(abs(s[36 + k]), np.sqrt(s[R.tri_index(k, k)] * s[44])), (k, num, s[36 + k])


def test_stereo_h_cli_passes_refine(monkeypatch):
    import torch
    from hesic_amd import stereo_h
    seen = []
    monkeypatch.setattr(stereo_h, "write_sidecars", lambda *a, **kw: seen.append(kw))
    monkeypatch.setattr(torch.cuda, "is_available", lambda: True)
    assert stereo_h.main(["root", "--refine"]) == 0 and stereo_h.main(["root"]) == 0
    assert seen[0]["refine"] == {} and seen[1]["refine"] is None


def test_eval_summary_gains_refined_entries_only_with_refined_lines():
    from hesic_amd import homography_eval
    lines = [{"stem": "a", "corner_error": 2.0, "identity_corner_error": 5.0}, {"stem": "b", "corner_error": 0.5, "identity_corner_error": 6.0}]
    plain = homography_eval.summarise(lines, 0.1, 0.05)
    assert not any(k.startswith("refined") for k in plain)
    for r, e in zip(lines, (0.25, 3.5)):
        r["refined_corner_error"] = e
    s = homography_eval.summarise(lines, 0.1, 0.05)
    assert {k: s[k] for k in plain} == plain
    assert (s["refined_mean_corner_error"], s["refined_median_corner_error"], s["refined_under_1px"], s["refined_under_3px"]) == (1.875, 1.875, 0.5, 0.5)
    a = homography_eval.parser().parse_args(["root", "--checkpoint", "synthetic"])
    assert a.refine is False and (a.refine_levels, a.refine_iters) == (3, 10)


def test_refine_h_matrix_refusals_need_no_device():
    import torch
    from hesic_amd import geometry, homography
    x = torch.zeros(1, 3, 32, 32)
    with pytest.raises(NotImplementedError, match="align_corners"):
        homography.refine_h_matrix(x, x, torch.eye(3)[None], align_corners=False)
    with pytest.MonkeyPatch.context() as mp:
        mp.setattr(geometry, "DEFAULT_ALIGN_CORNERS", False)
        with pytest.raises(NotImplementedError, match="align_corners"):
            homography.refine_h_matrix(x, x, torch.eye(3)[None])
    with pytest.raises(TypeError, match="float32"):
        homography.refine_h_matrix(x.half(), x.half(), torch.eye(3)[None])
    with pytest.raises(RuntimeError, match="at least 16"):
        homography.refine_h_matrix(x[..., :15], x[..., :15], torch.eye(3)[None])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        homography.refine_h_matrix(x, x, torch.eye(3)[None])


def test_host_entry_points_and_argument_checks():
    """The host-side entry points answer without a device, and the launching ones refuse bad arguments before any launch."""
    import ctypes as C
    import os
    from hesic_amd import _lib as L
    if not os.path.exists(L.LIB_PATH):
        import __graft_entry__ as ge
        ge.build()
    l = L.lib()
    for (h, w, lv) in [(96, 128, 3), (75, 101, 6), (33, 47, 3), (15, 40, 3), (512, 512, 3)]:
        sizes = R.level_sizes(h, w, lv)
        assert l.hesic_hrefine_levels(h, w, lv) == len(sizes)
        assert l.hesic_hrefine_pyramid_elems(4, h, w, lv) == sum(2 * 4 * a * b for a, b in sizes)
        for a, b in sizes:
            assert l.hesic_hrefine_blocks(a, b) == min(64, -(-a * b // 256))
    assert l.hesic_hrefine_levels(96, 128, 0) == -1 and l.hesic_hrefine_levels(96, 128, 7) == -1
    assert l.hesic_homography_refine_ws_bytes(2, 96, 128, 3) >= 4 * l.hesic_hrefine_pyramid_elems(2, 96, 128, 3) + 2 * (64 * 46 + 80) * 8
    s4 = (C.c_int64 * 4)(3 * 32 * 32, 32 * 32, 32, 1)
    p = C.c_void_p(256)
    assert l.hesic_homography_refine(p, s4, p, s4, 1, 2, 32, 32, p, 3, 10, 0.0, 0.25, p, 1 << 30, p, p, None) == -1 and b"C is 1 or 3" in l.hesic_last_error()
    assert l.hesic_homography_refine(p, s4, p, s4, 1, 3, 8, 32, p, 3, 10, 0.0, 0.25, p, 1 << 30, p, p, None) == -1
    assert l.hesic_homography_refine(p, s4, p, s4, 1, 3, 32, 32, p, 3, 10, 0.0, 0.25, p, 64, p, p, None) == -1 and b"workspace" in l.hesic_last_error()
    assert l.hesic_homography_refine(p, s4, p, s4, 1, 3, 32, 32, p, 9, 10, 0.0, 0.25, p, 1 << 30, p, p, None) == -1
    assert l.hesic_hrefine_normal_eq(p, 1, 32, 32, 2, 2, p, 9, 0.0, p, None) == -1 and b"level" in l.hesic_last_error()

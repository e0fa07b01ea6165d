"""The fp64 reference of the differentiable homography geometry (tests/homography_train_ref.py) and the bars the GPU tests hold the kernels
to: the reference against the pinned oracle, its closed-form gradients against fp64 autograd and central differences, the bars against
seven planted defects, the descent the GPU test repeats, and the C ABI of include/hesic_homography_train.h.  No GPU."""
import subprocess

import numpy as np
import pytest
import torch

import homography_train_ref as R
from hesic_amd import _lib as L
from oracle import hesic_oracle as O


def _rel(a, b):
    return float((a - b).abs().max()) / float(b.abs().max())


@pytest.mark.parametrize("fmt", ["bf16", "f16"])
def test_abi_header_bindings_exports(fmt):
    declared = L.declared_symbols("hesic_homography_train.h")
    assert declared == ["hesic_h_from_delta_backward", "hesic_perspective_transform_backward", "hesic_photometric_backward",
                        "hesic_photometric_forward", "hesic_warp_perspective_backward_m"]
    assert set(declared) == set(L._HOMOGRAPHY_TRAIN_SIGS)
    assert not set(declared) & set(L.declared_symbols())                # a header of its own: include/hesic_hip.h does not list them
    text = open(L.header_path("hesic_homography_train.h")).read()
    assert f"#define HESIC_HTRAIN_MAX_BLOCKS {L.HTRAIN_MAX_BLOCKS}\n" in text
    assert f"#define HESIC_HTRAIN_PARTIAL_WIDTH {L.HTRAIN_PARTIAL_WIDTH}\n" in text
    assert "#define HESIC_ABI_VERSION 3" in open(L.header_path("hesic_hip.h")).read() and L.ABI_VERSION == 3
    exported = subprocess.check_output(["nm", "-D", "--defined-only", L.LIB_PATH_F16 if fmt == "f16" else L.LIB_PATH], text=True)
    for s in declared:
        assert f" T {s}\n" in exported, s


def test_public_interface_refuses_cpu_tensors():
    from hesic_amd import homography
    delta, img_a, patch_b, corners = R.stage1_inputs("tails_40x52_p21x35")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        homography.photometric_loss(delta, img_a, patch_b, corners)
    with pytest.raises(RuntimeError, match="delta only"):
        homography.photometric_loss(delta, img_a.clone().requires_grad_(), patch_b, corners)


@pytest.mark.parametrize("name", ["tails_40x52_p21x35", "96_p64_d24", "corner_64_p32"])
def test_reference_loss_equals_oracle(name):
    """loss == L1(O.warp_perspective(img_a, inverse(O.get_perspective_transform(c0, corners + delta)), dsize), patch_b).  The oracle's DLT
    returns fp32 (one rounding of h: coordinates move by ~1e-5 px), hence 1e-5."""
    delta, img_a, patch_b, corners = R.stage1_inputs(name)
    for ac in (True, False):
        h = O.get_perspective_transform(corners - corners[:, :1], corners + delta)
        want = (O.warp_perspective(img_a.double(), torch.inverse(h.double()), tuple(patch_b.shape[-2:]), align_corners=ac) - patch_b).abs().mean()
        assert abs(float(R.photometric_torch(delta, img_a, patch_b, corners, ac)) - float(want)) < 1e-5
        assert abs(float(R.photometric_closed(delta, img_a, patch_b, corners, ac)[0]) - float(want)) < 1e-5


@pytest.mark.parametrize("name", sorted(R.STAGE1_CASES))
def test_stage1_inputs_are_well_conditioned(name):
    """No residual of the fp64 reference is close enough to zero for rounding to decide its sign (homography_train_ref.MIN_ABS_RESIDUAL), and
    the case built for out-of-image taps has them: pixels with no, one (the image's corner), two (its edges) and four valid taps."""
    args = R.stage1_inputs(name)
    assert all(v.dtype == torch.float32 for v in args) and float((args[0] - args[0].round()).abs().min()) > 1e-3      # non-integer deltas
    for ac in (True, False):
        assert R.min_abs_residual(*args, ac) >= R.MIN_ABS_RESIDUAL
    if name == "corner_64_p32":
        delta, img_a, patch_b, corners = args
        h = R.dlt_torch((corners - corners[:, :1]).double(), (corners + delta).double())
        taps = R._taps(torch.ones_like(img_a).double(), h, patch_b.shape[-2:], True)[0]
        valid = sum(taps)[:, 0]                                      # valid taps per pixel
        assert float((valid == 0).float().mean()) > 0.2 and all(int((valid == k).sum()) > 0 for k in (1, 2, 4))


@pytest.mark.parametrize("ac", [True, False], ids=["ac1", "ac0"])
@pytest.mark.parametrize("name", ["tails_40x52_p21x35", "corner_64_p32"])
def test_closed_form_photometric_gradient(name, ac):
    """The chain rule as the kernels apply it == fp64 autograd (grid_sample's zero-padding gradient included) == central differences."""
    delta, img_a, patch_b, corners = R.stage1_inputs(name)
    loss, g = R.photometric_closed(delta, img_a, patch_b, corners, ac)
    d = delta.double().requires_grad_()
    la = R.photometric_torch(d, img_a, patch_b, corners, ac)
    (ga,) = torch.autograd.grad(la, d)
    assert abs(float(loss) - float(la.detach())) < 1e-13 and _rel(g, ga) < 1e-10
    eps = 1e-5
    for idx in [(0, 0, 0), (1, 2, 1), (delta.shape[0] - 1, 3, 0)]:
        dp, dm = delta.double().clone(), delta.double().clone()
        dp[idx] += eps
        dm[idx] -= eps
        fd = (R.photometric_torch(dp, img_a, patch_b, corners, ac) - R.photometric_torch(dm, img_a, patch_b, corners, ac)) / (2 * eps)
        assert abs(float(fd) - float(g[idx])) < 2e-3 * float(g.abs().max())      # a few of the 2205+ residuals change sign inside +-eps


@pytest.mark.parametrize("inverse_map", [False, True], ids=["fwdmap", "invmap"])
@pytest.mark.parametrize("ac", [True, False], ids=["ac1", "ac0"])
def test_closed_form_dM(ac, inverse_map):
    src = R.smooth_images(7, 2, 3, 24, 30).double()
    d_dst = (R.smooth_images(8, 2, 3, 17, 21).double() - 0.5)
    M = torch.tensor([[[1.05, 0.04, 2.5], [-0.03, 0.97, 1.25], [4e-4, -3e-4, 1.0]], [[0.9, -0.1, -3.5], [0.08, 1.1, 4.75], [-6e-4, 2e-4, 1.02]]],
                     dtype=torch.float64)
    Mg = M.clone().requires_grad_()
    A = Mg if inverse_map else torch.linalg.inv(Mg)
    (ga,) = torch.autograd.grad((R.warp_torch(src, A, (17, 21), ac) * d_dst).sum(), Mg)
    assert _rel(R.warp_dM_closed(src, M, d_dst, (17, 21), ac, inverse_map), ga) < 1e-10


def test_closed_form_dlt_adjoint_and_h_adjust():
    from hesic_amd import synthetic
    _, _, corners = synthetic.homography_batch(1, 4)
    delta = R.deltas(11, 4, 24.0)
    c0 = (corners - corners[:, :1]).double()
    src, dst = c0.clone().requires_grad_(), (c0 + delta.double()).requires_grad_()
    gH = torch.from_numpy(np.random.Generator(np.random.PCG64(3)).normal(size=(4, 3, 3)))
    gs, gd = torch.autograd.grad((R.dlt_torch(src, dst) * gH).sum(), (src, dst))
    cs, cd = R.dlt_adjoint_closed(src.detach(), dst.detach(), gH.reshape(4, 9)[:, :8])
    assert _rel(cs, gs) < 1e-9 and _rel(cd, gd) < 1e-9
    # the reference's DLT is the oracle's (which rounds its result to fp32)
    assert float((R.dlt_torch(src.detach(), dst.detach()) - O.get_perspective_transform(src.detach(), dst.detach())).abs().max()) < 1e-5
    for (ih, iw, pic) in [(256, 256, 256), (512, 512, 256), (860, 1080, 256)]:
        d = delta.double().requires_grad_()
        Hm = R.h_matrix_from_delta_torch(corners.double(), d, ih, iw, pic)
        want = O.h_matrix_from_delta(corners, delta, ih, iw, pic)
        assert float(((Hm.detach() - want).abs() / (want.abs() + 1e-3)).max()) < 1e-4
        (ga,) = torch.autograd.grad((Hm * gH).sum(), d)
        assert _rel(R.h_matrix_from_delta_grad_closed(corners.double(), delta.double(), ih, iw, pic, gH), ga) < 1e-9


@pytest.mark.parametrize("mutate", R.MUTATIONS)
def test_bars_reject_planted_defects(mutate):
    """Each defect, planted in the closed form, has to miss the bars the GPU tests use -- on a case built to show it."""
    name, ac = {"drop_ac_factor": ("tails_40x52_p21x35", False), "outside_tap": ("corner_64_p32", True)}.get(mutate, ("tails_40x52_p21x35", True))
    args = R.stage1_inputs(name)
    loss, g = R.photometric_closed(*args, ac)
    assert R.within_bars(loss, g, loss, g)[0]
    bl, bg = R.photometric_closed(*args, ac, mutate=mutate)
    ok, le, ge = R.within_bars(bl, bg, loss, g)
    print(f"{mutate}: loss error {le:.2e} (bar {R.LOSS_BAR:.0e}), gradient error {ge:.2e} (bar {R.GRAD_BAR:.0e})")
    assert not ok and ge > 10 * R.GRAD_BAR


@pytest.mark.parametrize("name", ["tails_40x52_p21x35", "96_p64_d24", "real_256_p128_d32"])
def test_fp32_torch_evaluation_is_inside_the_bars(name):
    """The noise floor: the same reference evaluated by plain fp32 torch ops sits well inside the bars, so they ask nothing impossible."""
    args = R.stage1_inputs(name)
    loss, g = R.photometric_closed(*args, True)
    d = args[0].clone().requires_grad_()
    l32 = R.photometric_torch(d, *args[1:], True, dtype=torch.float32)
    (g32,) = torch.autograd.grad(l32, d)
    ok, le, ge = R.within_bars(l32, g32, loss, g)
    print(f"{name}: fp32 torch loss error {le:.2e}, gradient error {ge:.2e} of max|g|")
    assert ok


@pytest.mark.parametrize("which", [0, 1])
def test_descent_reference(which):
    """The GPU descent test on the reference itself: Adam(lr=0.2) on delta from 0.25, 150 steps, inside the same bars."""
    img_a, patch_b, corners, true = R.descent_setup(which)
    delta = torch.full_like(true, 0.25)
    opt = torch.optim.Adam([delta], lr=0.2)
    start = float((delta - true).norm(dim=-1).mean())
    for _ in range(150):
        loss, g = R.photometric_closed(delta, img_a, patch_b, corners, True)
        delta.grad = g.float()
        opt.step()
    err = float((delta - true).norm(dim=-1).mean())
    loss = float(R.photometric_closed(delta, img_a, patch_b, corners, True)[0])
    print(f"descent {which}: corner error {start:.3f} -> {err:.4f} px, loss {loss:.5f}")
    assert err <= 0.25 and loss <= 0.02

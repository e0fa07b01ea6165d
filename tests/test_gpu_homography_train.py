"""The differentiable homography geometry on the GPU (include/hesic_homography_train.h, csrc/homography_train.hip) against the fp64
reference of tests/homography_train_ref.py: the photometric loss with its gradient to the corner deltas, d(warp_perspective)/dM, the DLT
adjoint behind get_perspective_transform / h_matrix_from_delta, run-to-run bit identity, a descent through the HIP loss, and the same
launches inside guarded, poisoned allocations.

Bars (homography_train_ref.LOSS_BAR / GRAD_BAR): |loss - ref| <= 1e-6 max(1, |ref|); max |g - ref| <= 2e-5 max |ref|.  Each case prints
"homography_train_parity <case> <loss error> <gradient error / max|g|>"  before anything is asserted; the values measured when the tests were
written are in profiles/homography_train_parity.json."""
import contextlib

import numpy as np
import pytest
import torch

import homography_train_ref as R
import memguard
from hesic_amd import functional as Fn
from hesic_amd import geometry, homography, synthetic

pytestmark = pytest.mark.gpu

_REF = {}


def _ref(name, ac):
    """The fp64 reference of a stage-1 case, computed once and shared."""
    if (name, ac) not in _REF:
        args = R.stage1_inputs(name)
        _REF[name, ac] = (args, R.photometric_closed(*args, ac))
    return _REF[name, ac]


@contextlib.contextmanager
def _convention(ac):
    """photometric_loss follows geometry.DEFAULT_ALIGN_CORNERS, as warp_perspective does."""
    with pytest.MonkeyPatch.context() as mp:
        mp.setattr(geometry, "DEFAULT_ALIGN_CORNERS", ac)
        yield


def _strided(t):
    """``t``'s values as a non-contiguous view: channels last, every second column of a wider buffer, one row of slack per image."""
    B, C, H, W = t.shape
    buf = torch.full((B, H + 1, 2 * W, C), float("nan"), dtype=t.dtype, device=t.device)
    v = buf[:, :H, ::2, :].permute(0, 3, 1, 2)
    v.copy_(t)
    return v


def _run(delta, img_a, patch_b, corners):
    d = delta.cuda().requires_grad_()
    loss = homography.photometric_loss(d, img_a, patch_b, corners.cuda())
    (g,) = torch.autograd.grad(loss, d)
    return loss.detach(), g


@pytest.mark.parametrize("ac", [True, False], ids=["ac1", "ac0"])
@pytest.mark.parametrize("name", sorted(R.STAGE1_CASES))
def test_photometric_loss_and_gradient(name, ac):
    (delta, img_a, patch_b, corners), (rl, rg) = _ref(name, ac)
    a, b = img_a.cuda(), patch_b.cuda()
    if name.startswith("c3"):
        a, b = _strided(a), _strided(b)
        assert not a.is_contiguous() and not b.is_contiguous()
    with _convention(ac):
        loss, g = _run(delta, a, b, corners)
        loss2, g2 = _run(delta, a, b, corners)
    assert loss.shape == () and loss.dtype == torch.float32 and loss.is_cuda and g.shape == delta.shape
    ok, le, ge = R.within_bars(loss.cpu(), g.cpu(), rl, rg)
    print(f"homography_train_parity photometric/{name}/ac{int(ac)} {le:.3e} {ge:.3e}")
    assert le <= R.LOSS_BAR, (name, ac, le)
    assert ge <= R.GRAD_BAR, (name, ac, ge)
    assert torch.equal(loss, loss2) and torch.equal(g, g2)            # no atomics: the same bits in every run


def test_upstream_gradient_is_read_on_the_device():
    (delta, img_a, patch_b, corners), _ = _ref("tails_40x52_p21x35", True)
    a, b, c = img_a.cuda(), patch_b.cuda(), corners.cuda()
    d = delta.cuda().requires_grad_()
    with _convention(True):
        (g1,) = torch.autograd.grad(homography.photometric_loss(d, a, b, c), d)
        (g3,) = torch.autograd.grad(homography.photometric_loss(d, a, b, c) * -3.0, d)
        with torch.no_grad():
            l0 = homography.photometric_loss(d, a, b, c)
        assert not l0.requires_grad
    assert float((g3 + 3.0 * g1).abs().max()) <= 1e-6 * float(g1.abs().max())
    with pytest.raises(RuntimeError, match="delta only"):
        homography.photometric_loss(d, a.clone().requires_grad_(), b, c)


_M = torch.tensor([[[1.05, 0.04, 2.5], [-0.03, 0.97, 1.25], [4e-4, -3e-4, 1.0]], [[0.9, -0.1, -3.5], [0.08, 1.1, 4.75], [-6e-4, 2e-4, 1.02]]])


@pytest.mark.parametrize("inverse_map", [False, True], ids=["fwdmap", "invmap"])
@pytest.mark.parametrize("ac", [True, False], ids=["ac1", "ac0"])
@pytest.mark.parametrize("layout", ["c1", "c3_strided"])
def test_warp_perspective_matrix_gradient(layout, ac, inverse_map):
    """geometry.warp_perspective hands M its gradient (it was silently dropped), through the in-kernel inverse or not; the gradient of src
    is what it was.  Some destination pixels fall outside the 40 x 52 source."""
    C = 1 if layout == "c1" else 3
    src, d_dst = R.smooth_images(21, 2, C, 40, 52), R.smooth_images(22, 2, C, 33, 47) - 0.5
    want = R.warp_dM_closed(src, _M, d_dst, (33, 47), ac, inverse_map)
    s, gd = src.cuda(), d_dst.cuda()
    if layout == "c3_strided":
        s, gd = _strided(s), _strided(gd)
    s.requires_grad_()
    M = _M.cuda().requires_grad_()
    out = geometry.warp_perspective(s, M, (33, 47), align_corners=ac, inverse_map=inverse_map)
    assert type(out.grad_fn).__name__ == "_WarpMFnBackward" and len(out.grad_fn.saved_tensors) == 2      # the matrix and the source
    gs, gM = torch.autograd.grad(out, (s, M), gd)
    err = float((gM.double().cpu() - want).abs().max()) / float(want.abs().max())
    print(f"homography_train_parity warp_dM/{layout}/ac{int(ac)}/{'inv' if inverse_map else 'fwd'}map {0.0:.3e} {err:.3e}")
    assert gM.shape == (2, 3, 3) and err <= R.GRAD_BAR
    # without a gradient for M the warp goes through _WarpFn, whose code this feature does not touch, and the source gradient is what it was
    out = geometry.warp_perspective(s, _M.cuda(), (33, 47), align_corners=ac, inverse_map=inverse_map)
    assert type(out.grad_fn).__name__ == "_WarpFnBackward" and len(out.grad_fn.saved_tensors) == 1
    (gs0,) = torch.autograd.grad(out, s, gd)
    sd, A = src.double().requires_grad_(), _M.double() if inverse_map else torch.linalg.inv(_M.double())
    (want_s,) = torch.autograd.grad((R.warp_torch(sd, A, (33, 47), ac) * d_dst.double()).sum(), sd)
    assert float((gs0.double().cpu() - want_s).abs().max()) <= 1e-5 * float(want_s.abs().max())
    assert float((gs.double().cpu() - want_s).abs().max()) <= 1e-5 * float(want_s.abs().max())     # (atomics: not bit-identical run to run)


def test_dlt_backward_matches_fp64_autograd():
    """get_perspective_transform / h_matrix_from_delta backward against fp64 autograd, at the image sizes test_gpu_h_matrix_derivation uses."""
    _, _, corners = synthetic.homography_batch(1, 6)
    delta = torch.from_numpy(np.random.Generator(np.random.PCG64(5)).uniform(-24, 24, (6, 4, 2)).astype(np.float32))
    gH = torch.from_numpy(np.random.Generator(np.random.PCG64(6)).normal(size=(6, 3, 3)).astype(np.float32))
    c0 = corners - corners[:, :1]
    src, dst = c0.double().requires_grad_(), (c0 + delta).double().requires_grad_()
    ws, wd = torch.autograd.grad((R.dlt_torch(src, dst) * gH.double()).sum(), (src, dst))
    s, d = c0.cuda().requires_grad_(), (c0 + delta).cuda().requires_grad_()
    H = homography.get_perspective_transform(s, d)
    assert float((H.detach().cpu().double() - R.dlt_torch(src, dst).detach()).abs().max()) < 1e-5
    gs, gd = torch.autograd.grad(H, (s, d), gH.cuda())
    for tag, got, want in (("d_src", gs, ws), ("d_dst", gd, wd)):
        err = float((got.double().cpu() - want).abs().max()) / float(want.abs().max())
        print(f"homography_train_parity perspective_transform/{tag} {0.0:.3e} {err:.3e}")
        assert err <= R.GRAD_BAR
    (gd_only,) = torch.autograd.grad(homography.get_perspective_transform(c0.cuda(), d), d, gH.cuda())      # the null d_src path
    assert torch.equal(gd_only, gd)
    for (ih, iw, pic, sub) in [(256, 256, 256, True), (512, 512, 256, True), (860, 1080, 256, True), (1, 1, 1, False)]:
        dd = delta.double().requires_grad_()
        (want,) = torch.autograd.grad((R.h_matrix_from_delta_torch(corners.double(), dd, ih, iw, pic, sub) * gH.double()).sum(), dd)
        dg = delta.cuda().requires_grad_()
        (got,) = torch.autograd.grad(homography.h_matrix_from_delta(corners.cuda(), dg, ih, iw, pic, subtract_origin=sub), dg, gH.cuda())
        err = float((got.double().cpu() - want).abs().max()) / float(want.abs().max())
        print(f"homography_train_parity h_matrix_from_delta/{ih}x{iw}/sub{int(sub)} {0.0:.3e} {err:.3e}")
        assert err <= R.GRAD_BAR


@pytest.mark.parametrize("which", [0, 1])
def test_descent_through_the_hip_loss(which):
    """patch_b is img_a sampled at a known homography: Adam on delta through the HIP loss has to find it (the CPU test holds the fp64
    reference to the same bars)."""
    img_a, patch_b, corners, true = R.descent_setup(which)
    a, b, c = img_a.cuda(), patch_b.cuda(), corners.cuda()
    delta = torch.full_like(true, 0.25).cuda().requires_grad_()
    opt = torch.optim.Adam([delta], lr=0.2)
    with _convention(True):
        for _ in range(150):
            opt.zero_grad()
            homography.photometric_loss(delta, a, b, c).backward()
            opt.step()
        loss = float(homography.photometric_loss(delta.detach(), a, b, c))
    err = float((delta.detach().cpu() - true).norm(dim=-1).mean())
    print(f"homography_train_parity descent/{which} corner error {err:.4f} px, loss {loss:.5f}")
    assert err <= 0.25 and loss <= 0.02


def test_multi_block_launches_in_guarded_poisoned_allocations():
    """The multi-block launches once more with every input inside NaN guards and every torch.empty of the wrappers (h, the fp64 partials,
    the loss, the gradients) poisoned: nothing outside a tensor is read into a result, nothing is read before it is written, no guard moves."""
    name = "96_p64_d24"
    (delta, img_a, patch_b, corners), (rl, rg) = _ref(name, True)
    ins = [memguard.guarded(t.cuda(), name=n) for t, n in ((delta, "delta"), (img_a, "img_a"), (patch_b, "patch_b"), (corners, "corners"))]
    with _convention(True), memguard.poisoned_allocations([Fn]):
        d = ins[0].requires_grad_()
        loss = homography.photometric_loss(d, ins[1], ins[2], ins[3])
        (g,) = torch.autograd.grad(loss, d)
    memguard.check_all(ins)
    ok, le, ge = R.within_bars(loss.detach().cpu(), g.cpu(), rl, rg)
    assert ok, (le, ge)
    src, d_dst = R.smooth_images(21, 2, 3, 40, 52), R.smooth_images(22, 2, 3, 33, 47) - 0.5
    want = R.warp_dM_closed(src, _M, d_dst, (33, 47), True, False)
    gin = [memguard.guarded(src.cuda(), name="src"), memguard.guarded(_M.cuda(), name="M"), memguard.guarded(d_dst.cuda(), name="d_dst")]
    with memguard.poisoned_allocations([Fn]):
        M = gin[1].requires_grad_()
        (gM,) = torch.autograd.grad(geometry.warp_perspective(gin[0], M, (33, 47), align_corners=True), M, gin[2])
    memguard.check_all(gin)
    assert float((gM.double().cpu() - want).abs().max()) <= R.GRAD_BAR * float(want.abs().max())

"""MS-SSIM as a training loss, host side: the closed-form backward the device kernel implements (tests/msssim_loss_ref.py) against fp64
autograd of the oracle's ``ms_ssim``, the criterion's definition, and the argument checks of ``rd_loss`` / ``Trainer``.  No GPU."""
import math

import pytest
import torch

import msssim_loss_ref as R
from oracle import hesic_oracle as O


@pytest.mark.parametrize("shape,recipe", [((2, 3, 161, 178), "noise0.2"), ((1, 3, 176, 161), "noise0.05"), ((1, 1, 193, 200), "smooth")])
def test_closed_form_backward_equals_autograd_of_the_oracle(shape, recipe):
    xh, x = R.smooth_pair(3, shape) if recipe == "smooth" else R.noisy_pair(5, shape, float(recipe[5:]))
    go = -torch.linspace(0.5, 1.5, shape[0], dtype=torch.float64)                 # a different weight per image
    ms_ref, g_ref = R.ms_ssim_autograd(xh, x, go)
    ms, g = R.ms_ssim_grad(xh, x, go)
    assert float((ms - ms_ref).abs().max()) <= 1e-12
    assert float(g_ref.abs().max()) > 0
    assert float((g - g_ref).abs().max()) <= 1e-10 * float(g_ref.abs().max())


def test_clamped_factor_gives_a_zero_gradient_for_that_image_only():
    xh, x = R.noisy_pair(11, (2, 3, 161, 170), 0.1)
    x = x.clone()
    x[1] = -xh[1]                                                              # image 1 against its own negative: cs <= 0 at every scale
    ms_ref, g_ref = R.ms_ssim_autograd(xh, x)
    ms, g = R.ms_ssim_grad(xh, x)
    assert float(ms_ref[1]) == 0.0 and float(ms[1]) == 0.0
    assert bool(torch.isfinite(g_ref).all()) and float(g_ref[1].abs().max()) == 0.0 and float(g[1].abs().max()) == 0.0
    _, g0 = R.ms_ssim_autograd(xh[:1], x[:1])
    assert float((g[0] - g0[0]).abs().max()) <= 1e-10 * float(g0.abs().max())


def test_criterion_matches_its_definition():
    gen = torch.Generator().manual_seed(2)
    xh1, x1 = R.noisy_pair(21, (2, 3, 176, 161), 0.1)
    xh2, x2 = R.noisy_pair(22, (2, 3, 176, 161), 0.2)
    xh1 = xh1 + 0.3                                                            # reconstructions are not clamped
    lik = {k: torch.rand(s, generator=gen).clamp_min(1e-3) for k, s in
           (("y1", (2, 8, 11, 11)), ("y2", (2, 8, 11, 11)), ("z1", (2, 4, 3, 3)), ("z2", (2, 4, 3, 3)))}
    out = {"x1_hat": xh1, "x2_hat": xh2, "likelihoods": lik}
    lmbda = 7.5
    c, mse_c = R.rd_loss_ms_ssim(out, x1, x2, lmbda), O.rd_loss(out, x1, x2, lmbda)
    bpp = sum(float(torch.log2(l.double()).sum()) for l in lik.values()) / -(2 * 176 * 161)
    msl = (1 - float(O.ms_ssim(xh1, x1).mean())) + (1 - float(O.ms_ssim(xh2, x2).mean()))
    assert set(c) == {"loss", "bpp_loss", "mse_loss", "ms_ssim_loss"}
    assert float(c["bpp_loss"]) == pytest.approx(bpp, rel=1e-5) and float(c["bpp_loss"]) == float(mse_c["bpp_loss"])
    assert float(c["mse_loss"]) == float(mse_c["mse_loss"])
    assert float(c["ms_ssim_loss"]) == pytest.approx(msl, rel=1e-12)
    assert float(c["loss"]) == pytest.approx(lmbda * msl + bpp, rel=1e-5)          # no 255^2 factor
    assert not math.isclose(float(c["loss"]), float(mse_c["loss"]), rel_tol=1e-2)


def test_rd_loss_refuses_an_unknown_distortion():
    from hesic_amd import functional as Fn
    x = torch.zeros(1, 3, 176, 176)
    out = {"x1_hat": x, "x2_hat": x, "likelihoods": {k: torch.ones(1, 2, 2, 2) for k in ("y1", "y2", "z1", "z2")}}
    with pytest.raises(ValueError, match="distortion"):
        Fn.rd_loss(out, x, x, 0.01, distortion="psnr")


def test_trainer_refuses_an_unknown_distortion():
    from hesic_amd.train import Trainer

    class Tiny(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.w, self.q = torch.nn.Parameter(torch.zeros(4)), torch.nn.Parameter(torch.zeros(2))

        def aux_parameters(self):
            return [self.q]

    with pytest.raises(ValueError, match="distortion"):
        Trainer(Tiny(), distortion="psnr")
    assert Trainer(Tiny()).distortion == "mse" and Trainer(Tiny(), distortion="ms-ssim").distortion == "ms-ssim"


@pytest.mark.parametrize("fmt", ["bf16", "f16"])
def test_both_libraries_export_the_backward_entry_point(fmt):
    """include/hesic_msssim_loss.h (included by hesic_hip.h): declared, bound and exported by both builds; the ABI version stays 2."""
    import os
    import subprocess
    from hesic_amd import _lib as L
    if not os.path.exists(L.LIB_PATH):
        import __graft_entry__ as ge
        ge.build()
    declared = L.declared_symbols("hesic_msssim_loss.h")
    assert declared == ["hesic_ssim_scale_backward"] and set(declared) == set(L._MSSSIM_LOSS_SIGS)
    assert '#include "hesic_msssim_loss.h"' in open(L.header_path("hesic_hip.h")).read()
    l = L.lib(torch.float16 if fmt == "f16" else torch.bfloat16)
    assert l.hesic_abi_version() == 3
    exported = subprocess.check_output(["nm", "-D", "--defined-only", L.LIB_PATH_F16 if fmt == "f16" else L.LIB_PATH], text=True)
    assert " T hesic_ssim_scale_backward\n" in exported
    assert l.hesic_ssim_scale_backward(None, None, None, None, 1, 3, 176, 176, 1.0, None, None, None, 5, 0, None, None, None, None) == -1
    assert b"ssim_scale_backward" in l.hesic_last_error()

"""MS-SSIM as a training loss on the device: ``functional.ms_ssim`` (forward = ``models.ms_ssim``, backward = five launches of
``hesic_ssim_scale_backward``), ``rd_loss(..., distortion="ms-ssim")`` and ``Trainer`` / ``GraphedTrainer(distortion="ms-ssim")``.

The gradient's reference is fp64 autograd of the oracle's ``ms_ssim``.  Its bar is measured, not chosen: the closed-form backward
(tests/msssim_loss_ref.py, pinned against that autograd to 1e-10 on the CPU) is evaluated in fp32 on the CPU as well, e32 = max|g32 - g64|,
and the device gradient must satisfy max|g - g64| <= 8 * e32.  The kernel sums the same 121 fp32 taps and forms E[x^2] - mu^2 in fp32 as
that evaluation does, only in another order; a wrong tap, halo, pool offset or gain shows at 1e-2 or more of the largest entry."""
import functools

import pytest
import torch

import memguard as MG
import msssim_loss_ref as R
from hesic_amd import synthetic
from oracle import hesic_oracle as O

pytestmark = pytest.mark.gpu

BAR = 8.0

# the smallest shapes at which every branch is live: 161 -> 81 -> 41 -> 21 -> 11 (every scale has an odd side, the last a single valid row),
# odd x even and even x odd sides, one and three channels, more than one tile per side and ragged last tiles
SHAPES = {"2x3x161x178": (2, 3, 161, 178), "1x3x176x161": (1, 3, 176, 161), "1x1x193x200": (1, 1, 193, 200)}
RECIPES = ("noise0.05", "noise0.2", "smooth0.03")


def _pair(shape, recipe, seed=0):
    if recipe.startswith("smooth"):
        return R.smooth_pair(100 + seed, shape, float(recipe[6:]))
    return R.noisy_pair(200 + seed, shape, float(recipe[5:]))


def _oracle_factors(xh, x):
    """Per (scale, image, channel) factor relu(mean cs) / relu(mean ssim) from the oracle alone: one-hot exponents leave one factor of the
    product, and channels moved into the batch keep them apart (window and pool act per channel)."""
    N, Cc, H, W = x.shape
    a, b = xh.reshape(N * Cc, 1, H, W), x.reshape(N * Cc, 1, H, W)
    return torch.stack([O.ms_ssim(a, b, weights=tuple(1.0 if i == s else 0.0 for i in range(5))) for s in range(5)])


@functools.lru_cache(maxsize=None)
def _reference(shape_key, recipe):
    """Inputs and the gradient of (1 - MS).sum(): fp64 autograd of the oracle, the restatement in fp32, and their distance e32."""
    xh, x = _pair(SHAPES[shape_key], recipe)
    ms64, g64 = R.ms_ssim_autograd(xh, x, -torch.ones(xh.shape[0], dtype=torch.float64))
    _, g32 = R.ms_ssim_grad(xh, x, -torch.ones(xh.shape[0]), dtype=torch.float32)
    e32 = float((g32.double() - g64).abs().max())
    return xh, x, ms64, g64, e32


def _device_grad(xh, x):
    from hesic_amd import functional as Fn
    xh = xh.detach().requires_grad_(True)
    ms = Fn.ms_ssim(xh, x)
    (1 - ms).sum().backward()
    return ms.detach(), xh.grad


def _check_grad(g, g64, e32, what):
    err, top = float((g.double().cpu() - g64).abs().max()), float(g64.abs().max())
    print(f"{what}: max|g - g64| = {err:.3e}  e32 = {e32:.3e}  ratio = {err / e32:.2f}  (max|g64| = {top:.3e}, e32 / max = {e32 / top:.1e})")
    assert g.dtype == torch.float32 and bool(torch.isfinite(g).all())
    assert err <= BAR * e32, (what, err, e32, err / e32)


def test_forward_is_the_metric():
    from hesic_amd import functional as Fn, models
    xh, x, ms64, _, _ = _reference("2x3x161x178", "noise0.2")
    a, b = xh.cuda(), x.cuda()
    got = Fn.ms_ssim(a.clone().requires_grad_(True), b)
    assert got.dtype == torch.float64 and got.shape == (2,) and got.requires_grad
    assert torch.equal(got.detach(), models.ms_ssim(a, b))
    with torch.no_grad():
        assert torch.equal(Fn.ms_ssim(a, b), got.detach())
    assert float((got.detach().cpu() - ms64).abs().max()) <= 5e-6               # the bound of tests/test_msssim.py
    with pytest.raises(ValueError, match="160"):
        Fn.ms_ssim(a[..., :160, :], b[..., :160, :])


@pytest.mark.parametrize("recipe", RECIPES)
@pytest.mark.parametrize("shape_key", list(SHAPES))
def test_gradient_against_fp64_autograd_of_the_oracle(shape_key, recipe):
    xh, x, ms64, g64, e32 = _reference(shape_key, recipe)
    fac = _oracle_factors(xh, x)
    print(f"smallest per-scale factor {float(fac.min()):.3f}")
    assert float(fac.min()) > 0.5                                            # no clamp in play: it could hide an error
    ms, g = _device_grad(xh.cuda(), x.cuda())
    assert float((ms.cpu() - ms64).abs().max()) <= 5e-6
    assert g.shape == xh.shape and g.is_contiguous()
    _check_grad(g, g64, e32, f"{shape_key} {recipe}")


def test_gradient_with_a_channels_last_reconstruction():
    xh, x, _, g64, e32 = _reference("1x3x176x161", "noise0.05")
    _, g = _device_grad(xh.cuda().contiguous(memory_format=torch.channels_last), x.cuda())
    _check_grad(g, g64, e32, "channels-last x_hat")


def test_gradient_with_the_target_a_crop_of_a_larger_tensor():
    xh, x, _, g64, e32 = _reference("2x3x161x178", "smooth0.03")
    big = torch.full((2, 3, 161 + 20, 178 + 30), float("nan"))
    big[:, :, 7:7 + 161, 11:11 + 178] = x
    _, g = _device_grad(xh.cuda(), big.cuda()[:, :, 7:7 + 161, 11:11 + 178])
    _check_grad(g, g64, e32, "cropped target")


def test_16_bit_reconstruction_is_cast_like_the_metric():
    from hesic_amd import functional as Fn, models
    xh, x, _, _, _ = _reference("1x3x176x161", "noise0.05")
    a = xh.cuda().bfloat16().requires_grad_(True)
    ms = Fn.ms_ssim(a, x.cuda())
    assert torch.equal(ms.detach(), models.ms_ssim(a.detach(), x.cuda()))
    (1 - ms).sum().backward()
    _, g64 = R.ms_ssim_autograd(a.detach().float().cpu(), x, -torch.ones(1, dtype=torch.float64))
    # the gradient autograd hands a bf16 leaf is rounded to bf16: 2^-9 relative per element on top of the fp32 kernel's error
    assert a.grad.shape == a.shape and float((a.grad.double().cpu() - g64).abs().max()) <= 2.0 ** -8 * float(g64.abs().max())


def test_memory_guards_inputs_and_poisoned_allocations():
    """NaN-guarded inputs (the target a crop: the gaps between its rows are guards too) and poisoned allocations: every gradient element
    is written, nothing outside the views is read or written."""
    import hesic_amd.functional as Fn
    xh, x, _, g64, e32 = _reference("2x3x161x178", "noise0.05")
    big = torch.zeros((2, 3, 161 + 9, 178 + 13))
    big[:, :, 4:4 + 161, 6:6 + 178] = x
    a = MG.guarded(xh.cuda().requires_grad_(True), name="x_hat")
    b = MG.guarded(big.cuda()[:, :, 4:4 + 161, 6:6 + 178], name="x")
    with MG.poisoned_allocations([Fn]) as record:
        ms = Fn.ms_ssim(a, b)
        (1 - ms).sum().backward()
        torch.cuda.synchronize()
    assert len(record) >= 1 + 8 + 5                                          # the sums, eight pooled images, one gradient per scale
    MG.check_all([a, b])
    assert bool(torch.isfinite(a.grad).all()) and bool(torch.isfinite(ms).all())
    _check_grad(a.grad, g64, e32, "guarded")


def test_clamped_image_has_value_zero_and_a_zero_gradient():
    xh, x, _, g64, e32 = _reference("2x3x161x178", "noise0.05")
    x = x.clone()
    x[1] = -xh[1] + 0.01 * torch.randn(xh[1].shape, generator=torch.Generator().manual_seed(9))      # image 1 against its own negative, plus noise
    ms64, g64b = R.ms_ssim_autograd(xh, x, -torch.ones(2, dtype=torch.float64))
    assert float(ms64[1]) == 0.0 and float(g64b[1].abs().max()) == 0.0          # what autograd of the oracle gives
    ms, g = _device_grad(xh.cuda(), x.cuda())
    assert float(ms[1]) == 0.0
    assert bool(torch.isfinite(g).all()) and float(g[1].abs().max()) == 0.0
    assert float(abs(ms[0].cpu() - ms64[0])) <= 5e-6
    _check_grad(g[:1], g64[:1], e32, "image 0 next to a clamped image")      # as when computed alone


def _hand_made_out(seed=0):
    gen = torch.Generator().manual_seed(40 + seed)
    xh1, x1 = R.noisy_pair(41, (2, 3, 192, 192), 0.05)
    xh2, x2 = R.noisy_pair(42, (2, 3, 192, 192), 0.2)
    lik = {k: 1 - 0.999 * torch.rand(s, generator=gen) for k, s in
           (("y1", (2, 192, 12, 12)), ("y2", (2, 192, 12, 12)), ("z1", (2, 128, 3, 3)), ("z2", (2, 128, 3, 3)))}
    return xh1, x1, xh2, x2, lik


def _on_device(xh1, xh2, lik):
    return {"x1_hat": xh1.cuda().requires_grad_(True), "x2_hat": xh2.cuda().requires_grad_(True),
            "likelihoods": {k: v.cuda().requires_grad_(True) for k, v in lik.items()}}


def test_rd_loss_with_ms_ssim_distortion():
    from hesic_amd import functional as Fn
    xh1, x1, xh2, x2, lik = _hand_made_out()
    lmbda, N = 8.73, 2
    d1, d2 = x1.cuda(), x2.cuda()
    out, out_mse, out3 = (_on_device(xh1, xh2, lik) for _ in range(3))
    c = Fn.rd_loss(out, d1, d2, lmbda, distortion="ms-ssim")
    m = Fn.rd_loss(out_mse, d1, d2, lmbda)
    assert set(c) == {"loss", "bpp_loss", "mse_loss", "ms_ssim_loss"} and set(m) == {"loss", "bpp_loss", "mse_loss"}
    for k in ("bpp_loss", "mse_loss"):            # the same fused reduction: fp64 atomics in another order, then one rounding to fp32
        assert float(c[k]) == pytest.approx(float(m[k]), rel=2e-7), k
    msl = (1 - float(O.ms_ssim(xh1, x1).mean())) + (1 - float(O.ms_ssim(xh2, x2).mean()))
    assert float(c["ms_ssim_loss"]) == pytest.approx(msl, abs=2 * 5e-6)
    assert float(c["loss"].detach()) == pytest.approx(lmbda * float(c["ms_ssim_loss"]) + float(c["bpp_loss"]), rel=1e-6)       # no 255^2 factor
    assert not c["bpp_loss"].requires_grad and not c["ms_ssim_loss"].requires_grad
    c["loss"].backward()
    m["loss"].backward()
    for k in lik:                                                            # the bpp part is the MSE criterion's
        assert torch.equal(out["likelihoods"][k].grad, out_mse["likelihoods"][k].grad), k
    c3 = Fn.rd_loss(out3, d1, d2, lmbda, distortion="ms-ssim")
    (3 * c3["loss"]).backward()                                              # a scaled loss scales every gradient
    for key, xh, x in (("x1_hat", xh1, x1), ("x2_hat", xh2, x2)):
        _, g64 = R.ms_ssim_autograd(xh, x, -torch.ones(N, dtype=torch.float64))
        _, g32 = R.ms_ssim_grad(xh, x, -torch.ones(N), dtype=torch.float32)
        e32 = float((g32.double() - g64).abs().max())
        _check_grad(out[key].grad, lmbda / N * g64, lmbda / N * e32, f"rd_loss {key}")
        # the factor goes into the fp64 gain of the scale, so the scaled gradient is another fp32 evaluation: the same bar, scaled
        _check_grad(out3[key].grad, 3 * lmbda / N * g64, 3 * lmbda / N * e32, f"rd_loss {key}, loss x 3")
    for k in lik:                                                            # one more multiply of the same values
        torch.testing.assert_close(out3["likelihoods"][k].grad, 3 * out["likelihoods"][k].grad, rtol=1e-6, atol=0)
    with pytest.raises(ValueError, match="distortion"):
        Fn.rd_loss(out, d1, d2, lmbda, distortion="psnr")
    with pytest.raises(ValueError, match="160"):
        Fn.rd_loss({"x1_hat": out["x1_hat"][..., :128, :128], "x2_hat": out["x2_hat"][..., :128, :128], "likelihoods": out["likelihoods"]},
                   d1[..., :128, :128], d2[..., :128, :128], lmbda, distortion="ms-ssim")


# ------------------------------------------------------------------------------------------------ trainers
LMBDA_MS = 31.73


def _noise_for(step):
    shp = {"z1": (2, 128, 3, 3), "z2": (2, 128, 3, 3)}
    return {k: synthetic._uniform(f"msl.noise.{step}.{k}", shp.get(k, (2, 192, 12, 12)), -0.5, 0.5).cuda()
            for k in ("z1", "y1", "y1b", "y1w", "z2", "y2", "y2b")}


def _run(cls, steps, **kw):
    from hesic_amd import models
    x1, x2, Hm = (t.cuda() for t in synthetic.stereo_batch(0, 2, 192, 192))
    net = models.HSIC()
    synthetic.fill_state_dict_(net.state_dict())
    tr = cls(net.cuda(), lr=1e-4, aux_lr=1e-3, **kw)
    trace = []
    for step in range(steps):
        c = tr.step(x1, x2, Hm, noise=_noise_for(step))
        trace.append({k: float(v) for k, v in c.items()})
    return tr, trace


@pytest.fixture
def bf16():
    import hesic_amd
    prev = hesic_amd.functional.compute_dtype()
    hesic_amd.set_compute_dtype(torch.bfloat16)
    yield
    hesic_amd.set_compute_dtype(prev)


def test_trainers_with_ms_ssim_distortion(bf16):
    from hesic_amd.train import Trainer, GraphedTrainer
    _, eager = _run(Trainer, 5, lmbda=LMBDA_MS, distortion="ms-ssim")
    tr, graphed = _run(GraphedTrainer, 3, lmbda=LMBDA_MS, distortion="ms-ssim", warmup=2)
    assert tr.graph is not None                                               # the step with MS-SSIM forward and backward was captured
    x1, x2, Hm = (t.cuda() for t in synthetic.stereo_batch(0, 2, 192, 192))
    for step in (3, 4):
        graphed.append({k: float(v) for k, v in tr.step(x1, x2, Hm, noise=_noise_for(step)).items()})
    assert set(eager[0]) == {"loss", "bpp_loss", "mse_loss", "ms_ssim_loss", "aux_loss"}
    for a, b in zip(eager, graphed):
        for k in a:
            assert a[k] == pytest.approx(b[k], rel=2e-3), (k, eager, graphed)      # test_graphed_trainer_follows_the_eager_trace's HESIC tolerance
        assert a["loss"] == pytest.approx(LMBDA_MS * a["ms_ssim_loss"] + a["bpp_loss"], rel=1e-5)
    print("ms_ssim_loss per step:", [round(t["ms_ssim_loss"], 5) for t in eager], [round(t["ms_ssim_loss"], 5) for t in graphed])
    assert eager[4]["ms_ssim_loss"] < eager[0]["ms_ssim_loss"] and graphed[4]["ms_ssim_loss"] < graphed[0]["ms_ssim_loss"]


def test_default_trainer_is_the_mse_trainer(bf16):
    from hesic_amd.train import Trainer
    tr, default = _run(Trainer, 3, lmbda=0.0067)
    _, mse = _run(Trainer, 3, lmbda=0.0067, distortion="mse")
    assert tr.distortion == "mse"
    for a, b in zip(default, mse):
        assert set(a) == set(b) == {"loss", "bpp_loss", "mse_loss", "aux_loss"}       # no "ms_ssim_loss"
        for k in a:
            # two runs of the same code: bf16 + atomics are not bit-stable from run to run (eager reruns agree to 4-5 digits)
            assert a[k] == pytest.approx(b[k], rel=1e-3), (k, default, mse)
        assert a["loss"] == pytest.approx(0.0067 * 255 ** 2 * a["mse_loss"] + a["bpp_loss"], rel=1e-5)


def test_ms_ssim_trainers_refuse_small_images_on_the_host(bf16):
    from hesic_amd import models
    from hesic_amd.train import Trainer, GraphedTrainer
    from hesic_amd import _lib as L
    net = models.HSIC()
    synthetic.fill_state_dict_(net.state_dict())
    net = net.cuda()
    x1, x2, Hm = (t.cuda() for t in synthetic.stereo_batch(0, 2, 128, 128))
    for cls in (Trainer, GraphedTrainer):
        tr = cls(net, lmbda=LMBDA_MS, distortion="ms-ssim")
        launches = []
        with L.call_hook(lambda name, args: launches.append(name)):
            with pytest.raises(ValueError, match="160"):
                tr.step(x1, x2, Hm)
        assert not launches                                                  # refused before anything was launched
        tr.main_reducer.close(); tr.aux_reducer.close()
    with pytest.raises(ValueError, match="distortion"):
        Trainer(net, distortion="psnr")

"""MS-SSIM as a training loss, restated without autograd: the closed-form backward that ``csrc/msssim.hip::ssim_scale_backward_kernel``
implements, and the R-D criterion built on it.  The forward is ``oracle.hesic_oracle.ms_ssim`` (the definition); this module adds

- ``ms_ssim_grad(x_hat, x, grad_out, dtype)``: value and d(sum_n grad_out[n] * MS[n]) / d x_hat through per-position coefficient maps, the
  transposed ("full") separable window and the 2 x 2 pool's adjoint -- in ``dtype`` (fp64: pinned against autograd of the oracle by
  tests/test_msssim_loss_cpu.py; fp32: the arithmetic the kernel does, which gives the GPU tests their error bar);
- ``rd_loss_ms_ssim(out, x1, x2, lmbda)``: ``lmbda * ((1 - mean MS(x1_hat, x1)) + (1 - mean MS(x2_hat, x2))) + bpp_loss``.

Per scale, with m = (mu_x, mu_y, E[xx], E[yy], E[xy]) the window means at a valid position (x differentiated, y the target),
D1 = mu_x^2 + mu_y^2 + C1, D2 = s_x^2 + s_y^2 + C2, l = (2 mu_x mu_y + C1) / D1:
    d cs / d Exy = 2 / D2        d cs / d Exx = -cs / D2        d cs / d mu_x = (2 / D2) (cs mu_x - mu_y)
    ssim = l cs: the three above times l, plus cs (2 mu_y - 2 mu_x l) / D1 on the mu_x coefficient
    dL/dx(q) = (G^T a_mu)(q) + 2 x(q) (G^T a_xx)(q) + y(q) (G^T a_xy)(q) + 0.25 * (dL/dx of the next coarser scale at q's pool cell)
where a_* are the coefficients times the scale's gain  grad_out[n] / C * w_s * MS_c / v_s / count_s  (0 where any v <= 0)."""
import math

import torch
import torch.nn.functional as F

from oracle import hesic_oracle as O

WIN, SIGMA = 11, 1.5


def window(dtype):
    co = torch.arange(WIN, dtype=torch.float32) - WIN // 2
    g = torch.exp(-(co ** 2) / (2 * SIGMA ** 2))
    return (g / g.sum()).to(dtype)


def _blur(t, g, transpose=False):
    ch = t.shape[1]
    wh, wv = g.reshape(1, 1, 1, -1).repeat(ch, 1, 1, 1), g.reshape(1, 1, -1, 1).repeat(ch, 1, 1, 1)
    if transpose:
        return F.conv_transpose2d(F.conv_transpose2d(t, wv, groups=ch), wh, groups=ch)
    return F.conv2d(F.conv2d(t, wh, groups=ch), wv, groups=ch)


def _pool(t):
    return F.avg_pool2d(t, 2, padding=[s % 2 for s in t.shape[2:]])


def _pool_adjoint(gc, H, W):
    """Gradient a fine H x W image receives from its pooled image's gradient ``gc``: 0.25 x the cell of every pixel (padding offsets)."""
    up = gc.repeat_interleave(2, -2).repeat_interleave(2, -1)
    return 0.25 * up[..., H % 2:H % 2 + H, W % 2:W % 2 + W]


@torch.no_grad()
def ms_ssim_grad(x_hat, x, grad_out=None, dtype=torch.float64, data_range=1.0, weights=O.MS_SSIM_WEIGHTS, return_factors=False):
    """(MS (N,), gradient of sum_n grad_out[n] * MS[n] with respect to x_hat), both in ``dtype``; grad_out defaults to ones."""
    a, b = x_hat.detach().to(dtype), x.detach().to(dtype)
    N, Cc = a.shape[:2]
    g = window(dtype)
    C1, C2 = (0.01 * data_range) ** 2, (0.03 * data_range) ** 2
    go = torch.ones(N, dtype=dtype) if grad_out is None else grad_out.to(dtype)
    levels, v = [], []
    for s in range(len(weights)):
        mx, my = _blur(a, g), _blur(b, g)
        exx, eyy, exy = _blur(a * a, g), _blur(b * b, g), _blur(a * b, g)
        D2 = (exx - mx * mx) + (eyy - my * my) + C2
        D1 = mx * mx + my * my + C1
        cs = (2 * (exy - mx * my) + C2) / D2
        l = (2 * mx * my + C1) / D1
        c_xy, c_xx, c_mu = 2 / D2, -cs / D2, (2 / D2) * (cs * mx - my)
        if s == len(weights) - 1:
            c_xy, c_xx, c_mu = c_xy * l, c_xx * l, c_mu * l + cs * (2 * my - 2 * mx * l) / D1
            v.append((l * cs).flatten(2).mean(-1))
        else:
            v.append(cs.flatten(2).mean(-1))
        levels.append((a, b, c_mu, c_xx, c_xy))
        if s < len(weights) - 1:
            a, b = _pool(a), _pool(b)
    v = torch.stack(v, 0)                                                       # (levels, N, C) before the clamp
    live = (v > 0).all(0)                                                       # a factor <= 0 zeroes the product and every gradient
    vc = v.clamp_min(0)
    w = torch.tensor(weights, dtype=dtype).reshape(-1, 1, 1)
    ms_c = torch.prod(vc ** w, 0)                                               # (N, C)
    grad = None
    for s in reversed(range(len(weights))):
        a, b, c_mu, c_xx, c_xy = levels[s]
        count = c_mu.shape[-2] * c_mu.shape[-1]
        gain = torch.where(live, go.reshape(-1, 1) / Cc * weights[s] * ms_c / torch.where(live, v[s], torch.ones_like(v[s])) / count,
                           torch.zeros_like(ms_c)).reshape(N, Cc, 1, 1)
        gs = _blur(c_mu * gain, g, True) + 2 * a * _blur(c_xx * gain, g, True) + b * _blur(c_xy * gain, g, True)
        if grad is not None:
            gs = gs + _pool_adjoint(grad, a.shape[-2], a.shape[-1])
        grad = gs
    if return_factors:
        return ms_c.mean(1), grad, vc
    return ms_c.mean(1), grad


def ms_ssim_autograd(x_hat, x, grad_out=None):
    """fp64 autograd of the oracle: (MS (N,), d(sum_n grad_out[n] MS[n]) / d x_hat)."""
    xh = x_hat.detach().double().requires_grad_(True)
    ms = O.ms_ssim(xh, x.detach().double())
    go = torch.ones_like(ms) if grad_out is None else grad_out.double()
    (grad,) = torch.autograd.grad((ms * go).sum(), xh)
    return ms.detach(), grad


def rd_loss_ms_ssim(out, x1, x2, lmbda):
    """The MS-SSIM criterion: bpp_loss and mse_loss as ``oracle.rd_loss`` reports them, no 255^2 factor, reconstructions not clamped."""
    n, _, h, w = x1.shape
    bpp = sum(torch.log(l).sum() / (-math.log(2) * n * h * w) for l in out["likelihoods"].values())
    mse = F.mse_loss(out["x1_hat"], x1) + F.mse_loss(out["x2_hat"], x2)
    msl = (1 - O.ms_ssim(out["x1_hat"], x1).mean()) + (1 - O.ms_ssim(out["x2_hat"], x2).mean())
    return {"bpp_loss": bpp, "mse_loss": mse, "ms_ssim_loss": msl, "loss": lmbda * msl + bpp}


# ------------------------------------------------------------------------------ the inputs of the gradient tests
def noisy_pair(seed, shape, sigma):
    """x = rand, x_hat = clamp(x + sigma * randn, 0, 1)."""
    gen = torch.Generator().manual_seed(seed)
    x = torch.rand(shape, generator=gen)
    return (x + sigma * torch.randn(shape, generator=gen)).clamp(0, 1), x


def smooth_pair(seed, shape, sigma=0.03):
    """A smooth target (bilinear x 8 of a coarse random field) and x_hat = clamp(x + sigma * randn, 0, 1)."""
    gen = torch.Generator().manual_seed(seed)
    N, Cc, H, W = shape
    coarse = torch.rand((N, Cc, -(-H // 8) + 1, -(-W // 8) + 1), generator=gen)
    x = F.interpolate(coarse, scale_factor=8, mode="bilinear", align_corners=False)[..., :H, :W].contiguous()
    return (x + sigma * torch.randn(shape, generator=gen)).clamp(0, 1), x

"""fp64 reference of the differentiable homography geometry (include/hesic_homography_train.h): the photometric loss of
ywz/mywork/model.py:18-45 with its closed-form gradient to the corner deltas, d(warp_perspective)/dM, and the DLT adjoint.  No GPU.

Two independent statements of the same thing live here: ``*_torch`` builds the value from differentiable torch ops (``linalg.solve``,
``grid_sample``) so that autograd supplies the gradient, at any dtype; ``*_closed`` spells the chain rule out as the kernels do.  The CPU
tests pin one against the other (and against the oracle and central differences); the GPU tests compare the kernels with the closed form.
``mutate=...`` breaks the closed form in one named way: the bars used on the GPU have to reject every one of them."""
import numpy as np
import torch
import torch.nn.functional as F

LOSS_BAR = 1e-6          # |loss - ref| <= LOSS_BAR * max(1, |ref|)
GRAD_BAR = 2e-5          # max |g - ref| <= GRAD_BAR * max |ref|

MUTATIONS = ("sign", "no_mean", "zero_h2", "transposed_adjoint", "no_origin_shift", "drop_ac_factor", "outside_tap")


def within_bars(loss, grad, ref_loss, ref_grad):
    """(ok, loss error / bar unit, grad error / max|g|)."""
    le = abs(float(loss) - float(ref_loss)) / max(1.0, abs(float(ref_loss)))
    ge = float((grad.double() - ref_grad.double()).abs().max()) / float(ref_grad.double().abs().max())
    return (le <= LOSS_BAR and ge <= GRAD_BAR), le, ge


# ------------------------------------------------------------------------------------------------------------------ inputs
def smooth_images(seed, B, C, H, W):
    """Sums of six sinusoids with |frequency| <= 0.25 rad/px (PCG64): smooth enough that a bilinear tap flipping at an integer coordinate
    changes the gradient negligibly, so fp32 against fp64 is well-conditioned.  (B,C,H,W) fp32 in about [0,1]."""
    r = np.random.Generator(np.random.PCG64(seed))
    ys, xs = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    out = np.full((B, C, H, W), 0.5)
    for b in range(B):
        for c in range(C):
            for _ in range(6):
                fx, fy, ph = r.uniform(-0.25, 0.25), r.uniform(-0.25, 0.25), r.uniform(0, 2 * np.pi)
                out[b, c] += r.uniform(0.04, 0.08) * np.sin(fx * xs + fy * ys + ph)
    return torch.from_numpy(out.astype(np.float32))


def box_corners(tl, ph, pw):
    """(B,4,2) corners (top-left, top-right, bottom-right, bottom-left) of a ph x pw patch whose top-left is ``tl`` (B,2)."""
    box = torch.tensor([[0.0, 0.0], [pw, 0.0], [pw, ph], [0.0, ph]])
    return torch.as_tensor(tl, dtype=torch.float32).view(-1, 1, 2) + box


def deltas(seed, B, amp):
    """Non-integer corner offsets, uniform in [-amp, amp]."""
    r = np.random.Generator(np.random.PCG64(seed))
    return torch.from_numpy(r.uniform(-amp, amp, (B, 4, 2)).astype(np.float32))


# --------------------------------------------------------------------------------------------------------------------- DLT
def dlt_system(src, dst):
    """The 8x8 system of the 4-point DLT with h22 = 1: rows [x y 1 0 0 0 -xu -yu | u], [0 0 0 x y 1 -xv -yv | v]."""
    x, y, u, v = src[..., 0], src[..., 1], dst[..., 0], dst[..., 1]
    z, o = torch.zeros_like(x), torch.ones_like(x)
    r0 = torch.stack([x, y, o, z, z, z, -x * u, -y * u], -1)
    r1 = torch.stack([z, z, z, x, y, o, -x * v, -y * v], -1)
    A = torch.stack([r0, r1], 2).reshape(src.shape[0], 8, 8)
    rhs = torch.stack([u, v], 2).reshape(src.shape[0], 8)
    return A, rhs


def dlt_torch(src, dst):
    """(B,3,3) with dst ~ H src, differentiable, in the dtype of its inputs."""
    A, rhs = dlt_system(src, dst)
    h = torch.linalg.solve(A, rhs.unsqueeze(-1)).squeeze(-1)
    return torch.cat([h, torch.ones_like(h[:, :1])], 1).view(-1, 3, 3)


def dlt_adjoint_closed(src, dst, g8, transposed=False):
    """(d_src, d_dst) from the gradient g8 (B,8) of h[0..7]: lambda = A^-T g, d rhs = lambda, dA = -lambda h^T mapped onto the points."""
    A, rhs = dlt_system(src, dst)
    h = torch.linalg.solve(A, rhs.unsqueeze(-1)).squeeze(-1)
    lam = torch.linalg.solve(A if transposed else A.transpose(1, 2), g8.unsqueeze(-1)).squeeze(-1)
    l0, l1 = lam[:, 0::2], lam[:, 1::2]
    x, y, u, v = src[..., 0], src[..., 1], dst[..., 0], dst[..., 1]
    hh = [h[:, k:k + 1] for k in range(8)]
    w = 1.0 + hh[6] * x + hh[7] * y
    d_dst = torch.stack([l0 * w, l1 * w], -1)
    d_src = torch.stack([-l0 * (hh[0] - hh[6] * u) - l1 * (hh[3] - hh[6] * v), -l0 * (hh[1] - hh[7] * u) - l1 * (hh[4] - hh[7] * v)], -1)
    return d_src, d_dst


def inverse_adjoint_closed(m, g):
    """Gradient of a matrix from the gradient ``g`` of its inverse ``m``: -m^T g m^T."""
    return -m.transpose(1, 2) @ g @ m.transpose(1, 2)


def h_adjust(h, a, b):
    """newtrain1_real.py:47-57 out of place: entry (r, c) times rs[r] * cs[c], rs = (a, b, 1), cs = (1/a, 1/b, 1)."""
    rs = torch.tensor([a, b, 1.0], dtype=h.dtype).view(1, 3, 1)
    cs = torch.tensor([1.0 / a, 1.0 / b, 1.0], dtype=h.dtype).view(1, 1, 3)
    return h * rs * cs


def h_matrix_from_delta_torch(corners, delta, img_h, img_w, pic_size, subtract_origin=True):
    c0 = corners - corners[:, :1] if subtract_origin else corners
    return h_adjust(torch.linalg.inv(dlt_torch(c0, c0 + delta)), img_h / pic_size, img_w / pic_size)


def h_matrix_from_delta_grad_closed(corners, delta, img_h, img_w, pic_size, gH, subtract_origin=True):
    """d_delta from the gradient gH (B,3,3) of the h_matrix: h_adjust, the 3x3 inverse, the DLT adjoint."""
    c0 = corners - corners[:, :1] if subtract_origin else corners
    hi = torch.linalg.inv(dlt_torch(c0, c0 + delta))
    gh = inverse_adjoint_closed(hi, h_adjust(gH, img_h / pic_size, img_w / pic_size))
    return dlt_adjoint_closed(c0, c0 + delta, gh.reshape(-1, 9)[:, :8])[1]


# ---------------------------------------------------------------------------------------------------------------- sampling
def _pixel_grid(Ho, Wo, dtype):
    ys, xs = torch.meshgrid(torch.arange(Ho, dtype=dtype), torch.arange(Wo, dtype=dtype), indexing="ij")
    return xs, ys


def warp_torch(src, A, dsize, align_corners):
    """dst(p) = bilinear(src, A p), zeros outside: ``A`` (B,3,3) maps destination pixels to source pixels.  grid_sample in src's dtype."""
    B, C, H, W = src.shape
    xs, ys = _pixel_grid(dsize[0], dsize[1], src.dtype)
    p = torch.stack([xs, ys, torch.ones_like(xs)], 0).reshape(1, 3, -1)
    s = A.to(src.dtype) @ p
    sx, sy = (s[:, 0] / s[:, 2]).reshape(B, *dsize), (s[:, 1] / s[:, 2]).reshape(B, *dsize)
    grid = torch.stack([2.0 * sx / (W - 1) - 1.0, 2.0 * sy / (H - 1) - 1.0], -1)
    return F.grid_sample(src, grid, mode="bilinear", padding_mode="zeros", align_corners=align_corners)


def _taps(src, A, dsize, align_corners, clamp_outside=False):
    """Per-pixel pieces of the closed form: the four taps (zero outside the image), the weights, x = X/Z, y = Y/Z, 1/Z, kx, ky."""
    B, C, H, W = src.shape
    xs, ys = _pixel_grid(dsize[0], dsize[1], src.dtype)
    X = A[:, 0, 0, None, None] * xs + A[:, 0, 1, None, None] * ys + A[:, 0, 2, None, None]
    Y = A[:, 1, 0, None, None] * xs + A[:, 1, 1, None, None] * ys + A[:, 1, 2, None, None]
    Z = A[:, 2, 0, None, None] * xs + A[:, 2, 1, None, None] * ys + A[:, 2, 2, None, None]
    x, y = X / Z, Y / Z
    kx, ky = (1.0, 1.0) if align_corners else (W / (W - 1), H / (H - 1))
    sx, sy = (x, y) if align_corners else (x * kx - 0.5, y * ky - 0.5)
    x0, y0 = torch.floor(sx), torch.floor(sy)
    wx1, wy1 = (sx - x0).unsqueeze(1), (sy - y0).unsqueeze(1)

    def tap(yy, xx):
        ok = ((xx >= 0) & (xx < W) & (yy >= 0) & (yy < H)).unsqueeze(1)
        idx = (yy.clamp(0, H - 1) * W + xx.clamp(0, W - 1)).long().view(B, 1, -1).expand(B, C, -1)
        v = src.reshape(B, C, -1).gather(2, idx).view(B, C, *dsize)
        return v if clamp_outside else v * ok
    return (tap(y0, x0), tap(y0, x0 + 1), tap(y0 + 1, x0), tap(y0 + 1, x0 + 1)), (1 - wx1, wx1, 1 - wy1, wy1), (x, y, 1.0 / Z, xs, ys, kx, ky)


def matrix_grad_closed(src, A, g, dsize, align_corners, drop_ac_factor=False, clamp_outside=False):
    """(value, dA): dst = bilinear(src, A p) and the gradient of sum(g * dst) with respect to the destination -> source matrix A."""
    (i00, i01, i10, i11), (wx0, wx1, wy0, wy1), (x, y, rz, xs, ys, kx, ky) = _taps(src, A, dsize, align_corners)
    val = i00 * wx0 * wy0 + i01 * wx1 * wy0 + i10 * wx0 * wy1 + i11 * wx1 * wy1
    if g is None:
        return val, None
    if clamp_outside:
        (i00, i01, i10, i11) = _taps(src, A, dsize, align_corners, clamp_outside=True)[0]
    if drop_ac_factor:
        kx = ky = 1.0
    gx = (g * (wy0 * (i01 - i00) + wy1 * (i11 - i10))).sum(1) * kx
    gy = (g * (wx0 * (i10 - i00) + wx1 * (i11 - i01))).sum(1) * ky
    t = [gx * rz, gy * rz, -(gx * x + gy * y) * rz]
    dA = torch.stack([(tk * pj).sum((1, 2)) for tk in t for pj in (xs, ys, torch.ones_like(xs))], 1).view(-1, 3, 3)
    return val, dA


def warp_dM_closed(src, M, d_dst, dsize, align_corners, inverse_map):
    """dM of warp_perspective(src, M, dsize): through the inverse unless ``M`` already maps destination to source."""
    src, M, d_dst = src.double(), M.double(), d_dst.double()
    A = M if inverse_map else torch.linalg.inv(M)
    dA = matrix_grad_closed(src, A, d_dst, dsize, align_corners)[1]
    return dA if inverse_map else inverse_adjoint_closed(A, dA)


# --------------------------------------------------------------------------------------------------------- photometric loss
def photometric_torch(delta, img_a, patch_b, corners, align_corners=True, dtype=torch.float64):
    """model.py:18-45 from differentiable torch ops in ``dtype`` (fp64: the reference value; fp32: the noise floor of a plain evaluation)."""
    delta, img_a, patch_b, corners = delta.to(dtype), img_a.to(dtype), patch_b.to(dtype), corners.to(dtype)
    h = dlt_torch(corners - corners[:, :1], corners + delta)
    return (warp_torch(img_a, h, patch_b.shape[-2:], align_corners) - patch_b).abs().mean()


def photometric_closed(delta, img_a, patch_b, corners, align_corners=True, mutate=None):
    """(loss, d_delta) in fp64 from the chain rule as the kernels apply it.  ``mutate``: one of MUTATIONS."""
    assert mutate is None or mutate in MUTATIONS
    delta, img_a, patch_b, corners = delta.double(), img_a.double(), patch_b.double(), corners.double()
    c0 = corners if mutate == "no_origin_shift" else corners - corners[:, :1]
    dst = corners + delta
    h = dlt_torch(c0, dst)
    dsize = patch_b.shape[-2:]
    val = matrix_grad_closed(img_a, h, None, dsize, align_corners)[0]
    diff = val - patch_b
    loss = diff.abs().mean()
    g = torch.sign(diff) / (1.0 if mutate == "no_mean" else diff.numel())
    dh = matrix_grad_closed(img_a, h, g, dsize, align_corners, drop_ac_factor=mutate == "drop_ac_factor",
                            clamp_outside=mutate == "outside_tap")[1].reshape(-1, 9)[:, :8].clone()
    if mutate == "zero_h2":
        dh[:, 6:] = 0.0
    d_delta = dlt_adjoint_closed(c0, dst, dh, transposed=mutate == "transposed_adjoint")[1]
    return loss, (-d_delta if mutate == "sign" else d_delta)


# the GPU stage-1 shapes: name -> (B, C, image H, W, patch h, w, patch top-left, |delta|, seed); the first is the
# strided three-channel case (the GPU test hands its images over as non-contiguous views)
STAGE1_CASES = {
    "c3_40x52_p21x35": (2, 3, 40, 52, 21, 35, (8.0, 9.0), 4.0, 0),
    "tails_40x52_p21x35": (3, 1, 40, 52, 21, 35, (9.0, 8.0), 4.0, 0),
    "96_p64_d24": (2, 1, 96, 96, 64, 64, (16.0, 16.0), 24.0, 30),
    "corner_64_p32": (2, 1, 64, 64, 32, 32, (0.0, 0.0), 6.0, 0),
    "real_256_p128_d32": (2, 1, 256, 256, 128, 128, (64.0, 64.0), 32.0, 670),
}
# sign(residual) is decided by rounding where a residual is within the evaluation's own noise of zero, and ONE flipped pixel moves the
# gradient of the largest case by 2 / (B h w) = 6e-5 of a typical entry -- three times the bar.  A plain fp32 evaluation places its sampling
# coordinates within ~5e-5 px (the kernels, which form them in fp64: ~8e-6 px) and these images have slopes below 0.1 per px, so a residual
# is safe from 5e-6 on.  The seeds are the first for which the fp64 reference has no residual below that, under both sampling conventions
# (test_homography_train_cpu.py checks it): the comparison is then well-conditioned by construction, not by luck.
MIN_ABS_RESIDUAL = 5e-6


def stage1_inputs(name):
    """(delta, img_a, patch_b, corners) of a stage-1 case.  patch_b is 0.7 x img_a seen through a homography up to 3 px per corner away
    from the one ``delta`` gives, plus 0.3 x another smooth image: the gradient is the coherent pull towards that homography a training
    step sees, and the residual still has both signs everywhere."""
    B, C, H, W, ph, pw, tl, amp, seed = STAGE1_CASES[name]
    img_a = smooth_images(100 + seed, B, C, H, W)
    corners = box_corners(torch.tensor([tl] * B) + torch.arange(B).view(B, 1).float(), ph, pw)
    delta = deltas(300 + seed, B, amp)
    if name == "corner_64_p32":            # push the patch over the image's top-left corner: pixels with one and two valid taps
        delta = delta - corners[:, :1] - 6.0
    near = dlt_torch((corners - corners[:, :1]).double(), (corners + delta + deltas(400 + seed, B, 3.0)).double())
    patch_b = 0.7 * warp_torch(img_a.double(), near, (ph, pw), True) + 0.3 * smooth_images(200 + seed, B, C, ph, pw).double()
    return delta, img_a, patch_b.float(), corners


def min_abs_residual(delta, img_a, patch_b, corners, align_corners):
    """The smallest |patch_b_hat - patch_b| of the fp64 reference."""
    h = dlt_torch((corners - corners[:, :1]).double(), (corners + delta).double())
    return float((matrix_grad_closed(img_a.double(), h, None, patch_b.shape[-2:], align_corners)[0] - patch_b.double()).abs().min())


def descent_setup(which):
    """The descent test's (img_a, patch_b, corners, true delta): patch_b is img_a sampled at a known homography."""
    B, H, W, ph, pw, amp, tl = ((3, 64, 64, 32, 32, 4.0, (16.0, 16.0)), (2, 96, 80, 48, 40, 5.0, (20.0, 24.0)))[which]
    img_a = smooth_images(400 + which, B, 1, H, W)
    corners = box_corners(torch.tensor([tl] * B), ph, pw)
    true = deltas(500 + which, B, amp)
    h = dlt_torch((corners - corners[:, :1]).double(), (corners + true).double())
    patch_b = warp_torch(img_a.double(), h, (ph, pw), True).float()
    return img_a, patch_b, corners, true

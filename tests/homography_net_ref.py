"""Reference of HomographyNet in training mode (include/hesic_homography_net.h; a plain module, not a conftest).  No GPU.

* ``philox4x32_10`` / ``dropout_words`` / ``keep_mask`` / ``flatten_dropout``: the NumPy statement of the dropout masks -- Philox4x32-10 with
  counter (q lo, q hi, step, site), q = (b F + j) >> 2, key (seed lo, seed hi); an element is kept iff its word >= thr = rint(p 2^32).
* ``net_forward`` / ``net_grads``: ``Net`` (ywz/mywork/model.py:73-101) from ``F.conv2d`` / ``F.max_pool2d`` / ``F.linear`` with explicit
  masks, at any dtype (fp64: the reference; fp32: the noise floor of a plain evaluation) and any ``patch_size``.
* ``linear_reference``: the fp64 reference of the small-batch Linear kernels with the per-element error model of tests/conv_grad_ref.py,
  bar_e = 8 sqrt(n) 2^-24 S_e (+ 2^-8 |ref_e| where the output is stored in 16 bits): S_e the sum of absolute terms, n = In for y, Out for
  gx, B for dW and db.  The result has ``conv_grad_ref``'s layout, so ``conv_grad_ref.check`` compares every element.
* ``train_loop``: plain torch Adam over the restatement with the photometric loss of tests/homography_train_ref.py."""
import functools

import numpy as np
import torch
import torch.nn.functional as F

import conv_grad_ref as G
import homography_train_ref as HT
from conv_grad_ref import C_BAR, U24  # noqa: F401  (the bar model's constants: used through conv_grad_ref.check, not restated)
from hesic_amd import synthetic

_M0, _M1, _W0, _W1, _LO = (np.uint64(v) for v in (0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85, 0xFFFFFFFF))
_S32 = np.uint64(32)


def philox4x32_10(counter, key):
    """counter (..., 4) and key (2,) of 32-bit words -> (..., 4) uint32.  Each round:
    c' = (hi(M1 c2) ^ c1 ^ k0, lo(M1 c2), hi(M0 c0) ^ c3 ^ k1, lo(M0 c0)), then k0 += 0x9E3779B9, k1 += 0xBB67AE85."""
    counter = np.asarray(counter, dtype=np.uint64)
    c = [counter[..., i] for i in range(4)]
    k0, k1 = np.uint64(key[0]), np.uint64(key[1])
    for _ in range(10):
        p0, p1 = _M0 * c[0], _M1 * c[2]
        c = [(p1 >> _S32) ^ c[1] ^ k0, p1 & _LO, (p0 >> _S32) ^ c[3] ^ k1, p0 & _LO]
        k0, k1 = (k0 + _W0) & _LO, (k1 + _W1) & _LO
    return np.stack(c, -1).astype(np.uint32)


def dropout_words(B, Fdim, seed, step, site):
    """(B, F) uint32: the word of every element of a (B, F) output; F % 4 == 0."""
    assert Fdim % 4 == 0
    q = np.arange(B * Fdim // 4, dtype=np.uint64)
    ctr = np.stack([q & _LO, q >> _S32, np.full_like(q, step), np.full_like(q, site)], -1)
    return philox4x32_10(ctr, (seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF)).reshape(B, Fdim)


def thr_scale(p):
    """(thr, scale) of drop probability p: thr = rint(p 2^32) clamped to [0, 2^32 - 1]; scale the fp32 value 1.0f / (1.0f - (float)p)."""
    thr = min(max(int(np.rint(np.float64(p) * 4294967296.0)), 0), 4294967295)
    return thr, float(np.float32(1.0) / (np.float32(1.0) - np.float32(p)))


def keep_mask(B, Fdim, p, seed, step, site):
    """(B, F) bool tensor: True where the element is kept."""
    return torch.from_numpy(dropout_words(B, Fdim, seed, step, site) >= np.uint32(thr_scale(p)[0]))


def flatten_dropout(x, p, seed, step, site):
    """``x`` (B,C,H,W) or (B,F) -> (B,F) in x's dtype: NCHW flatten, kept elements times scale (one fp32 product), dropped ones +0."""
    flat = x.reshape(x.shape[0], -1)
    keep = keep_mask(flat.shape[0], flat.shape[1], p, seed, step, site)
    prod = (flat.float() * torch.tensor(thr_scale(p)[1], dtype=torch.float32)).to(x.dtype)
    return torch.where(keep, prod, torch.zeros((), dtype=x.dtype))


def flatten_dropout_backward(gy, shape, p, seed, step, site):
    """The gradient of ``flatten_dropout`` for an input of ``shape``."""
    return flatten_dropout(gy, p, seed, step, site).reshape(shape)


# ------------------------------------------------------------------------------------------------------------------ max pool
def pool_input(shape, name):
    """A ReLU output (>= 30 % exact zeros) with planted ties: all-zero windows and two equal positives in every pair of window positions."""
    x = torch.relu(synthetic._uniform(name, shape, -1.0, 1.5))
    B, Cc, H, W = shape
    x[:, :, 0:2, 0:2] = 0.0
    pairs = [(a, b) for a in range(4) for b in range(a + 1, 4)]
    for i, (p, q) in enumerate(pairs):
        wy, wx = divmod(i + 1, W // 2)
        if wy >= H // 2:
            break
        win = x[:, :, 2 * wy:2 * wy + 2, 2 * wx:2 * wx + 2]
        win.mul_(0.25)
        win[:, :, p // 2, p % 2] = 0.75
        win[:, :, q // 2, q % 2] = 0.75
    return x


# ------------------------------------------------------------------------------------------------------------------ the network
def net_masks(B, patch_size, seed, step, p=(0.5, 0.5)):
    """The two multiplicative masks (keep * scale, fp32 values) of a train-mode forward with dropout state (seed, step)."""
    side = patch_size // 8
    out = []
    for site, Fdim in enumerate((128 * side * side, 1024)):
        out.append(keep_mask(B, Fdim, p[site], seed, step, site).float() * torch.tensor(thr_scale(p[site])[1], dtype=torch.float32))
    return out


def net_forward(P, a, b, masks=None, dtype=torch.float64):
    """``Net.forward``: eval mode when ``masks`` is None, else train mode with the two masks of ``net_masks``.  ``P``: tensors of ``dtype``."""
    x = torch.cat((a, b), 1).to(dtype)
    for blk in range(4):
        pre = f"cnn.{blk}.layers."
        x = F.relu(F.conv2d(x, P[pre + "0.weight"], P[pre + "0.bias"], padding=1))
        x = F.relu(F.conv2d(x, P[pre + "2.weight"], P[pre + "2.bias"], padding=1))
        if blk < 3:
            x = F.max_pool2d(x, 2, 2)
    x = x.flatten(1)
    if masks is not None:
        x = x * masks[0].to(dtype)
    x = F.relu(F.linear(x, P["fc.2.weight"], P["fc.2.bias"]))
    if masks is not None:
        x = x * masks[1].to(dtype)
    return F.linear(x, P["fc.5.weight"], P["fc.5.bias"]).view(-1, 4, 2)


def net_params(patch_size=128, salt=0):
    """The synthetic state dict (fp32) of a net for ``patch_size``."""
    side = patch_size // 8
    shapes = {}
    for blk, (ci, co) in enumerate(((2, 64), (64, 64), (64, 128), (128, 128))):
        for idx, cin in ((0, ci), (2, co)):
            shapes[f"cnn.{blk}.layers.{idx}.weight"] = (co, cin, 3, 3)
            shapes[f"cnn.{blk}.layers.{idx}.bias"] = (co,)
    shapes.update({"fc.2.weight": (1024, 128 * side * side), "fc.2.bias": (1024,), "fc.5.weight": (8, 1024), "fc.5.bias": (8,)})
    return synthetic.fill_homography_state_dict_({k: torch.empty(v) for k, v in shapes.items()}, salt)


def net_grads(P, a, b, g, masks=None, dtype=torch.float64):
    """(delta, {name: d sum(delta * g) / d parameter}) by torch autograd at ``dtype``."""
    leaves = {k: v.detach().to(dtype).clone().requires_grad_() for k, v in P.items()}
    delta = net_forward(leaves, a, b, masks, dtype)
    grads = torch.autograd.grad((delta * g.to(dtype)).sum(), list(leaves.values()))
    return delta.detach(), dict(zip(leaves, grads))


def rel_err(x, ref):
    """|| x - ref ||_2 / || ref ||_2 in fp64."""
    x, ref = x.detach().double().cpu().reshape(-1), ref.detach().double().cpu().reshape(-1)
    return float((x - ref).norm()) / float(ref.norm())


# -------------------------------------------------------------------------------------------------------------- the Linear kernels
# tag: (B, In, Out, 16-bit activations)
LINEAR_CASES = {
    "b1_2048_1024": (1, 2048, 1024, False),
    "b3_520_8": (3, 520, 8, False),
    "b64_2048_1024": (64, 2048, 1024, False),
    "b5_1024_8": (5, 1024, 8, False),
    "b2_32768_1024": (2, 32768, 1024, False),          # fc.2 at patch_size = 128
    "h16_b3_2048_1024": (3, 2048, 1024, True),
}


# more rows than the small-batch kernels take: ``functional.linear`` goes through the 1x1 conv route
FALLBACK_CASES = {"b65_512_32": (65, 512, 32, False)}


@functools.lru_cache(maxsize=None)
def linear_operands(tag):
    """(x, w, b, gy) fp32; x and gy hold bf16-representable values in the 16-bit case (what the kernel is handed)."""
    B, In, Out, h16 = {**LINEAR_CASES, **FALLBACK_CASES}[tag]
    a = (6.0 / In) ** 0.5
    x = synthetic._uniform(f"lin.{tag}.x", (B, In), -1.0, 1.0)
    w = synthetic._uniform(f"lin.{tag}.w", (Out, In), -a, a)
    b = synthetic._uniform(f"lin.{tag}.b", (Out,), -0.05, 0.05)
    gy = synthetic._uniform(f"lin.{tag}.gy", (B, Out), -1.0, 1.0)
    if h16:
        x, gy = G.bf(x), G.bf(gy)
    return x, w, b, gy


def linear_reference(tag, act, y_saved=None):
    """fp64 y, dx (= gx), dw, db of a case with sums of absolute terms and term counts, in ``conv_grad_ref``'s layout.  With ReLU the
    incoming gradient is gated by the y the backward saved (``y_saved``) when the caller has it, as ``conv_grad_ref`` does."""
    B, In, Out, h16 = {**LINEAR_CASES, **FALLBACK_CASES}[tag]
    x, w, b, gy = (t.double() for t in linear_operands(tag))
    pre = x @ w.t() + b
    y = torch.relu(pre) if act == G.ACT_RELU else pre
    g = G.act_grad(gy, y if y_saved is None else y_saved.double().cpu(), act, h16)
    ref = {"y": y, "dx": g @ w, "dw": g.t() @ x, "db": g.sum(0)}
    S = {"y": x.abs() @ w.abs().t() + b.abs(), "dx": g.abs() @ w.abs(), "dw": g.abs().t() @ x.abs(), "db": g.abs().sum(0)}
    return {"ref": ref, "S": S, "n": {"y": In, "dx": Out, "dw": B, "db": B}, "y16": h16, "dx16": h16, "g": g}


def linear_torch_fp32(tag, act):
    """torch's own fp32 ``F.linear`` + autograd on the same operands: {"y", "dx", "dw", "db"}."""
    x, w, b, gy = (t.clone().requires_grad_() for t in linear_operands(tag))
    pre = F.linear(x, w, b)
    y = torch.relu(pre) if act == G.ACT_RELU else pre
    dx, dw, db = torch.autograd.grad(y, (x, w, b), gy.detach())
    return {"y": y.detach(), "dx": dx, "dw": dw, "db": db}


# ------------------------------------------------------------------------------------------------------------------ training loop
def trainer_inputs(B=4, seed=0):
    """(img_a, patch_a, patch_b, corners) of the trainer tests: a smooth 64 x 64 texture, patch_b its warp by a known small homography
    (up to 2 px per corner) sampled on the 32 x 32 patch at (16, 16), patch_a the plain crop."""
    img_a = HT.smooth_images(700 + seed, B, 1, 64, 64)
    corners = HT.box_corners(torch.tensor([[16.0, 16.0]] * B), 32, 32)
    true = HT.deltas(710 + seed, B, 2.0)
    h = HT.dlt_torch((corners - corners[:, :1]).double(), (corners + true).double())
    patch_b = HT.warp_torch(img_a.double(), h, (32, 32), True).float()
    return img_a, img_a[:, :, 16:48, 16:48].contiguous(), patch_b, corners


def eval_loss(P, inputs, dtype=torch.float64):
    img_a, patch_a, patch_b, corners = inputs
    with torch.no_grad():
        delta = net_forward({k: v.to(dtype) for k, v in P.items()}, patch_a, patch_b, None, dtype)
        return float(HT.photometric_torch(delta, img_a, patch_b, corners, True, dtype=dtype))


def train_loop(P0, inputs, steps, lr, seed, dtype=torch.float64, patch_size=32, first_step=0):
    """``steps`` iterations of forward (train mode, the masks of (seed, first_step + t)) -> photometric loss -> backward -> torch.optim.Adam on
    one fixed batch.  Returns (losses before each update, final parameters)."""
    img_a, patch_a, patch_b, corners = inputs
    P = {k: v.detach().to(dtype).clone().requires_grad_() for k, v in P0.items()}
    opt = torch.optim.Adam(list(P.values()), lr=lr)
    losses = []
    for t in range(steps):
        masks = net_masks(patch_a.shape[0], patch_size, seed, first_step + t)
        delta = net_forward(P, patch_a, patch_b, masks, dtype)
        loss = HT.photometric_torch(delta, img_a, patch_b, corners, True, dtype=dtype)
        opt.zero_grad()
        loss.backward()
        opt.step()
        losses.append(float(loss.detach()))
    return losses, {k: v.detach() for k, v in P.items()}


@functools.lru_cache(maxsize=None)
def trainer_reference(steps, fp64):
    """(P0, inputs, L0, losses, final parameters) of ``train_loop`` on ``trainer_inputs()`` from ``net_params(32)`` with lr 1e-4 and seed 0:
    computed once per (steps, dtype) and shared by the tests that need it (read-only)."""
    inputs, P0 = trainer_inputs(), net_params(32)
    losses, P = train_loop(P0, inputs, steps, 1e-4, 0, dtype=torch.float64 if fp64 else torch.float32)
    return P0, inputs, eval_loss(P0, inputs), losses, P

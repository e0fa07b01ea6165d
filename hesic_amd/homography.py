"""HomographyNet and the h_matrix derivation -- the step immediately in front of ``HSIC.forward`` in the reference's
``_real`` scripts: ``Net`` of ``ywz/mywork/model.py:73-111`` and ``newtrain1_real.py:113-123``.

Same module tree and state-dict keys as the reference (``cnn.N.layers.{0,2}.{weight,bias}``, ``fc.{2,5}.*``), so a
``homo_best.pth.tar`` checkpoint loads strictly.  Every layer runs on the HIP kernels of ``libhesic_hip.so``.

Inference (eval mode under ``torch.no_grad()``, its use on the path: the reference keeps the net frozen, ``newtrain1_real.py:78``):

* conv3x3 + ReLU: the narrow (Cin = 2) / implicit-GEMM conv kernels with the activation fused;
* MaxPool2d(2,2): ``hesic_maxpool2_forward`` on the NHWC map;
* Linear: a 1x1 implicit-GEMM conv over the NHWC-flattened map (the first Linear's columns are permuted once from the
  reference's NCHW flatten order; the low-resolution split-K launch spreads its 32768-deep contraction over the GPU);
* corner deltas -> h_matrix: ``hesic_h_from_delta`` (4-point DLT, 3x3 inverse and the reference's ``h_adjust``).

With grad mode on, or in training mode (``udh/udh/QHtrain.py:88-102``; ``train.HomographyTrainer``), the same conv blocks are followed by
the kernels of include/hesic_homography_net.h: the max pools get their backward, the map is flattened into the reference's NCHW order with
the first Dropout fused in (``hesic_flatten_dropout_*``: the ACTIVATION is permuted, so ``fc.2.weight`` is used -- and its gradient lands --
in its own layout), and both Linear layers run on the small-batch kernels over the fp32 master weights (``hesic_linear_*``; more than 64
rows fall back to the 1x1 conv route).  Dropout masks are a Philox4x32-10 stream of ``(seed, step, site, element index)``:
``set_dropout_state`` / ``dropout_state``; every train-mode forward uses the current ``step`` for both sites and then increments it.
Up to 64 rows per batch no gradient kernel on this route uses atomics (the conv blocks run under ``functional.deterministic_conv_grads``):
the same inputs give the same bits in every run.  Larger batches train too, but the conv route of their fc layers sums biases with float
atomics, so their last bits vary.
Training mode needs ``dtype=torch.float32``, what the reference trains.

Image pairs that are already on the device become the net's inputs in one launch (``prepare_inputs``, include/hesic_homography_prep.h:
the loader's ``ImageFolder._homonet_inputs`` -- resize to 256 x 256, quantise, normalise, grey, one 128 x 128 window with its corners -- for
both views of a batch); ``h_matrix_from_pair`` goes from such a batch to its ``h_matrix``.

Feature maps are fp32 by default (the deltas are pixel offsets that steer a full-resolution warp); pass
``dtype=torch.bfloat16`` for bf16 storage.
"""
from __future__ import annotations

import torch
import torch.nn as nn

from . import _lib as L
from . import functional as Fn
from . import geometry
from .compressai.models.utils import HipConv2d

__all__ = ["Net", "Block", "Flatten", "max_pool2", "get_perspective_transform", "h_matrix_from_delta", "h_matrix", "photometric_loss", "corner_error",
           "refine_h_matrix",
           "window_origins", "draw_deltas", "prepare_inputs", "h_matrix_from_pair", "load_checkpoint", "checkpoint_state_dict", "net_state_dict"]


def max_pool2(x):
    """nn.MaxPool2d(2, 2) on a channels_last map (model.py:62-63); differentiable (``hesic_maxpool2_backward``)."""
    return Fn.max_pool2(x)


class _HipMaxPool2d(nn.MaxPool2d):
    def forward(self, x):
        if self.kernel_size not in (2, (2, 2)) or self.stride not in (2, (2, 2)) or self.padding not in (0, (0, 0)):
            raise NotImplementedError("hesic_amd max pool: 2x2 stride 2")
        return max_pool2(x)


class Flatten(nn.Module):
    def forward(self, x):
        return x.reshape(x.size(0), -1)


class Block(nn.Module):
    """conv3x3 + ReLU, conv3x3 + ReLU, [MaxPool2d(2,2)] (model.py:50-71; batch_norm=False is what the scripts use)."""

    def __init__(self, inchannels, outchannels, batch_norm=False, pool=True):
        super().__init__()
        if batch_norm:
            raise NotImplementedError("HomographyNet on the HIP path: batch_norm=False (the configuration the reference trains)")
        layers = [HipConv2d(inchannels, outchannels, kernel_size=3, padding=1), nn.ReLU(),
                  HipConv2d(outchannels, outchannels, kernel_size=3, padding=1), nn.ReLU()]
        if pool:
            layers.append(_HipMaxPool2d(2, 2))
        self.layers = nn.Sequential(*layers)

    def forward(self, x):
        x = self.layers[0].run(x, act=L.ACT_RELU)
        x = self.layers[2].run(x, act=L.ACT_RELU)
        return self.layers[4](x) if len(self.layers) > 4 else x


class Net(nn.Module):
    """HomographyNet: two grey patches -> (B,4,2) corner deltas (model.py:73-101)."""

    def __init__(self, batch_norm=False, patch_size=128, dtype=torch.float32):
        super().__init__()
        self.cnn = nn.Sequential(Block(2, 64, batch_norm), Block(64, 64, batch_norm), Block(64, 128, batch_norm),
                                 Block(128, 128, batch_norm, pool=False))
        self.side = patch_size // 8
        self.fc = nn.Sequential(Flatten(), nn.Dropout(p=0.5), nn.Linear(128 * self.side * self.side, 1024), nn.ReLU(),
                                nn.Dropout(p=0.5), nn.Linear(1024, 4 * 2))
        self.dtype = dtype
        self._fc_pack = [Fn.PackedWeight(), Fn.PackedWeight(), Fn.PackedWeight(), Fn.PackedWeight()]      # inference fc.2 / fc.5; the > 64-row training route
        self._fc1_nhwc = None
        self._drop_seed, self._drop_step = 0, 0
        self._drop_dev = None                       # dropout_on_device: int32 {seed lo, seed hi, step, 0} in device memory

    def _fc1_weight(self):
        """fc.2.weight with its columns moved from NCHW-flatten (c, y, x) to NHWC-flatten (y, x, c) order; cached."""
        w = self.fc[2].weight
        tag = (w.data_ptr(), w._version)
        if self._fc1_nhwc is None or self._fc1_nhwc[0] != tag:
            s = self.side
            wn = w.detach().view(-1, 128, s, s).permute(0, 2, 3, 1).reshape(w.shape[0], -1, 1, 1).contiguous()
            self._fc1_nhwc = (tag, wn)
        return self._fc1_nhwc[1]

    def set_dropout_state(self, seed, step=0):
        """Seed and step counter of the dropout masks (both sites of ``fc``).  With ``dropout_on_device`` the device copy is rewritten too
        (device fills: not while a stream is capturing)."""
        self._drop_seed, self._drop_step = int(seed) & 0xFFFFFFFFFFFFFFFF, int(step) & 0xFFFFFFFF
        if self._drop_dev is not None:
            if torch.cuda.is_current_stream_capturing():
                raise RuntimeError("Net.set_dropout_state: the device copy of the dropout state cannot be rewritten while a stream is capturing")
            for i, word in enumerate(Fn._dropout_words(self._drop_seed, self._drop_step).tolist()):
                self._drop_dev[i:i + 1].fill_(word)      # device fills, as FlatAdam.sync_lr: no host buffer, no synchronisation

    def dropout_state(self):
        """(seed, step): ``step`` is what the NEXT train-mode forward uses.  With ``dropout_on_device`` it is read back from the device
        (synchronises)."""
        if self._drop_dev is not None:
            lo, hi, step, _ = (int(v) & 0xFFFFFFFF for v in self._drop_dev.tolist())
            self._drop_seed, self._drop_step = lo | (hi << 32), step
        return self._drop_seed, self._drop_step

    def dropout_on_device(self, flag=True):
        """Keep the dropout ``(seed, step)`` in sixteen bytes of device memory (``hesic_dropout_state_take`` / ``hesic_flatten_dropout_*_state``):
        a train-mode forward then takes the state in one tiny launch -- both sites use what it took, the step is incremented on the device --
        so a forward recorded into a HIP graph draws a new mask at every replay (``train.GraphedHomographyTrainer``).  The masks are those
        of the by-value route for the same ``(seed, step)``.  Off (the default), the forward issues exactly the by-value launches."""
        if flag and self._drop_dev is None:
            self._drop_dev = Fn.dropout_state(self._drop_seed, self._drop_step, self.fc[2].weight.device)
        elif not flag and self._drop_dev is not None:
            self.dropout_state()                    # the host copy takes over where the device copy stands
            self._drop_dev = None
        return self

    def forward(self, a, b):
        if self.training or torch.is_grad_enabled():
            return self._forward_train(a, b)
        L.require_cuda(a, b)
        x = torch.cat((a, b), dim=1).to(self.dtype)
        prev = Fn.compute_dtype()
        Fn.set_compute_dtype(self.dtype)            # storage type of the maps the narrow first conv produces
        try:
            x = self.cnn(x)                          # (B,128,side,side), NHWC in memory
            B = x.shape[0]
            x = x.contiguous(memory_format=torch.channels_last).permute(0, 2, 3, 1).reshape(B, -1, 1, 1)
            x = x.contiguous(memory_format=torch.channels_last)
            x = Fn.conv2d(x, self._fc1_weight(), self.fc[2].bias, kernel_size=1, stride=1, padding=0, act=L.ACT_RELU,
                          packer=self._fc_pack[0])
            w2 = self.fc[5].weight                   # 8 outputs: still the implicit-GEMM kernel (one padded cout tile)
            wp = self._fc_pack[1].get(w2.view(w2.shape[0], w2.shape[1], 1, 1), None, w2.shape[0], w2.shape[1], 1, 1, False,
                                      False, x.dtype)
            x = Fn._wide_conv(x, wp, self.fc[5].bias, B, 1, 1, w2.shape[1], 1, 1, w2.shape[0], 1, 1, 0, False)
        finally:
            Fn.set_compute_dtype(prev)
        return x.reshape(-1, 4, 2).float()

    def _forward_train(self, a, b):
        """Grad mode on (eval: no dropout, differentiable) or training mode (dropout at ``fc[1].p`` / ``fc[4].p``, with or without grad)."""
        if self.training and self.dtype != torch.float32:
            raise NotImplementedError("hesic_amd HomographyNet: training mode needs dtype=torch.float32 (what the reference trains); "
                                      f"this module stores its maps as {self.dtype}")
        seed, step = self._drop_seed, self._drop_step
        cfgs = [Fn.dropout_args(self.fc[i].p if self.training else 0.0, seed, step, site) for site, i in enumerate((1, 4))]
        L.require_cuda(a, b)
        on_device = self.training and self._drop_dev is not None       # eval mode with grad: p = 0, no state needed and none taken
        if on_device:
            taken = Fn.dropout_state_take(self._drop_dev)        # both sites use what it took; the device step is incremented
            cfgs = [Fn.dropout_state_args(self.fc[i].p, taken, site) for site, i in enumerate((1, 4))]
        x = torch.cat((a, b), dim=1).to(self.dtype)
        prev = Fn.compute_dtype()
        Fn.set_compute_dtype(self.dtype)
        try:
            with Fn.deterministic_conv_grads():      # no float atomics in the conv biases' / first layer's gradients: the same bits in every run
                #   (up to 64 rows: above that fc takes the conv route, whose bias sums end in atomics)
                x = self.cnn(x)
            x = Fn.flatten_dropout(x, cfgs[0])       # (B, 128 side^2) in the reference's flatten order
            x = Fn.linear(x, self.fc[2].weight, self.fc[2].bias, act=L.ACT_RELU, packer=self._fc_pack[2])
            x = Fn.flatten_dropout(x, cfgs[1])
            x = Fn.linear(x, self.fc[5].weight, self.fc[5].bias, packer=self._fc_pack[3])
        finally:
            Fn.set_compute_dtype(prev)
        if self.training and self._drop_dev is None:
            self._drop_step = (step + 1) & 0xFFFFFFFF
        return x.reshape(-1, 4, 2).float()

    def get_h(self, a, b, corners):
        """inverse(get_perspective_transform(corners, corners + delta)) (model.py:99-111)."""
        delta = self.forward(a, b)
        return h_matrix_from_delta(corners, delta, 1.0, 1.0, 1.0, subtract_origin=False)


def get_perspective_transform(src, dst):
    """kornia.get_perspective_transform (B,4,2),(B,4,2) -> (B,3,3) with dst ~ H src.  Differentiable in both point sets (the DLT adjoint,
    ``hesic_perspective_transform_backward``)."""
    L.require_cuda(src, dst)
    return Fn.perspective_transform(src.contiguous().float(), dst.contiguous().float())


def h_matrix_from_delta(corners, delta, img_h, img_w, pic_size, subtract_origin=True):
    """newtrain1_real.py:113-123: corners0 = corners - corners[:,0]; h = gpt(corners0, corners0 + delta);
    h_matrix = h_adjust(img_h, img_w, pic_size, pic_size, inverse(h)) -- one kernel, no host round trip.  Differentiable in ``delta``
    (``hesic_h_from_delta_backward``: h_adjust, the 3x3 inverse and the DLT adjoint in one kernel)."""
    L.require_cuda(corners, delta)
    return Fn.h_from_delta(corners.contiguous().float(), delta.contiguous().float(), float(img_h) / float(pic_size),
                           float(img_w) / float(pic_size), subtract_origin)


def photometric_loss(delta, img_a, patch_b, corners):
    """The loss HomographyNet trains on (ywz/mywork/model.py:18-45; udh/udh/QHtrain.py:99)::

        c0 = corners - corners[:, :1];  h = get_perspective_transform(c0, corners + delta)
        patch_b_hat = warp_perspective(img_a, inverse(h), patch_b.shape[-2:]);  loss = l1_loss(patch_b_hat, patch_b)

    ``patch_b_hat(p) = bilinear(img_a, h p)`` is the warp by ``inverse(h)``: no matrix is inverted.  ``delta``, ``corners`` (B,4,2);
    ``img_a`` (B,C,H,W) and ``patch_b`` (B,C,h,w) fp32 with any strides.  Returns a 0-d fp32 device tensor with autograd to ``delta`` only,
    bit-identical from run to run; the sampling convention is ``geometry.DEFAULT_ALIGN_CORNERS``, as in ``geometry.warp_perspective``."""
    if img_a.requires_grad or patch_b.requires_grad:
        raise RuntimeError("photometric_loss: the gradient goes to delta only (img_a / patch_b must not require grad)")
    if img_a.dim() != 4 or patch_b.dim() != 4 or patch_b.shape[:2] != img_a.shape[:2]:
        raise ValueError(f"photometric_loss: expected img_a (B,C,H,W) and patch_b (B,C,h,w), got {tuple(img_a.shape)}, {tuple(patch_b.shape)}")
    if tuple(delta.shape) != (img_a.shape[0], 4, 2) or corners.shape != delta.shape:
        raise ValueError(f"photometric_loss: expected delta and corners (B,4,2), got {tuple(delta.shape)}, {tuple(corners.shape)}")
    if img_a.dtype != torch.float32 or patch_b.dtype != torch.float32:
        raise TypeError("photometric_loss: float32 images")
    return Fn.photometric_loss(delta.float(), img_a, patch_b, corners.float(), geometry.DEFAULT_ALIGN_CORNERS)


def corner_error(delta_hat, delta):
    """Mean corner error per pair: the mean over the four corners of ``||delta_hat_k - delta_k||_2``, in pixels of the frame the deltas are
    measured in.  (B,4,2) twice -> (B,) fp32.  ``delta_hat = 0`` gives the error of predicting the identity, the figure to beat."""
    return (delta_hat.float() - delta.float()).square().sum(-1).sqrt().mean(-1)


def refine_h_matrix(x1, x2, h_matrix, *, levels=3, iters=10, huber=None, min_overlap=0.25, align_corners=None):
    """Refine ``h_matrix`` photometrically: Gauss-Newton with Levenberg-Marquardt damping on ``grey(x1)(H^-1 p) - grey(x2)(p)``, coarse to
    fine over ``levels`` pyramid levels with ``iters`` candidates after each level's first (include/hesic_homography_refine.h).

    ``x1``, ``x2``: (B,C,H,W) fp32 of one shape, C = 1 or 3, any non-negative strides (un-padded views are fine), at least 16 pixels on a
    side; ``h_matrix``: (B,3,3) or (1,3,3), x1 pixel -> x2 pixel, what ``HSIC.forward`` takes.  ``huber``: None for plain least squares, or
    the residual (in grey levels of the input's scale) above which a pixel's weight falls as ``huber / |r|``.  A candidate that keeps fewer
    than ``min_overlap`` of the level's pixels valid is rejected.

    Returns ``(h_refined, info)``: (B,3,3) fp32 and a dict of device tensors that this function never reads back -- ``cost_before`` /
    ``cost_after`` (mean squared grey residual over the valid pixels of level 0, fp64), ``accepted`` / ``rejected`` (int32 candidate counts),
    ``valid_share`` (fp64) and ``levels_used`` (int32).  The result is never worse than the input by that measure: where no candidate was
    accepted or level 0's final cost is not below ``cost_before`` -- no overlap, a singular matrix, an ``x2`` without contrast (a constant
    view says nothing about geometry: such a level does nothing), ``iters=0`` -- the pair's input comes back
    bit for bit with ``cost_after == cost_before``.  Deterministic, free of host synchronisation, and capturable into a graph.

    This is a refiner, not an estimator: its basin is a few texture correlation lengths at the coarsest level (start it from the SURF + RANSAC
    sidecar or from HomographyNet).  Only ``align_corners=True`` sampling is implemented."""
    for t in (x1, x2, h_matrix):
        if not torch.is_tensor(t):
            raise TypeError(f"refine_h_matrix: tensors expected, got {type(t).__name__}")
    ac = geometry.DEFAULT_ALIGN_CORNERS if align_corners is None else bool(align_corners)
    if not ac:
        raise NotImplementedError("refine_h_matrix: only align_corners=True sampling is implemented; the legacy align_corners=False "
                                  "convention (geometry.use_reference_era_warp, HESIC_WARP_ALIGN_CORNERS=0) is out of scope")
    if x1.dim() != 4 or x1.shape != x2.shape or x1.shape[1] not in (1, 3):
        raise RuntimeError(f"refine_h_matrix: x1 and x2 must be (B, 1 or 3, H, W) tensors of one shape, got {tuple(x1.shape)} and {tuple(x2.shape)}")
    B, _, H, W = x1.shape
    if B == 0:
        raise RuntimeError("refine_h_matrix: empty batch")
    if h_matrix.dim() != 3 or h_matrix.shape[-2:] != (3, 3) or h_matrix.shape[0] not in (1, B):
        raise RuntimeError(f"refine_h_matrix: h_matrix must be (B, 3, 3) (or (1, 3, 3)), got {tuple(h_matrix.shape)}")
    if x1.dtype != torch.float32 or x2.dtype != torch.float32 or h_matrix.dtype != torch.float32:
        raise TypeError(f"refine_h_matrix: float32 images and matrix, got {x1.dtype}, {x2.dtype}, {h_matrix.dtype}")
    if min(H, W) < L.HREFINE_MIN_SIDE:
        raise RuntimeError(f"refine_h_matrix: images must be at least {L.HREFINE_MIN_SIDE} pixels on a side, got {H}x{W}")
    if not 1 <= int(levels) <= L.HREFINE_MAX_LEVELS or int(iters) < 0:
        raise ValueError(f"refine_h_matrix: levels in [1, {L.HREFINE_MAX_LEVELS}] and iters >= 0, got levels={levels}, iters={iters}")
    if huber is not None and not float(huber) > 0.0:
        raise ValueError(f"refine_h_matrix: huber is None or positive, got {huber}")
    if not 0.0 <= float(min_overlap) <= 1.0:
        raise ValueError(f"refine_h_matrix: min_overlap in [0, 1], got {min_overlap}")
    if any(s < 0 for s in x1.stride() + x2.stride()):
        raise ValueError("refine_h_matrix: negative strides are not supported")
    L.require_cuda(x1, x2, h_matrix)
    h = h_matrix.detach().expand(B, 3, 3).contiguous()
    out, rec = Fn.homography_refine(x1.detach(), x2.detach(), h, int(levels), int(iters), huber, float(min_overlap))
    info = {"cost_before": rec[:, 0], "cost_after": rec[:, 1], "accepted": rec[:, 2].to(torch.int32), "rejected": rec[:, 3].to(torch.int32),
            "valid_share": rec[:, 4], "levels_used": rec[:, 5].to(torch.int32)}
    return out, info


def h_matrix(net, homo_img1, homo_img2, homo_corners, img_h, img_w, pic_size=256):
    """The h_matrix of a stereo pair as the `_real` scripts derive it (newtrain1_real.py:108-123)."""
    with torch.no_grad():
        delta = net(homo_img1, homo_img2)
        return h_matrix_from_delta(homo_corners, delta, img_h, img_w, pic_size)


def window_origins(batch, xy=None, pic_size=256, patch_size=128, rho=45, rng=None):
    """The (x, y) window origins of ``batch`` items as a list of pairs.  ``xy=None``: the loader's rule and draw order
    (``ImageFolder._homonet_inputs``) -- per item ``x`` then ``y`` from ``randint(rho, S - rho - P)`` when ``S - rho - P >= rho``, else 0, 0 --
    from ``rng`` (a ``random.Random``; default: Python's global ``random``, so a seeded run reproduces the loader's windows).
    ``xy="centre"``: ``(S - P) // 2`` for both.  A (B, 2) integer tensor or sequence is used as given.  Range violations raise ValueError."""
    import random
    S, P, rho, B = int(pic_size), int(patch_size), int(rho), int(batch)
    if not 1 <= P <= S:
        raise ValueError(f"prepare_inputs: need 1 <= patch_size <= pic_size, got patch_size={P}, pic_size={S}")
    if isinstance(xy, str):
        if xy != "centre":
            raise ValueError(f"prepare_inputs: xy is None, 'centre' or (B,2) integers, got {xy!r}")
        return [((S - P) // 2, (S - P) // 2)] * B
    if xy is None:
        if rho < 0:
            raise ValueError(f"prepare_inputs: rho must not be negative, got {rho}")
        r = rng if rng is not None else random
        out = []
        for _ in range(B):
            if S - rho - P >= rho:
                x = r.randint(rho, S - rho - P)
                y = r.randint(rho, S - rho - P)
            else:
                x = y = 0
            out.append((x, y))
        return out
    if torch.is_tensor(xy):
        if xy.is_floating_point() or xy.is_complex() or xy.dtype == torch.bool:
            raise TypeError(f"prepare_inputs: xy must hold integers, got {xy.dtype}")
        vals = xy.detach().cpu().tolist()
    else:
        vals = [list(v) if hasattr(v, "__len__") else v for v in xy]
    if len(vals) != B or any(not hasattr(v, "__len__") or len(v) != 2 for v in vals):
        raise ValueError(f"prepare_inputs: xy must have shape ({B}, 2)")
    out = []
    for x, y in vals:
        if int(x) != x or int(y) != y:
            raise TypeError(f"prepare_inputs: xy must hold integers, got ({x!r}, {y!r})")
        if not (0 <= x <= S - P and 0 <= y <= S - P):
            raise ValueError(f"prepare_inputs: window origin ({x}, {y}) outside [0, {S - P}] (pic_size {S}, patch_size {P})")
        out.append((int(x), int(y)))
    return out


def draw_deltas(batch, windows, patch_size, rho, rng):
    """The corner offsets of ``batch`` synthetic warps (include/hesic_homonet_synth.h) as a list of eight integers per item, the label of
    supervised training: per item eight ``rng.randrange(-rho, rho)`` in the order corner 0 x, corner 0 y, ... corner 3 y -- the range of the
    reference's ``randint_like(corners, -rho, rho)`` (udh/udh/dataset.py) --, drawn again, all eight, while the window's corners moved by
    them are not a strictly convex quadrilateral (``functional.perturbed_quad_is_convex``).  ``windows``: the items' window origins
    ``(wx, wy)``, or their (B,4,2) corners, whose first corner is the origin.  ``rho = 0`` gives zeros without a draw.  A pure host function
    that consumes only ``rng`` (a ``random.Random``)."""
    B, P, rho = int(batch), int(patch_size), int(rho)
    if rho < 0:
        raise ValueError(f"draw_deltas: rho must not be negative, got {rho}")
    if torch.is_tensor(windows):
        windows = windows.detach().cpu().tolist()
    origins = []
    for w in windows:
        x, y = w[0] if hasattr(w[0], "__len__") else w
        if int(x) != x or int(y) != y:
            raise TypeError(f"draw_deltas: window origins must hold integers, got ({x!r}, {y!r})")
        origins.append((int(x), int(y)))
    if len(origins) != B:
        raise ValueError(f"draw_deltas: {B} items need as many windows, got {len(origins)}")
    out = []
    for wx, wy in origins:
        if rho == 0:
            out.append([0] * 8)
            continue
        while True:
            d = [rng.randrange(-rho, rho) for _ in range(8)]
            if Fn.perturbed_quad_is_convex(wx, wy, P, d):
                break
        out.append(d)
    return out


def prepare_inputs(x1, x2, xy=None, pic_size=256, patch_size=128, rho=45, rng=None):
    """HomographyNet's inputs of a stereo batch on the device, in one launch (``hesic_homonet_prepare``): what the loader's
    ``ImageFolder._homonet_inputs`` computes per item on the host.  ``x1``, ``x2``: (B,3,H,W) of one shape and dtype, uint8 or float32 in
    [0, 1], any non-negative strides.  ``xy``: see ``window_origins``.  Returns ``(grey1, grey2, patch1, patch2, corners)``: the normalised
    grey frames (B,1,S,S), their windows (B,1,P,P) and the windows' corners (B,4,2), all fp32."""
    from .compressai.datasets import MEAN, STD
    for t in (x1, x2):
        if not torch.is_tensor(t):
            raise TypeError(f"prepare_inputs: tensors expected, got {type(t).__name__}")
    if x1.dim() != 4 or x1.shape[1] != 3 or x1.shape != x2.shape:
        raise ValueError(f"prepare_inputs: expected two (B,3,H,W) tensors of one shape, got {tuple(x1.shape)}, {tuple(x2.shape)}")
    if x1.dtype != x2.dtype or x1.dtype not in (torch.uint8, torch.float32):
        raise TypeError(f"prepare_inputs: both views uint8 or both float32, got {x1.dtype}, {x2.dtype}")
    origins = window_origins(x1.shape[0], xy, pic_size, patch_size, rho, rng)          # host checks come before any launch
    L.require_cuda(x1, x2)
    xy_dev = torch.tensor(origins, dtype=torch.int32).reshape(-1, 2).to(x1.device, non_blocking=True)
    return Fn.homonet_prepare(x1, x2, xy_dev, int(pic_size), int(patch_size), float(MEAN), float(STD))


def h_matrix_from_pair(net, x1, x2, xy="centre", pic_size=256):
    """(B,3,3) ``h_matrix`` of a stereo batch on the device, for the images' own size: ``prepare_inputs`` (window side ``net.side * 8``),
    then ``h_matrix`` -- the `_real` scripts' derivation for every pair (newtrain1_real.py:108-126), under ``no_grad``."""
    with torch.no_grad():
        _, _, p1, p2, corners = prepare_inputs(x1, x2, xy, pic_size, net.side * 8)
        return h_matrix(net, p1, p2, corners, x1.shape[-2], x1.shape[-1], pic_size)


_CKPT_PREFIX = "model."


def checkpoint_state_dict(net):
    """``net.state_dict()`` on the host under the reference's key names: ``HomographyModel`` wraps ``Net`` as ``.model``, so a
    ``homo_best.pth.tar`` names every tensor ``model.<key>``."""
    return {_CKPT_PREFIX + k: v.detach().cpu().clone() for k, v in net.state_dict().items()}


def net_state_dict(sd):
    """A checkpoint's state dict under ``Net``'s own key names: the ``model.`` prefix is dropped where every key carries it."""
    if sd and all(k.startswith(_CKPT_PREFIX) for k in sd):
        return {k[len(_CKPT_PREFIX):]: v for k, v in sd.items()}
    return dict(sd)


def load_checkpoint(net, path):
    """Load a HomographyNet checkpoint strictly: a file with a ``state_dict`` entry (what ``python -m hesic_amd.homography_train`` and the
    reference's QHtrain write) or a bare state dict, its keys with or without the ``model.`` prefix.  Returns the loaded file's dict."""
    ckpt = torch.load(path, map_location="cpu")
    net.load_state_dict(net_state_dict(ckpt["state_dict"] if isinstance(ckpt, dict) and "state_dict" in ckpt else ckpt), strict=True)
    return ckpt

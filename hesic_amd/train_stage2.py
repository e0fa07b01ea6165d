"""``python -m hesic_amd.train_stage2 ROOT``: train the enhancement net ``Independent_EN`` on the reconstructions of a FROZEN HSIC / HSICJoint
from a stereo folder -- ``ywz/mywork/newtrain6_real.py``'s loop on the device, the stage between ``train_folder`` and
``eval_folder --enhancer``.

    ROOT/train/{left,right}/ + ROOT/train/H/, ROOT/<--valid-split>/{left,right}/            the layout of ``train_folder``

    -e/--epochs 100  -lr/--learning-rate 1e-4  --lambda 1e-2  --batch-size 16  --test-batch-size 64  --patch-size 256 256  -n/--num-workers 3
    --save  --seed S  --homography sidecar|net|surf  --homography-checkpoint PATH  --clip-max-norm X  --skip-nonfinite  --graphed
    --dtype bf16|f32  --cache device|stream  --cache-gb G  --valid-split test  --out DIR  --augment hflip vflip swap    as in ``train_folder``
    --model hesic|joint  --checkpoint PATH|synthetic   the frozen model (required; ``synthetic``: the deterministic weights)
    --infer-dtype f16|bf16|f32                         the format of the frozen forward (default f16); ``--dtype`` is the enhancer's training format
    --resume PATH|none                                 a ``second_checkpoint*.pth.tar`` of this command

Batches come from ``pair_cache.DevicePairCache`` and ``pair_cache.epoch_plan`` exactly as in ``train_folder`` (one gather launch per batch; the
shared pieces -- options, refusals, the epoch passes and the run loop -- live in ``folder_loop``).  The step is
``train.EnhancerTrainer.step``, or with ``--graphed`` ``train.GraphedEnhancerTrainer.step`` (the gather writes into the captured step's static inputs; an epoch's ragged last batch is dropped and counted).

Per epoch: train, then a validation pass in eval mode under ``no_grad`` in the inference format: the frozen forward feeds
``Independent_EN.forward``; per batch ``loss = lambda * 255^2 * mse_loss``, ``mse_loss``, ``bpp_loss`` (from the frozen model's likelihoods),
``psnr1`` and ``psnr2`` -- ``models.rate_distortion``'s quantities, taken from ``models.pair_metrics``' per-pair sums because those are added in a
fixed order (a record is then the same bits in every run) -- on the enhanced images, and ``ms_ssim1`` / ``ms_ssim2`` (``models.ms_ssim``) when
both patch sides exceed 160.  The reported value is the mean over batches, added up on the device and read back once; ``psnr`` =
(psnr1 + psnr2) / 2 and ``psnr_of_mse`` = mse2psnr(mse_loss / 2) are both in the record.  With ``--save``: ``DIR/second_checkpoint.pth.tar`` =
``{"epoch", "state_dict", "loss", "optimizer", "aux_optimizer", "seed"}`` -- ``state_dict`` is ``Independent_EN``'s, on the host, under the
reference's keys (``eval_folder.load_enhancer`` and the reference's ``Independent_EN().load_state_dict`` read it); ``aux_optimizer`` is the
state of a never-stepped Adam over the frozen model's aux parameters, kept for readers of the reference's format -- copied to
``DIR/second_checkpoint_best_loss.pth.tar`` when the validation loss is the lowest so far.

Determinism: the plans are ``train_folder``'s (``random.Random(f"{seed}/{e}")``).  Stage 2 draws no noise, and every kernel on its path reduces in
a fixed order (no atomics in the enhancement kernels, the criterion or the optimiser; the warp's scatter backward does not run because the
reconstructions carry no gradient), so under ``--homography sidecar`` a run resumed with ``--resume`` reproduces the uninterrupted run's
parameters, Adam state and validation records BIT FOR BIT.

One JSON line per epoch; ``main(argv, log)`` returns the records, or 2 without a ROCm device.  One process, one device.
"""
from __future__ import annotations

import argparse
import sys

import torch

from . import folder_loop
from .folder_loop import _DTYPES, _Homography, _inputs, _kept, mse2psnr  # noqa: F401  (the shared pieces, under the names they had here)

_INFER_DTYPES = {"f16": torch.float16, "bf16": torch.bfloat16, "f32": torch.float32}
TRAIN_KEYS = ("loss", "mse_loss")
VALID_KEYS = ("loss", "mse_loss", "bpp_loss", "psnr1", "psnr2")
MS_SSIM_KEYS = ("ms_ssim1", "ms_ssim2")


def parser():
    p = argparse.ArgumentParser(prog="python -m hesic_amd.train_stage2",
                                description="Train Independent_EN on a frozen HSIC / HSICJoint's reconstructions of ROOT/train/{left,right} on the GPU.")
    folder_loop.add_shared_options(p, "second_checkpoint")
    p.add_argument("--dtype", choices=sorted(_DTYPES), default="bf16", help="the enhancer's training format")
    p.add_argument("--model", choices=("hesic", "joint"), default="hesic", help="the frozen model: HSIC (default) or HESIC+ (HSICJoint)")
    p.add_argument("--checkpoint", default=None, metavar="PATH|synthetic", help="the frozen model's weights (required; 'synthetic': the deterministic ones)")
    p.add_argument("--infer-dtype", choices=sorted(_INFER_DTYPES), default="f16", help="the format of the frozen forward")
    p.add_argument("--resume", default="none", metavar="PATH|none", help="a second_checkpoint*.pth.tar written by this command")
    return p


def train_epoch(trainer, cache, plan, ph, pw, homography=None):
    """One pass over ``plan``; returns ({key: mean over the steps}, steps, seconds).  The losses stay on the device until the end."""
    return folder_loop.train_epoch(trainer, cache, plan, ph, pw, TRAIN_KEYS, "train_stage2", homography)


def valid_batch_values(model, enhancer, x1, x2, h, lmbda, with_ms_ssim):
    """The per-batch values of the validation pass as one fp64 device vector, ``VALID_KEYS`` (then ``MS_SSIM_KEYS``) order."""
    from . import models
    out = model(x1, x2, h)
    en = enhancer(out["x1_hat"], out["x2_hat"], h)
    # rate_distortion's quantities, from the per-pair sums: ``hesic_rd_sums`` ends its sums in fp64 atomics, whose order -- and with it the last
    # bit of a record -- changes from run to run; ``pair_metrics`` adds in a fixed order, and so does the sum over the B pairs below
    pm = models.pair_metrics({"x1_hat": en["x1_hat"], "x2_hat": en["x2_hat"], "likelihoods": out["likelihoods"]}, x1, x2)
    n = pm["num_pixels"] * x1.shape[0]
    bpp = sum(v.sum() for k, v in pm.items() if k.startswith("bits_")).reshape(()) / n
    mse1, mse2 = pm["sse1"].sum().reshape(()) / (n * 3), pm["sse2"].sum().reshape(()) / (n * 3)
    mse = mse1 + mse2
    vals = [lmbda * 255 ** 2 * mse, mse, bpp, 10 * torch.log10(1 / mse1), 10 * torch.log10(1 / mse2)]
    if with_ms_ssim:
        hh, ww = x1.shape[-2:]
        vals += [models.ms_ssim(en["x1_hat"][..., :hh, :ww], x1).mean(), models.ms_ssim(en["x2_hat"][..., :hh, :ww], x2).mean()]
    return torch.stack(vals)


def test_epoch(model, enhancer, cache, plan, ph, pw, lmbda, homography=None):
    """newtrain6_real.py's ``test_epoch``: the mean over batches of the per-batch values, plus both printed forms of the PSNR."""
    model.eval()
    enhancer.eval()
    with_ms_ssim = min(ph, pw) > 160
    keys = VALID_KEYS + (MS_SSIM_KEYS if with_ms_ssim else ())
    rec = folder_loop.valid_epoch(cache, plan, ph, pw, keys, lambda x1, x2, h: valid_batch_values(model, enhancer, x1, x2, h, lmbda, with_ms_ssim),
                                  homography)
    enhancer.train()
    return rec


test_epoch.__test__ = False         # the reference's name for the validation pass, not a pytest case


def save_checkpoint(trainer, aux_optimizer, path, loss, epoch, seed):
    torch.save({"epoch": int(epoch), "state_dict": {k: v.detach().cpu().clone() for k, v in trainer.enhancer.state_dict().items()},
                "loss": float(loss), "optimizer": trainer.optimizer.state_dict(), "aux_optimizer": aux_optimizer.state_dict(),
                "seed": int(seed)}, path)


def _build(a, folder):
    """The frozen model, the enhancer and its trainer, a ``--resume`` checkpoint restored into them; ``folder_loop.run_epochs``' three callables."""
    from . import codec, models, train
    ph, pw = a.patch_size
    # the frozen model in the inference format (which stays the process's format outside the enhancer's forward / backward)
    net = codec.load_model(None if a.checkpoint == "synthetic" else a.checkpoint, _INFER_DTYPES[a.infer_dtype], device=folder.device, model=a.model)
    torch.manual_seed(folder.seed)                      # the enhancer's own initialisation, reproducibly
    enhancer = models.Independent_EN()
    if folder.resume is not None:
        enhancer.load_state_dict(folder.resume["state_dict"])
    enhancer = enhancer.to(folder.device).train()
    cls = train.GraphedEnhancerTrainer if a.graphed else train.EnhancerTrainer
    trainer = cls(net, enhancer, lr=a.learning_rate, lmbda=a.lmbda, train_dtype=_DTYPES[a.dtype], clip_max_norm=a.clip_max_norm,
                  skip_nonfinite=a.skip_nonfinite)
    aux_optimizer = torch.optim.Adam(net.aux_parameters(), lr=1e-3)          # never stepped (newtrain6_real.py:169-171): the file format's slot
    if folder.resume is not None:
        trainer.optimizer.load_state_dict(folder.resume["optimizer"])
        trainer.set_lr(a.learning_rate)
    return (lambda plan, homography: train_epoch(trainer, folder.tcache, plan, ph, pw, homography),
            lambda plan, homography: test_epoch(net, enhancer, folder.vcache, plan, ph, pw, a.lmbda, homography),
            lambda path, loss, epoch: save_checkpoint(trainer, aux_optimizer, path, loss, epoch, folder.seed))


def main(argv=None, log=print):
    """Returns the epochs' records (each also logged as one JSON line); 2 without a ROCm device."""
    p = parser()
    a = p.parse_args(argv)
    refusal = None if a.checkpoint else "--checkpoint is required: the frozen model's weights, or 'synthetic' for the deterministic ones"
    return folder_loop.run(p, a, "train_stage2", "second_checkpoint", _build, log, refusal)


if __name__ == "__main__":
    r = main()
    sys.exit(r if isinstance(r, int) else 0)

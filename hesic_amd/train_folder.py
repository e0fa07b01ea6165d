"""``python -m hesic_amd.train_folder ROOT``: train HSIC / HSICJoint on a stereo folder -- ``ywz/mywork/newtrain1.py``'s loop on the device.

    ROOT/train/{left,right}/            the training pairs, paired by file name (the loader's layout); ROOT/train/H/<stem>.npy|.txt sidecars
    ROOT/<--valid-split>/{left,right}/  the validation pairs (default ``test``)

    -e/--epochs 100  -lr/--learning-rate 1e-4  --aux-learning-rate 1e-3  --lambda 1e-2  --batch-size 16  --test-batch-size 64
    --patch-size 256 256  -n/--num-workers 3  --save  --seed S                                                  newtrain1.py's options
    --model hesic|joint  --homography sidecar|net|surf  --homography-checkpoint PATH  --distortion mse|ms-ssim  --clip-max-norm X
    --skip-nonfinite  --graphed  --dtype bf16|f32  --cache device|stream  --cache-gb G  --valid-split test  --resume PATH|none  --out DIR
    --augment hflip vflip swap   stereo-aware augmentation of the TRAINING batches (default: none)

Every pair is decoded once into device memory (``pair_cache.DevicePairCache``; ``--cache stream`` keeps the files on the host and uploads
crops per batch) and every batch of every epoch is one gather launch: the shared random crop, ToTensor and the homography of the crop, the
same bits the reference's ``ImageFolder`` + ``DataLoader`` produce.  The step is ``train.Trainer.step``, or with ``--graphed``
``train.GraphedTrainer.step``: the gather then writes straight into the captured step's static inputs, and the ragged last batch of an epoch is
dropped (and counted), because the captured step has one shape.

``--augment``: each named augmentation is applied to a training item with probability 1/2 -- ``hflip`` / ``vflip`` mirror both views,
``swap`` exchanges them -- by the gather launch itself (``hesic_pair_batch_gather_aug``, include/hesic_pair_augment.h), which also carries the
homography along (``F H F`` for a flip, the inverse for a swap); ``net`` and ``surf`` read the augmented pixels.  The flags of epoch ``e`` come
from a stream of their own, ``random.Random(f"{seed}/{e}/augment")``, so order and crops are those of a run without the option; the
validation batches are never augmented.  Each epoch's record then holds ``augmented: {"hflip": n, "vflip": n, "swap": n}``, the items that
got each.  Out of scope: the host ``ImageFolder`` loader and ``homography_train`` (another kernel) do not augment.

``--homography``: ``sidecar`` is newtrain1.py's ``d[2]`` (pairs without a sidecar are left out of the plan and counted: the reference's loader
returns a 2-tuple for them and its loop cannot use them); ``net`` is newtrain1_real.py:108-129, a frozen eval-mode HomographyNet on the
gathered crops (its random window from the epoch's random stream, after the plan's draws); ``surf`` is the reference loader's per-crop
``get_H``, ``stereo_h.estimate_homography`` on the gathered crops keyed by the dataset indices (invalid pairs get the identity and are
counted).

Per epoch: train, then ``test_epoch`` -- eval mode under ``no_grad``; per batch ``loss``, ``mse_loss``, ``bpp_loss``, ``aux_loss`` as the
reference's criterion defines them and ``psnr1`` / ``psnr2`` (newtrain1_real.py:83-84), from ``models.rate_distortion``'s sums; the reported value
is the mean over batches of the per-batch values (``AverageMeter.update(val)`` with n = 1), added up on the device and read back once; both
printed forms of the PSNR are in the record: ``psnr`` = (psnr1.avg + psnr2.avg) / 2 and ``psnr_of_mse`` = mse2psnr(mse_loss.avg / 2)
(newtrain1.py:141).  With ``--save``: ``DIR/checkpoint.pth.tar`` = the reference's ``{"epoch", "state_dict", "loss", "optimizer",
"aux_optimizer"}`` plus ``"seed"`` (``state_dict`` on the host under the model's own keys: the reference's
``net.load_state_dict(model["state_dict"])`` and ``codec.load_model(checkpoint=...)`` read it), copied to
``DIR/checkpoint_best_loss.pth.tar`` when the validation loss is the lowest so far.  ``"epoch"`` is the index of the epoch just finished.

Determinism: the order and the crops of epoch ``e`` come from ``random.Random(f"{seed}/{e}")``, the validation crops from a stream keyed by the
seed alone (``pair_cache.epoch_plan``).  ``--epochs`` is the TOTAL; ``--resume`` restores the model and both optimisers and continues at
``epoch + 1`` with that epoch's own plan, so a resumed run is fed the batches of the uninterrupted one.  Bit-identical PARAMETERS after a
resume are NOT promised: the quantisation noise comes from torch's device generator, whose state the checkpoint does not hold.

One JSON line per epoch; ``main(argv, log)`` returns the records, or 2 without a ROCm device.  One process, one device: a sampler per rank is
out of scope.  The options, refusals, epoch passes and the run loop that ``train_stage2`` has too live in ``folder_loop``.
"""
from __future__ import annotations

import argparse
import sys

import torch

from . import folder_loop
from .folder_loop import _DTYPES, _Homography, _inputs, _kept, mse2psnr  # noqa: F401  (the shared pieces, under the names they had here)

VALID_KEYS = ("loss", "mse_loss", "bpp_loss", "aux_loss", "psnr1", "psnr2")
TRAIN_KEYS = ("loss", "mse_loss", "bpp_loss", "aux_loss")


def parser():
    p = argparse.ArgumentParser(prog="python -m hesic_amd.train_folder", description="Train HSIC / HSICJoint on ROOT/train/{left,right} on the GPU.")
    folder_loop.add_shared_options(p, "checkpoint")
    p.add_argument("--aux-learning-rate", type=float, default=1e-3)
    p.add_argument("--model", choices=("hesic", "joint"), default="hesic", help="hesic: HSIC (default); joint: HESIC+ (HSICJoint)")
    p.add_argument("--distortion", choices=("mse", "ms-ssim"), default="mse")
    p.add_argument("--dtype", choices=sorted(_DTYPES), default="bf16")
    p.add_argument("--resume", default="none", metavar="PATH|none")
    return p


def train_epoch(trainer, cache, plan, ph, pw, homography=None):
    """One pass over ``plan``; returns ({key: mean over the steps}, steps, seconds).  The losses stay on the device until the end."""
    return folder_loop.train_epoch(trainer, cache, plan, ph, pw, TRAIN_KEYS, "train_folder", homography)


def valid_batch_values(model, x1, x2, h, lmbda, distortion="mse"):
    """The per-batch values of ``test_epoch`` as one fp64 device vector in ``VALID_KEYS`` order, from ``models.rate_distortion``'s sums."""
    from . import functional as Fn
    from . import models
    out = model(x1, x2, h)
    rd = models.rate_distortion(out, x1, x2)
    n = rd["num_pixels"]
    bpp = sum(v for k, v in rd.items() if k.startswith("bits_")).reshape(()) / n
    mse1, mse2 = rd["sse1"].reshape(()) / (n * 3), rd["sse2"].reshape(()) / (n * 3)
    mse = mse1 + mse2
    if distortion == "mse":
        loss = lmbda * 255 ** 2 * mse + bpp
    else:
        loss = Fn.rd_loss(out, x1, x2, lmbda, distortion=distortion)["loss"].detach().reshape(()).double()
    return torch.stack([loss, mse, bpp, model.aux_loss().detach().reshape(()).double(), 10 * torch.log10(1 / mse1), 10 * torch.log10(1 / mse2)])


def test_epoch(model, cache, plan, ph, pw, lmbda, distortion="mse", homography=None):
    """newtrain1.py's ``test_epoch``: the mean over batches of the per-batch values, plus both printed forms of the PSNR."""
    from . import functional as Fn
    model.eval()
    Fn.invalidate_weight_cache()
    rec = folder_loop.valid_epoch(cache, plan, ph, pw, VALID_KEYS, lambda x1, x2, h: valid_batch_values(model, x1, x2, h, lmbda, distortion),
                                  homography)
    model.train()
    return rec


test_epoch.__test__ = False         # the reference's name for the validation pass, not a pytest case


def save_checkpoint(trainer, path, loss, epoch, seed):
    torch.save({"epoch": int(epoch), "state_dict": {k: v.detach().cpu().clone() for k, v in trainer.model.state_dict().items()},
                "loss": float(loss), "optimizer": trainer.optimizer.state_dict(), "aux_optimizer": trainer.aux_optimizer.state_dict(),
                "seed": int(seed)}, path)


def _build(a, folder):
    """The model and its trainer, a ``--resume`` checkpoint restored into both; ``folder_loop.run_epochs``' three callables."""
    import hesic_amd
    from . import models, train
    ph, pw = a.patch_size
    hesic_amd.set_compute_dtype(_DTYPES[a.dtype])
    torch.manual_seed(folder.seed)                      # the constructor's own initialisation and the noise stream, reproducibly
    net = {"hesic": models.HSIC, "joint": models.HSICJoint}[a.model]()
    if folder.resume is not None:
        net.load_state_dict(folder.resume["state_dict"])
    net = net.to(folder.device).train()
    cls = train.GraphedTrainer if a.graphed else train.Trainer
    trainer = cls(net, lr=a.learning_rate, aux_lr=a.aux_learning_rate, lmbda=a.lmbda, distortion=a.distortion,
                  clip_max_norm=a.clip_max_norm, skip_nonfinite=a.skip_nonfinite)
    if folder.resume is not None:
        trainer.optimizer.load_state_dict(folder.resume["optimizer"])
        trainer.aux_optimizer.load_state_dict(folder.resume["aux_optimizer"])
        trainer.set_lr(a.learning_rate, a.aux_learning_rate)
    return (lambda plan, homography: train_epoch(trainer, folder.tcache, plan, ph, pw, homography),
            lambda plan, homography: test_epoch(net, folder.vcache, plan, ph, pw, a.lmbda, a.distortion, homography),
            lambda path, loss, epoch: save_checkpoint(trainer, path, loss, epoch, folder.seed))


def main(argv=None, log=print):
    """Returns the epochs' records (each also logged as one JSON line); 2 without a ROCm device."""
    p = parser()
    return folder_loop.run(p, p.parse_args(argv), "train_folder", "checkpoint", _build, log)


if __name__ == "__main__":
    r = main()
    sys.exit(r if isinstance(r, int) else 0)

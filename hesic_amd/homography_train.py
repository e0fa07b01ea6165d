"""``python -m hesic_amd.homography_train ROOT``: train HomographyNet on a stereo folder -- ``udh/udh/QHtrain.py``'s loop on the device.

    ROOT/train/{left,right}/   the training pairs, paired by file name (the loader's layout)
    ROOT/<--valid-split>/{left,right}/   the validation pairs (default ``test``)

    --batch_size 16 --learning_rate 1e-4 --epochs 10 --rho 45 --picsize 256 --patchsize 128      QHtrain's options
    --crop H W            one random crop offset shared by both views (default: the whole image)
    --seed 0  --resume PATH|none  --out DIR  --clip-max-norm X  --skip-nonfinite

The host only reads and crops: a batch is stacked as uint8 and uploaded as bytes, and ``HomographyTrainer.step_pairs`` turns it into the
net's inputs in one launch (resize, normalise, grey, random window), runs the forward, the photometric loss, the backward and Adam.  Pairs of
one size share a batch (as in ``codec.encode_folder``).  Per epoch: shuffle and train, then the validation loss -- eval mode under
``no_grad``, the mean of the per-batch losses, added up on the device and read back once --, ``DIR/checkpoint.pth.tar``, and a copy as
``DIR/checkpoint_best_loss.pth.tar`` when that loss is the lowest so far (QHtrain.py:121-133).

A checkpoint holds ``{"state_dict", "loss", "optimizer", "dropout", "epoch", "seed"}``; the ``state_dict`` keys carry the reference's
``model.`` prefix, so the `_real` scripts load the file as they load ``homo_best.pth.tar`` (``homography.load_checkpoint`` reads both forms).

Determinism: the shuffle, the crop offsets and the windows of epoch ``e`` come from a ``random.Random`` keyed by ``(seed, e)``, the validation
draws from one keyed by the seed alone (every epoch is judged on the same windows).  ``--epochs`` is the TOTAL number of epochs, as in QHtrain:
``--epochs 1`` followed by ``--resume DIR/checkpoint.pth.tar --epochs 2`` ends in the parameters of one ``--epochs 2`` run, bit for bit (up
to 64 rows per batch, the trainer's own condition).
"""
from __future__ import annotations

import argparse
import json
import os
import random
import shutil
import sys
import time
from pathlib import Path

import numpy as np
import torch


def list_pairs(root, split):
    """[(left path, right path, (width, height))] of ROOT/<split>, in sorted order."""
    from .codec import _pairs
    from .stereo_h import _image_size
    out = []
    for _, lf, rf, _ in _pairs(root, split):
        sa, sb = _image_size(lf), _image_size(rf)
        if sa != sb:
            raise ValueError(f"{os.path.basename(lf)}: the two views differ in size ({sa} vs {sb})")
        out.append((lf, rf, sa))
    return out


def _check_crop(pairs, crop):
    if crop is not None:
        for lf, _, (w, h) in pairs:
            if crop[0] > h or crop[1] > w:
                raise ValueError(f"{os.path.basename(lf)}: crop {tuple(crop)} larger than the image ({h}, {w})")


def batches(pairs, batch_size, crop, rng, shuffle):
    """Lists of pairs that share a batch: pairs of one (cropped) size, in ``rng``'s order when ``shuffle``."""
    groups = {}
    for p in pairs:
        groups.setdefault(tuple(crop) if crop is not None else (p[2][1], p[2][0]), []).append(p)
    out = []
    for key in sorted(groups):
        items = list(groups[key])
        if shuffle:
            rng.shuffle(items)
        out += [items[i:i + batch_size] for i in range(0, len(items), batch_size)]
    if shuffle:
        rng.shuffle(out)
    return out


def load_batch(items, crop, rng, device):
    """The two views of ``items`` as uint8 (B,3,H,W) device tensors (views of the uploaded (B,H,W,3) bytes); one crop offset per pair."""
    from .compressai.datasets import _read_rgb
    a, b = [], []
    for lf, rf, (w, h) in items:
        i1, i2 = _read_rgb(lf), _read_rgb(rf)
        if crop is not None:
            ch, cw = crop
            y0, x0 = rng.randint(0, h - ch), rng.randint(0, w - cw)
            i1, i2 = i1[y0:y0 + ch, x0:x0 + cw], i2[y0:y0 + ch, x0:x0 + cw]
        a.append(i1)
        b.append(i2)
    x1 = torch.from_numpy(np.stack(a)).to(device, non_blocking=True).permute(0, 3, 1, 2)
    x2 = torch.from_numpy(np.stack(b)).to(device, non_blocking=True).permute(0, 3, 1, 2)
    return x1, x2


def train_epoch(trainer, pairs, a, rng, device):
    """One pass over ``pairs``; returns (mean training loss, steps, seconds).  The losses stay on the device until the end."""
    total, n, t0 = torch.zeros((), device=device), 0, time.time()
    for items in batches(pairs, a.batch_size, a.crop, rng, True):
        x1, x2 = load_batch(items, a.crop, rng, device)
        total += trainer.step_pairs(x1, x2, None, a.picsize, a.rho, rng)["loss"]
        n += 1
    return float(total) / max(n, 1), n, time.time() - t0


def validate(trainer, pairs, a, rng, device):
    total, n = torch.zeros((), device=device), 0
    for items in batches(pairs, a.batch_size, a.crop, rng, False):
        x1, x2 = load_batch(items, a.crop, rng, device)
        total += trainer.evaluate_pairs(x1, x2, None, a.picsize, a.rho, rng)
        n += 1
    return float(total) / max(n, 1)


def save_checkpoint(trainer, path, loss, epoch, seed):
    from . import homography
    sd = trainer.state_dict()
    torch.save({"state_dict": homography.checkpoint_state_dict(trainer.net), "loss": float(loss), "optimizer": sd["optimizer"],
                "dropout": tuple(sd["dropout"]), "epoch": int(epoch), "seed": int(seed)}, path)


def parser():
    p = argparse.ArgumentParser(prog="python -m hesic_amd.homography_train", description="Train HomographyNet on ROOT/train/{left,right} on the GPU.")
    p.add_argument("root")
    p.add_argument("--valid-split", default="test")
    p.add_argument("--batch_size", type=int, default=16)
    p.add_argument("--learning_rate", type=float, default=1e-4)
    p.add_argument("--epochs", type=int, default=10, help="total number of epochs (a resumed run continues up to it)")
    p.add_argument("--rho", type=int, default=45)
    p.add_argument("--picsize", type=int, default=256)
    p.add_argument("--patchsize", type=int, default=128)
    p.add_argument("--crop", type=int, nargs=2, metavar=("H", "W"), default=None)
    p.add_argument("--seed", type=int, default=None, help="default: 0, or the seed of the --resume checkpoint")
    p.add_argument("--resume", default="none", metavar="PATH|none")
    p.add_argument("--out", default=".")
    p.add_argument("--clip-max-norm", type=float, default=None)
    p.add_argument("--skip-nonfinite", action="store_true")
    return p


def main(argv=None, log=print):
    """Returns the epochs' records ({"epoch", "train_loss", "valid_loss", "best", "steps", "seconds_per_step"}, each also logged as one JSON
    line); 2 without a ROCm device."""
    from . import homography, train
    p = parser()
    a = p.parse_args(argv)
    if a.batch_size < 1 or a.epochs < 0:
        p.error("--batch_size must be positive and --epochs not negative")
    if a.patchsize % 8 or not 8 <= a.patchsize <= a.picsize:
        p.error("--patchsize must be a multiple of 8, at most --picsize")
    if a.rho < 0:
        p.error("--rho must not be negative")
    if not torch.cuda.is_available():
        print("homography_train: needs a ROCm device (the training kernels have no CPU path)", file=sys.stderr)
        return 2
    device = torch.device("cuda", torch.cuda.current_device())
    train_pairs, valid_pairs = list_pairs(a.root, "train"), list_pairs(a.root, a.valid_split)
    _check_crop(train_pairs + valid_pairs, a.crop)
    resume = None if a.resume in (None, "none") else torch.load(a.resume, map_location="cpu")
    seed = a.seed if a.seed is not None else (int(resume["seed"]) if resume is not None else 0)
    if resume is None:
        torch.manual_seed(seed)                     # the constructor's own initialisation, reproducibly
    net = homography.Net(patch_size=a.patchsize).to(device)
    trainer = train.HomographyTrainer(net, lr=a.learning_rate, seed=seed, clip_max_norm=a.clip_max_norm, skip_nonfinite=a.skip_nonfinite)
    out = Path(a.out)
    out.mkdir(parents=True, exist_ok=True)
    last, best = out / "checkpoint.pth.tar", out / "checkpoint_best_loss.pth.tar"
    first_epoch, best_loss = 0, float("inf")
    if resume is not None:
        trainer.load_state_dict({"state_dict": homography.net_state_dict(resume["state_dict"]), "optimizer": resume["optimizer"],
                                 "dropout": resume["dropout"]})
        trainer.set_lr(a.learning_rate)
        first_epoch, best_loss = int(resume["epoch"]) + 1, float(resume["loss"])
        prev_best = Path(a.resume).with_name(best.name)
        if prev_best.is_file():
            best_loss = min(best_loss, float(torch.load(prev_best, map_location="cpu")["loss"]))
            if prev_best.resolve() != best.resolve() and not best.is_file():
                shutil.copyfile(prev_best, best)
    history = []
    for epoch in range(first_epoch, a.epochs):
        train_loss, steps, secs = train_epoch(trainer, train_pairs, a, random.Random(f"{seed}/{epoch}"), device)
        valid_loss = validate(trainer, valid_pairs, a, random.Random(f"{seed}/valid"), device)
        save_checkpoint(trainer, last, valid_loss, epoch, seed)
        is_best = valid_loss < best_loss
        if is_best or not best.is_file():
            best_loss = min(best_loss, valid_loss)
            shutil.copyfile(last, best)
        rec = {"epoch": epoch, "train_loss": train_loss, "valid_loss": valid_loss, "best": bool(is_best), "steps": steps,
               "seconds_per_step": secs / max(steps, 1)}
        history.append(rec)
        log(json.dumps(rec))
    return history


if __name__ == "__main__":
    r = main()
    sys.exit(r if isinstance(r, int) else 0)

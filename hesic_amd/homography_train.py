"""``python -m hesic_amd.homography_train ROOT``: train HomographyNet on a stereo folder -- ``udh/udh/QHtrain.py``'s loop on the device.

    ROOT/train/{left,right}/   the training pairs, paired by file name (the loader's layout)
    ROOT/<--valid-split>/{left,right}/   the validation pairs (default ``test``)

    --batch_size 16 --learning_rate 1e-4 --epochs 10 --rho 45 --picsize 256 --patchsize 128      QHtrain's options
    --crop H W            one random crop offset shared by both views (default: the whole image)
    --seed 0  --resume PATH|none  --out DIR  --clip-max-norm X  --skip-nonfinite
    --cache host|device|stream  --cache-gb G  -n/--num-workers 3  --mix-sizes
    --supervision photometric|synthetic  --graphed

``--cache host`` (the default): the host reads, decodes and crops every batch of every epoch on one thread; a batch is stacked as uint8
and uploaded as bytes, and ``HomographyTrainer.step_pairs`` turns it into the net's inputs in one launch (resize, normalise, grey, random
window), runs the forward, the photometric loss, the backward and Adam.  Pairs of one size share a batch (as in ``codec.encode_folder``).
``--cache device``: every pair is decoded ONCE into a uint8 device arena (``pair_cache.DevicePairCache``, one per split, ``-n`` host threads,
``--cache-gb`` its memory budget) and a batch's inputs come straight from the stored bytes in one launch
(``DevicePairCache.homonet_batch``, include/hesic_homonet_items.h), followed by ``HomographyTrainer.step`` -- the call ``step_pairs`` ends
in.  ``--cache stream`` keeps the files on the host (a set that does not fit): per batch ``-n`` threads read and crop, the crops are
uploaded into a reused slab and the same kernel runs on it.  ``draw_batch`` consumes the random stream exactly as the host route does, and
the kernel gives the host route's bits, so losses, parameters and checkpoints are the same in all three modes and a run may be resumed under
another one.  ``--mix-sizes`` (``device`` / ``stream`` only): the net sees every view resized to ``picsize``², so pairs of ALL sizes form one
pool instead of one group per image size -- fewer, fuller batches on a folder of mixed sizes (and other batches than without the flag).
Per epoch: shuffle and train, then the validation loss -- eval mode under
``no_grad``, the mean of the per-batch losses, added up on the device and read back once --, ``DIR/checkpoint.pth.tar``, and a copy as
``DIR/checkpoint_best_loss.pth.tar`` when that loss is the lowest so far (QHtrain.py:121-133).

A checkpoint holds ``{"state_dict", "loss", "optimizer", "dropout", "epoch", "seed"}``; the ``state_dict`` keys carry the reference's
``model.`` prefix, so the `_real` scripts load the file as they load ``homo_best.pth.tar`` (``homography.load_checkpoint`` reads both forms).

``--supervision synthetic`` (``--cache device|stream`` only) trains on pairs with a KNOWN answer instead: every batch is a fresh random
perspective warp of the LEFT views -- ``homography.draw_deltas`` moves each window corner by up to ``rho`` pixels,
``DevicePairCache.homonet_synth_batch`` (include/hesic_homonet_synth.h) makes the frame, its warp and both windows from the stored bytes --
and ``HomographyTrainer.step_supervised`` minimises the MSE between the net's deltas and the drawn ones: the finish of the reference's
``SyntheticDataset`` (udh/udh/dataset.py), and the augmentation a homography net wants.  The deltas come from a stream of their own,
``random.Random(f"{seed}/{epoch}/synth")`` (validation: ``f"{seed}/valid/synth"``), so the order, crops and windows of an epoch are those of
a photometric run with the same seed.  The records then carry ``"supervision"``, ``"valid_loss"`` -- the supervised MSE on synthetic
validation pairs, which the best checkpoint follows --, ``"valid_corner_error"`` (the mean over the pairs of the mean corner error, in
pixels of the ``picsize`` frame), ``"identity_corner_error"`` (the same for a net that answers zero: the figure to beat) and
``"valid_photometric"``, the photometric validation loss on the REAL right views, which shows whether the pre-training transfers; the
checkpoints gain ``"supervision"``.  ``--resume`` across supervisions is allowed -- synthetic pre-training, then photometric fine-tuning, is
the intended use --; the two losses are not comparable, so the lowest validation loss so far then starts again at +inf and the first
epoch's checkpoint becomes the best one.

``--graphed`` (``--cache device|stream`` only) trains with ``train.GraphedHomographyTrainer``: after three eager steps the step of the
run's batch shape is one HIP-graph launch, the dropout state lives on the device, and the batch's one prep launch writes straight into the
graph's static inputs (``out=``).  An epoch's ragged last batch -- and every other shape -- runs eagerly through the same kernels; validation
is eager.  Records, checkpoints and ``--resume`` are bit for bit those of a run without the flag, and a resume may switch it on or off.
The device is busy for all but a few percent of this step, so the gain is small: 4.82 -> 4.73 ms per step at batch 16, nothing measurable
at batch 64 (profiles/homography_graphed_bench.json).

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

from .folder_loop import resume_position


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


def batches(pairs, batch_size, crop, rng, shuffle, mix_sizes=False):
    """Lists of pairs that share a batch: pairs of one (cropped) size -- of any size under ``mix_sizes`` --, in ``rng``'s order when
    ``shuffle``."""
    groups = {}
    for p in pairs:
        groups.setdefault(() if mix_sizes else tuple(crop) if crop is not None else (p[2][1], p[2][0]), []).append(p)
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


def draw_batch(items, crop, rng, picsize, patchsize, rho):
    """``(origins, sizes, windows)`` of one batch for ``DevicePairCache.homonet_batch``: ``origins[i] = (y0, x0)``, ``sizes[i] = (ch, cw)``
    (``None`` without ``crop``: the whole images), ``windows[i] = (wx, wy)``.  A pure host function that consumes ``rng`` exactly as the host
    route does: first ``load_batch``'s draws -- per pair ``randint(0, h - ch)`` then ``randint(0, w - cw)``, only with ``crop`` --, then
    ``homography.window_origins``' for the batch."""
    from . import homography
    origins, sizes = [(0, 0)] * len(items), None
    if crop is not None:
        ch, cw = crop
        origins = [(rng.randint(0, h - ch), rng.randint(0, w - cw)) for _, _, (w, h) in items]
        sizes = [(ch, cw)] * len(items)
    return origins, sizes, homography.window_origins(len(items), None, picsize, patchsize, rho, rng)


def cached_inputs(cache, items, a, rng, out=None):
    """``(grey1, patch1, patch2, corners)`` of the batch ``items`` from the split's ``DevicePairCache``, one launch: what ``step_pairs`` /
    ``evaluate_pairs`` prepare from ``load_batch``'s upload.  ``out``: ``homonet_batch``'s five tensors to write into."""
    origins, sizes, windows = draw_batch(items, a.crop, rng, a.picsize, a.patchsize, a.rho)
    grey1, _, patch1, patch2, corners = cache.homonet_batch([cache.index_of[lf] for lf, _, _ in items], origins, sizes, windows, a.picsize,
                                                            a.patchsize, out=out)
    return grey1, patch1, patch2, corners


def synthetic_inputs(cache, items, a, rng, srng, out=None):
    """``(patch_a, patch_b, delta)`` of a synthetic-warp batch on the left views of ``items``: ``draw_batch`` on ``rng`` as ``cached_inputs``
    does, the corner offsets from ``srng``, one call of ``DevicePairCache.homonet_synth_batch`` (``out``: its seven tensors to write into)."""
    from . import homography
    origins, sizes, windows = draw_batch(items, a.crop, rng, a.picsize, a.patchsize, a.rho)
    deltas = homography.draw_deltas(len(items), windows, a.patchsize, a.rho, srng)
    _, patch_a, _, delta, _, _, patch_b = cache.homonet_synth_batch([cache.index_of[lf] for lf, _, _ in items], origins, sizes, windows, deltas,
                                                                    a.picsize, a.patchsize, out=out)
    return patch_a, patch_b, delta


def graph_outputs(trainer, kind, batch, picsize, spare):
    """The ``out=`` tuple that makes a batch's prep launch write into the static inputs of ``trainer``'s ``kind`` slot, or ``None`` -- an
    eager trainer, a slot not staged yet, a batch of another size (it runs eagerly).  The outputs the step does not read go to tensors kept
    in ``spare``."""
    static = trainer.static_inputs(kind) if hasattr(trainer, "static_inputs") else None
    if static is None or static[0].shape[0] != batch:
        return None
    if kind == "step":
        img_a, patch_a, patch_b, corners = static
        if kind not in spare:
            spare[kind] = torch.empty_like(img_a)
        return img_a, spare[kind], patch_a, patch_b, corners
    patch_a, patch_b, delta = static
    if kind not in spare:
        S, dev = picsize, patch_a.device
        spare[kind] = (torch.empty((batch, 1, S, S), device=dev), torch.empty((batch, 4, 2), device=dev),
                       torch.empty((batch, 9), dtype=torch.float64, device=dev), torch.empty((batch, 1, S, S), device=dev))
    grey_a, corners, h, grey_b = spare[kind]
    return grey_a, patch_a, corners, delta, h, grey_b, patch_b


def train_epoch(trainer, pairs, a, rng, device, cache=None, srng=None, spare=None):
    """One pass over ``pairs`` (from ``cache`` when given, else read on the host); returns (mean training loss, steps, seconds).  The losses
    stay on the device until the end.  ``srng``: the deltas' stream under ``--supervision synthetic``, which makes every step a supervised one.
    ``spare``: a dict that lives as long as a graphed ``trainer`` (``graph_outputs``)."""
    total, n, t0 = torch.zeros((), device=device), 0, time.time()
    spare = {} if spare is None else spare
    for items in batches(pairs, a.batch_size, a.crop, rng, True, cache is not None and a.mix_sizes):
        if srng is not None:
            out = graph_outputs(trainer, "supervised", len(items), a.picsize, spare)
            total += trainer.step_supervised(*synthetic_inputs(cache, items, a, rng, srng, out))["loss"]
        elif cache is None:
            x1, x2 = load_batch(items, a.crop, rng, device)
            total += trainer.step_pairs(x1, x2, None, a.picsize, a.rho, rng)["loss"]
        else:
            out = graph_outputs(trainer, "step", len(items), a.picsize, spare)
            total += trainer.step(*cached_inputs(cache, items, a, rng, out))["loss"]
        n += 1
    return float(total) / max(n, 1), n, time.time() - t0


def validate(trainer, pairs, a, rng, device, cache=None):
    total, n = torch.zeros((), device=device), 0
    for items in batches(pairs, a.batch_size, a.crop, rng, False, cache is not None and a.mix_sizes):
        if cache is None:
            x1, x2 = load_batch(items, a.crop, rng, device)
            total += trainer.evaluate_pairs(x1, x2, None, a.picsize, a.rho, rng)
        else:
            total += trainer.evaluate(*cached_inputs(cache, items, a, rng))
        n += 1
    return float(total) / max(n, 1)


def validate_synthetic(trainer, pairs, a, rng, srng, device, cache):
    """``(supervised MSE, mean corner error, identity corner error)`` on synthetic warps of the validation pairs' left views: the mean of the
    per-batch losses and the means over the PAIRS of the two corner errors, added up on the device and read back once."""
    from . import homography
    total, nb, n = torch.zeros(3, dtype=torch.float64, device=device), 0, 0
    for items in batches(pairs, a.batch_size, a.crop, rng, False, a.mix_sizes):
        patch_a, patch_b, delta = synthetic_inputs(cache, items, a, rng, srng)
        loss, err = trainer.evaluate_supervised(patch_a, patch_b, delta)
        ident = homography.corner_error(torch.zeros_like(delta), delta)
        total += torch.stack([loss.double(), err.double().sum(), ident.double().sum()])
        nb += 1
        n += len(items)
    loss, err, ident = total.tolist()
    return loss / max(nb, 1), err / max(n, 1), ident / max(n, 1)


def build_cache(root, split, pairs, a):
    """The split's ``DevicePairCache`` in ``--cache``'s mode, with ``index_of``: left file -> pair index (the listing is ``list_pairs``')."""
    from . import pair_cache
    budget = None if a.cache_gb is None else int(a.cache_gb * 2 ** 30)
    cache = pair_cache.DevicePairCache(root, split, mode=a.cache, budget_bytes=budget, workers=a.num_workers)
    if [f[0] for f in cache.files] != [p[0] for p in pairs]:
        raise RuntimeError(f"homography_train: {split}: the folder changed while it was listed")
    cache.index_of = {lf: i for i, (lf, _) in enumerate(cache.files)}
    return cache


def save_checkpoint(trainer, path, loss, epoch, seed, supervision="photometric"):
    from . import homography
    sd = trainer.state_dict()
    ckpt = {"state_dict": homography.checkpoint_state_dict(trainer.net), "loss": float(loss), "optimizer": sd["optimizer"],
            "dropout": tuple(sd["dropout"]), "epoch": int(epoch), "seed": int(seed)}
    if supervision != "photometric":              # a photometric checkpoint is the file it always was
        ckpt["supervision"] = supervision
    torch.save(ckpt, path)


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
    p.add_argument("--cache", choices=("host", "device", "stream"), default="host",
                   help="host: read and decode every batch; device: decode once into device memory; stream: read per batch on -n threads")
    p.add_argument("--cache-gb", type=float, default=None, help="device-memory budget of the decoded pairs (default: half of the free memory)")
    p.add_argument("-n", "--num-workers", type=int, default=3, help="host threads that decode image files (--cache device|stream)")
    p.add_argument("--mix-sizes", action="store_true", help="pairs of all sizes share batches (--cache device|stream)")
    p.add_argument("--supervision", choices=("photometric", "synthetic"), default="photometric",
                   help="photometric: the loss on the real pairs; synthetic: known random warps of the left views, MSE on the corner deltas "
                        "(--cache device|stream)")
    p.add_argument("--graphed", action="store_true",
                   help="record the training step into a HIP graph and replay it (--cache device|stream); the same bits as without the flag. "
                        "Measured at batch 16: about 2 %% faster per step on the folder loop (4 %% on the step alone); at batch 64, and under "
                        "--supervision synthetic, not faster than the eager step by more than its own run-to-run spread")
    return p


def main(argv=None, log=print):
    """Returns the epochs' records ({"epoch", "train_loss", "valid_loss", "best", "steps", "seconds_per_step"}, each also logged as one JSON
    line; ``--cache device|stream`` add "cache" and, in the run's first record, "decode_seconds"; ``--supervision synthetic`` adds
    "supervision", "valid_corner_error", "identity_corner_error" and "valid_photometric"); 2 without a ROCm device."""
    from . import homography, train
    p = parser()
    a = p.parse_args(argv)
    if a.batch_size < 1 or a.epochs < 0:
        p.error("--batch_size must be positive and --epochs not negative")
    if a.patchsize % 8 or not 8 <= a.patchsize <= a.picsize:
        p.error("--patchsize must be a multiple of 8, at most --picsize")
    if a.rho < 0:
        p.error("--rho must not be negative")
    if a.mix_sizes and a.cache == "host":
        p.error("--mix-sizes needs --cache device or --cache stream (the host route uploads a batch as one tensor of one size)")
    if a.supervision == "synthetic" and a.cache == "host":
        p.error("--supervision synthetic needs --cache device or --cache stream (the warps are made from the stored bytes on the device)")
    if a.graphed and a.cache == "host":
        p.error("--graphed needs --cache device or --cache stream (the host route's step_pairs draws its windows between the launches)")
    if a.num_workers < 1 or (a.cache_gb is not None and a.cache_gb <= 0):
        p.error("--num-workers and --cache-gb must be positive")
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
    trainer = (train.GraphedHomographyTrainer if a.graphed else train.HomographyTrainer)(
        net, lr=a.learning_rate, seed=seed, clip_max_norm=a.clip_max_norm, skip_nonfinite=a.skip_nonfinite)
    out = Path(a.out)
    out.mkdir(parents=True, exist_ok=True)
    last, best = out / "checkpoint.pth.tar", out / "checkpoint_best_loss.pth.tar"
    if resume is not None:
        trainer.load_state_dict({"state_dict": homography.net_state_dict(resume["state_dict"]), "optimizer": resume["optimizer"],
                                 "dropout": resume["dropout"]})
        trainer.set_lr(a.learning_rate)
    first_epoch, best_loss = resume_position(resume, a.resume, best, True)      # this command always saves
    if resume is not None and resume.get("supervision", "photometric") != a.supervision:
        best_loss = float("inf")                    # the other supervision's loss is not comparable: the first epoch's checkpoint is the best
    tcache = vcache = None
    if a.cache != "host" and first_epoch < a.epochs:
        tcache = build_cache(a.root, "train", train_pairs, a)
        vcache = tcache if a.valid_split == "train" else build_cache(a.root, a.valid_split, valid_pairs, a)
    history, synthetic, spare = [], a.supervision == "synthetic", {}
    for epoch in range(first_epoch, a.epochs):
        train_loss, steps, secs = train_epoch(trainer, train_pairs, a, random.Random(f"{seed}/{epoch}"), device, tcache,
                                              random.Random(f"{seed}/{epoch}/synth") if synthetic else None, spare)
        if synthetic:
            valid_loss, corner_err, identity_err = validate_synthetic(trainer, valid_pairs, a, random.Random(f"{seed}/valid"),
                                                                      random.Random(f"{seed}/valid/synth"), device, vcache)
            valid_photometric = validate(trainer, valid_pairs, a, random.Random(f"{seed}/valid"), device, vcache)
        else:
            valid_loss = validate(trainer, valid_pairs, a, random.Random(f"{seed}/valid"), device, vcache)
        save_checkpoint(trainer, last, valid_loss, epoch, seed, a.supervision)
        is_best = valid_loss < best_loss
        if is_best or not best.is_file():
            best_loss = min(best_loss, valid_loss)
            shutil.copyfile(last, best)
        rec = {"epoch": epoch, "train_loss": train_loss, "valid_loss": valid_loss, "best": bool(is_best), "steps": steps,
               "seconds_per_step": secs / max(steps, 1)}
        if synthetic:
            rec.update({"supervision": a.supervision, "valid_corner_error": corner_err, "identity_corner_error": identity_err,
                        "valid_photometric": valid_photometric})
        if tcache is not None:
            rec["cache"] = a.cache
            if not history:
                rec["decode_seconds"] = tcache.decode_seconds + (vcache.decode_seconds if vcache is not tcache else 0.0)
        history.append(rec)
        log(json.dumps(rec))
    return history


if __name__ == "__main__":
    r = main()
    sys.exit(r if isinstance(r, int) else 0)

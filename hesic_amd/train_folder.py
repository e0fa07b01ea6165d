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
out of scope.
"""
from __future__ import annotations

import argparse
import json
import math
import shutil
import sys
import time
from pathlib import Path

import torch

_DTYPES = {"bf16": torch.bfloat16, "f32": torch.float32}
VALID_KEYS = ("loss", "mse_loss", "bpp_loss", "aux_loss", "psnr1", "psnr2")
TRAIN_KEYS = ("loss", "mse_loss", "bpp_loss", "aux_loss")


def mse2psnr(mse):
    return 10 * math.log10(1 / mse)


def parser():
    p = argparse.ArgumentParser(prog="python -m hesic_amd.train_folder", description="Train HSIC / HSICJoint on ROOT/train/{left,right} on the GPU.")
    p.add_argument("root")
    p.add_argument("-e", "--epochs", type=int, default=100, help="total number of epochs (a resumed run continues up to it)")
    p.add_argument("-lr", "--learning-rate", type=float, default=1e-4)
    p.add_argument("--aux-learning-rate", type=float, default=1e-3)
    p.add_argument("--lambda", dest="lmbda", type=float, default=1e-2)
    p.add_argument("--batch-size", type=int, default=16)
    p.add_argument("--test-batch-size", type=int, default=64)
    p.add_argument("--patch-size", type=int, nargs=2, metavar=("H", "W"), default=(256, 256), help="multiples of 64")
    p.add_argument("-n", "--num-workers", type=int, default=3, help="host threads that decode image files")
    p.add_argument("--save", action="store_true", help="write DIR/checkpoint.pth.tar (and the best-loss copy) after every epoch")
    p.add_argument("--seed", type=int, default=None, help="default: 0, or the seed of the --resume checkpoint")
    p.add_argument("--model", choices=("hesic", "joint"), default="hesic", help="hesic: HSIC (default); joint: HESIC+ (HSICJoint)")
    p.add_argument("--homography", choices=("sidecar", "net", "surf"), default="sidecar")
    p.add_argument("--homography-checkpoint", default=None, help="HomographyNet weights for --homography net (default: synthetic weights)")
    p.add_argument("--distortion", choices=("mse", "ms-ssim"), default="mse")
    p.add_argument("--clip-max-norm", type=float, default=None)
    p.add_argument("--skip-nonfinite", action="store_true")
    p.add_argument("--graphed", action="store_true", help="replay the step as one HIP graph (drops an epoch's ragged last batch)")
    p.add_argument("--dtype", choices=sorted(_DTYPES), default="bf16")
    p.add_argument("--cache", choices=("device", "stream"), default="device")
    p.add_argument("--cache-gb", type=float, default=None, help="device-memory budget of the decoded pairs (default: half of the free memory)")
    p.add_argument("--augment", nargs="+", choices=("hflip", "vflip", "swap"), default=(), metavar="hflip|vflip|swap",
                   help="flip both views / exchange them in the training batches, the homography with them (default: none)")
    p.add_argument("--valid-split", default="test")
    p.add_argument("--resume", default="none", metavar="PATH|none")
    p.add_argument("--out", default=".")
    return p


class _Homography:
    """The ``h_matrix`` of a gathered batch for ``--homography net|surf``; ``invalid`` counts the pairs that got the identity."""

    def __init__(self, kind, checkpoint, device):
        self.kind, self.invalid, self.net = kind, 0, None
        self._flags = []
        if kind == "net":
            from .codec import load_homography_net
            self.net = load_homography_net(checkpoint, device)
            for q in self.net.parameters():
                q.requires_grad_(False)

    def __call__(self, x1, x2, indices, rng):
        from . import homography, stereo_h
        if self.kind == "net":
            xy = homography.window_origins(x1.shape[0], None, 256, self.net.side * 8, 45, rng)
            return homography.h_matrix_from_pair(self.net, x1, x2, xy).detach()
        H, valid, _ = stereo_h.estimate_homography(x1, x2, pair_ids=indices)
        eye = torch.eye(3, dtype=torch.float32, device=H.device).expand_as(H)
        self._flags.append(valid)
        return torch.where(valid.view(-1, 1, 1), H, eye)

    def flush(self):
        """Read the validity flags back (once per epoch) into ``invalid``."""
        if self._flags:
            self.invalid += int(sum(int(f.numel()) for f in self._flags) - int(torch.cat(self._flags).sum()))
            self._flags = []


def _inputs(cache, indices, origins, ph, pw, homography, rng, out=None, flags=None):
    x1, x2, h, _ = cache.batch(indices, origins, ph, pw, out=out, flags=flags)
    if homography is not None:
        hm = homography(x1, x2, indices, rng)
        h = h.copy_(hm) if out is not None else hm          # under --graphed the matrix lands in the captured step's static input
    return x1, x2, h


def train_epoch(trainer, cache, plan, ph, pw, homography=None):
    """One pass over ``plan``; returns ({key: mean over the steps}, steps, seconds).  The losses stay on the device until the end."""
    dev = cache.device
    total, n, t0 = torch.zeros(len(TRAIN_KEYS), dtype=torch.float64, device=dev), 0, time.time()
    static = getattr(trainer, "static_inputs", None)
    for i, (indices, origins) in enumerate(plan):
        flags = plan.flags[i] if plan.flags else None       # a plan made by hand carries none
        out = static() if static is not None else None
        if out is not None and out[0].shape[0] != len(indices):
            raise RuntimeError(f"train_folder: a batch of {len(indices)} for a step captured with {out[0].shape[0]}")
        x1, x2, h = _inputs(cache, indices, origins, ph, pw, homography, plan.rng, out, flags)
        crit = trainer.step(x1, x2, h)
        total += torch.stack([crit[k].reshape(()).double() for k in TRAIN_KEYS])
        n += 1
    vals = (total / max(n, 1)).tolist()                     # the one read-back of the epoch
    return dict(zip(TRAIN_KEYS, vals)), n, time.time() - t0


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
    total, n = torch.zeros(len(VALID_KEYS), dtype=torch.float64, device=cache.device), 0
    with torch.no_grad():
        for indices, origins in plan:
            x1, x2, h = _inputs(cache, indices, origins, ph, pw, homography, plan.rng)
            total += valid_batch_values(model, x1, x2, h, lmbda, distortion)
            n += 1
    model.train()
    rec = dict(zip(VALID_KEYS, (total / max(n, 1)).tolist()))
    rec["psnr"] = (rec["psnr1"] + rec["psnr2"]) / 2
    rec["psnr_of_mse"] = mse2psnr(rec["mse_loss"] / 2) if n else float("nan")
    rec["batches"] = n
    return rec


test_epoch.__test__ = False         # the reference's name for the validation pass, not a pytest case


def save_checkpoint(trainer, path, loss, epoch, seed):
    torch.save({"epoch": int(epoch), "state_dict": {k: v.detach().cpu().clone() for k, v in trainer.model.state_dict().items()},
                "loss": float(loss), "optimizer": trainer.optimizer.state_dict(), "aux_optimizer": trainer.aux_optimizer.state_dict(),
                "seed": int(seed)}, path)


def _kept(cache, homography):
    return [i for i in range(len(cache)) if cache.has_h[i]] if homography == "sidecar" else list(range(len(cache)))


def main(argv=None, log=print):
    """Returns the epochs' records (each also logged as one JSON line); 2 without a ROCm device."""
    import hesic_amd
    from . import functional as Fn
    from . import models, pair_cache, train
    p = parser()
    a = p.parse_args(argv)
    ph, pw = a.patch_size
    if ph < 64 or pw < 64 or ph % 64 or pw % 64:
        p.error(f"--patch-size must be positive multiples of 64, got {ph} {pw}")
    if a.batch_size < 1 or a.test_batch_size < 1 or a.epochs < 0 or a.num_workers < 1:
        p.error("--batch-size, --test-batch-size and --num-workers must be positive and --epochs not negative")
    if a.homography_checkpoint and a.homography != "net":
        p.error("--homography-checkpoint needs --homography net")
    if a.cache_gb is not None and a.cache_gb <= 0:
        p.error("--cache-gb must be positive")
    # listing needs no device: a patch that does not fit is refused here, before anything is decoded
    splits = list(dict.fromkeys(("train", a.valid_split)))
    sized = {s: pair_cache.DevicePairCache(a.root, s, mode="stream", workers=a.num_workers) for s in splits}
    for s, c in sized.items():
        for stem, (h, w) in zip(c.stems, c.sizes):
            if ph > h or pw > w:
                p.error(f"--patch-size {ph} {pw} larger than {s}/{stem} ({h}, {w})")
    if not torch.cuda.is_available():
        print("train_folder: needs a ROCm device (the training kernels have no CPU path)", file=sys.stderr)
        return 2
    device = sized["train"].device
    budget = None if a.cache_gb is None else int(a.cache_gb * 2 ** 30)
    caches = sized if a.cache == "stream" else \
        {s: pair_cache.DevicePairCache(a.root, s, mode="device", budget_bytes=budget, workers=a.num_workers) for s in splits}
    tcache, vcache = caches["train"], caches[a.valid_split]
    keep_t, keep_v = _kept(tcache, a.homography), _kept(vcache, a.homography)
    if not keep_t:
        p.error(f"no training pair has a sidecar under {a.root}/train/H (write them with python -m hesic_amd.stereo_h, or use --homography net|surf)")

    resume = None if a.resume in (None, "none") else torch.load(a.resume, map_location="cpu")
    seed = a.seed if a.seed is not None else (int(resume["seed"]) if resume is not None and "seed" in resume else 0)
    keep_dtype = Fn.compute_dtype()
    hesic_amd.set_compute_dtype(_DTYPES[a.dtype])
    try:
        torch.manual_seed(seed)                         # the constructor's own initialisation and the noise stream, reproducibly
        net = {"hesic": models.HSIC, "joint": models.HSICJoint}[a.model]()
        if resume is not None:
            net.load_state_dict(resume["state_dict"])
        net = net.to(device).train()
        cls = train.GraphedTrainer if a.graphed else train.Trainer
        trainer = cls(net, lr=a.learning_rate, aux_lr=a.aux_learning_rate, lmbda=a.lmbda, distortion=a.distortion,
                      clip_max_norm=a.clip_max_norm, skip_nonfinite=a.skip_nonfinite)
        first_epoch, best_loss = 0, float("inf")
        out = Path(a.out)
        last, best = out / "checkpoint.pth.tar", out / "checkpoint_best_loss.pth.tar"
        if a.save:
            out.mkdir(parents=True, exist_ok=True)
        if resume is not None:
            trainer.optimizer.load_state_dict(resume["optimizer"])
            trainer.aux_optimizer.load_state_dict(resume["aux_optimizer"])
            trainer.set_lr(a.learning_rate, a.aux_learning_rate)
            first_epoch, best_loss = int(resume["epoch"]) + 1, float(resume["loss"])
            prev_best = Path(a.resume).with_name(best.name)
            if prev_best.is_file():
                best_loss = min(best_loss, float(torch.load(prev_best, map_location="cpu")["loss"]))
                if a.save and prev_best.resolve() != best.resolve() and not best.is_file():
                    shutil.copyfile(prev_best, best)
        homography = None if a.homography == "sidecar" else _Homography(a.homography, a.homography_checkpoint, device)
        decode = {"decode_seconds": round(tcache.decode_seconds + (vcache.decode_seconds if vcache is not tcache else 0.0), 3)}
        history = []
        for epoch in range(first_epoch, a.epochs):
            tplan = pair_cache.epoch_plan(len(tcache), tcache.sizes, a.batch_size, ph, pw, seed, epoch, True, a.graphed, keep=keep_t,
                                          augment=a.augment)
            vplan = pair_cache.epoch_plan(len(vcache), vcache.sizes, a.test_batch_size, ph, pw, seed, None, False, False, keep=keep_v)
            tr, steps, secs = train_epoch(trainer, tcache, tplan, ph, pw, homography)
            va = test_epoch(net, vcache, vplan, ph, pw, a.lmbda, a.distortion, homography)
            if homography is not None:
                homography.flush()
            is_best = va["loss"] < best_loss
            best_loss = min(best_loss, va["loss"])
            if a.save:
                save_checkpoint(trainer, last, va["loss"], epoch, seed)
                if is_best or not best.is_file():
                    shutil.copyfile(last, best)
            rec = {"epoch": epoch, "steps": steps, "seconds_per_step": secs / max(steps, 1), "best": bool(is_best),
                   "train": tr, "valid": va, "train_loss": tr["loss"], "valid_loss": va["loss"],
                   "left_out_no_sidecar": tplan.left_out, "dropped_tail": tplan.dropped,
                   "invalid_homographies": homography.invalid if homography is not None else 0}
            if a.augment:
                rec["augmented"] = tplan.augmented()
            if epoch == first_epoch:
                rec.update(decode)
            history.append(rec)
            log(json.dumps(rec))
        return history
    finally:
        hesic_amd.set_compute_dtype(keep_dtype)


if __name__ == "__main__":
    r = main()
    sys.exit(r if isinstance(r, int) else 0)

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
shared pieces are imported from there).  The step is ``train.EnhancerTrainer.step``, or with ``--graphed`` ``train.GraphedEnhancerTrainer.step``
(the gather writes into the captured step's static inputs; an epoch's ragged last batch is dropped and counted).

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

import json
import shutil
import sys
import time
from pathlib import Path

import torch

from .train_folder import _DTYPES, _Homography, _inputs, _kept, mse2psnr

_INFER_DTYPES = {"f16": torch.float16, "bf16": torch.bfloat16, "f32": torch.float32}
TRAIN_KEYS = ("loss", "mse_loss")
VALID_KEYS = ("loss", "mse_loss", "bpp_loss", "psnr1", "psnr2")
MS_SSIM_KEYS = ("ms_ssim1", "ms_ssim2")


def parser():
    import argparse
    p = argparse.ArgumentParser(prog="python -m hesic_amd.train_stage2",
                                description="Train Independent_EN on a frozen HSIC / HSICJoint's reconstructions of ROOT/train/{left,right} on the GPU.")
    p.add_argument("root")
    p.add_argument("-e", "--epochs", type=int, default=100, help="total number of epochs (a resumed run continues up to it)")
    p.add_argument("-lr", "--learning-rate", type=float, default=1e-4)
    p.add_argument("--lambda", dest="lmbda", type=float, default=1e-2)
    p.add_argument("--batch-size", type=int, default=16)
    p.add_argument("--test-batch-size", type=int, default=64)
    p.add_argument("--patch-size", type=int, nargs=2, metavar=("H", "W"), default=(256, 256), help="multiples of 64")
    p.add_argument("-n", "--num-workers", type=int, default=3, help="host threads that decode image files")
    p.add_argument("--save", action="store_true", help="write DIR/second_checkpoint.pth.tar (and the best-loss copy) after every epoch")
    p.add_argument("--seed", type=int, default=None, help="default: 0, or the seed of the --resume checkpoint")
    p.add_argument("--homography", choices=("sidecar", "net", "surf"), default="sidecar")
    p.add_argument("--homography-checkpoint", default=None, help="HomographyNet weights for --homography net (default: synthetic weights)")
    p.add_argument("--clip-max-norm", type=float, default=None)
    p.add_argument("--skip-nonfinite", action="store_true")
    p.add_argument("--graphed", action="store_true", help="replay the step as one HIP graph (drops an epoch's ragged last batch)")
    p.add_argument("--dtype", choices=sorted(_DTYPES), default="bf16", help="the enhancer's training format")
    p.add_argument("--cache", choices=("device", "stream"), default="device")
    p.add_argument("--cache-gb", type=float, default=None, help="device-memory budget of the decoded pairs (default: half of the free memory)")
    p.add_argument("--augment", nargs="+", choices=("hflip", "vflip", "swap"), default=(), metavar="hflip|vflip|swap",
                   help="flip both views / exchange them in the training batches, the homography with them (default: none)")
    p.add_argument("--valid-split", default="test")
    p.add_argument("--out", default=".")
    p.add_argument("--model", choices=("hesic", "joint"), default="hesic", help="the frozen model: HSIC (default) or HESIC+ (HSICJoint)")
    p.add_argument("--checkpoint", default=None, metavar="PATH|synthetic", help="the frozen model's weights (required; 'synthetic': the deterministic ones)")
    p.add_argument("--infer-dtype", choices=sorted(_INFER_DTYPES), default="f16", help="the format of the frozen forward")
    p.add_argument("--resume", default="none", metavar="PATH|none", help="a second_checkpoint*.pth.tar written by this command")
    return p


def train_epoch(trainer, cache, plan, ph, pw, homography=None):
    """One pass over ``plan``; returns ({key: mean over the steps}, steps, seconds).  The losses stay on the device until the end."""
    total, n, t0 = torch.zeros(len(TRAIN_KEYS), dtype=torch.float64, device=cache.device), 0, time.time()
    static = getattr(trainer, "static_inputs", None)
    for i, (indices, origins) in enumerate(plan):
        flags = plan.flags[i] if plan.flags else None       # a plan made by hand carries none
        out = static() if static is not None else None
        if out is not None and out[0].shape[0] != len(indices):
            raise RuntimeError(f"train_stage2: a batch of {len(indices)} for a step captured with {out[0].shape[0]}")
        x1, x2, h = _inputs(cache, indices, origins, ph, pw, homography, plan.rng, out, flags)
        crit = trainer.step(x1, x2, h)
        total += torch.stack([crit[k].reshape(()).double() for k in TRAIN_KEYS])
        n += 1
    vals = (total / max(n, 1)).tolist()                     # the one read-back of the epoch
    return dict(zip(TRAIN_KEYS, vals)), n, time.time() - t0


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
    total, n = torch.zeros(len(keys), dtype=torch.float64, device=cache.device), 0
    with torch.no_grad():
        for indices, origins in plan:
            x1, x2, h = _inputs(cache, indices, origins, ph, pw, homography, plan.rng)
            total += valid_batch_values(model, enhancer, x1, x2, h, lmbda, with_ms_ssim)
            n += 1
    enhancer.train()
    rec = dict(zip(keys, (total / max(n, 1)).tolist()))
    rec["psnr"] = (rec["psnr1"] + rec["psnr2"]) / 2
    rec["psnr_of_mse"] = mse2psnr(rec["mse_loss"] / 2) if n else float("nan")
    rec["batches"] = n
    return rec


test_epoch.__test__ = False         # the reference's name for the validation pass, not a pytest case


def save_checkpoint(trainer, aux_optimizer, path, loss, epoch, seed):
    torch.save({"epoch": int(epoch), "state_dict": {k: v.detach().cpu().clone() for k, v in trainer.enhancer.state_dict().items()},
                "loss": float(loss), "optimizer": trainer.optimizer.state_dict(), "aux_optimizer": aux_optimizer.state_dict(),
                "seed": int(seed)}, path)


def main(argv=None, log=print):
    """Returns the epochs' records (each also logged as one JSON line); 2 without a ROCm device."""
    import hesic_amd
    from . import codec, models, pair_cache, train
    from . import functional as Fn
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
    if not a.checkpoint:
        p.error("--checkpoint is required: the frozen model's weights, or 'synthetic' for the deterministic ones")
    splits = list(dict.fromkeys(("train", a.valid_split)))
    sized = {s: pair_cache.DevicePairCache(a.root, s, mode="stream", workers=a.num_workers) for s in splits}
    for s, c in sized.items():
        for stem, (h, w) in zip(c.stems, c.sizes):
            if ph > h or pw > w:
                p.error(f"--patch-size {ph} {pw} larger than {s}/{stem} ({h}, {w})")
    if not torch.cuda.is_available():
        print("train_stage2: needs a ROCm device (the training kernels have no CPU path)", file=sys.stderr)
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
    try:
        # the frozen model in the inference format (which stays the process's format outside the enhancer's forward / backward)
        net = codec.load_model(None if a.checkpoint == "synthetic" else a.checkpoint, _INFER_DTYPES[a.infer_dtype], device=device, model=a.model)
        torch.manual_seed(seed)                         # the enhancer's own initialisation, reproducibly
        enhancer = models.Independent_EN()
        if resume is not None:
            enhancer.load_state_dict(resume["state_dict"])
        enhancer = enhancer.to(device).train()
        cls = train.GraphedEnhancerTrainer if a.graphed else train.EnhancerTrainer
        trainer = cls(net, enhancer, lr=a.learning_rate, lmbda=a.lmbda, train_dtype=_DTYPES[a.dtype], clip_max_norm=a.clip_max_norm,
                      skip_nonfinite=a.skip_nonfinite)
        aux_optimizer = torch.optim.Adam(net.aux_parameters(), lr=1e-3)          # never stepped (newtrain6_real.py:169-171): the file format's slot
        first_epoch, best_loss = 0, float("inf")
        out = Path(a.out)
        last, best = out / "second_checkpoint.pth.tar", out / "second_checkpoint_best_loss.pth.tar"
        if a.save:
            out.mkdir(parents=True, exist_ok=True)
        if resume is not None:
            trainer.optimizer.load_state_dict(resume["optimizer"])
            trainer.set_lr(a.learning_rate)
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
            va = test_epoch(net, enhancer, vcache, vplan, ph, pw, a.lmbda, homography)
            if homography is not None:
                homography.flush()
            is_best = va["loss"] < best_loss
            best_loss = min(best_loss, va["loss"])
            if a.save:
                save_checkpoint(trainer, aux_optimizer, last, va["loss"], epoch, seed)
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

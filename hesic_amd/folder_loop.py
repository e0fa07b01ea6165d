"""What the folder training commands share: ``python -m hesic_amd.train_folder`` and ``python -m hesic_amd.train_stage2`` are this run loop
around a trainer and a validation pass of their own; ``homography_train`` takes ``resume_position``.

    add_shared_options, refuse      the options both commands have (defaults and help text included) and their refusals, in one order
    open_folder                     refusals -> listing pass (a patch larger than an image is refused before anything is decoded) -> device check
                                    -> the caches -> the ``--resume`` file and the seed
    train_epoch, valid_epoch        one pass over a plan: the values of ``keys`` added up on the device and read back once
    resume_position                 ``--resume`` -> (first epoch, lowest validation loss so far), the sibling best file included
    run_epochs                      plan, train, validate, flush the homography counter, save last and best, build and log the record
    run                             ``open_folder`` -> the command's ``build`` -> ``run_epochs``, the compute dtype restored at the end

A command's file keeps its docstring, its own options, its model and trainer construction, ``valid_batch_values`` and ``save_checkpoint``.  It
hands ``run`` a ``build(a, folder)`` that returns three plain callables, ``train(plan, homography)``, ``valid(plan, homography)`` and
``save(path, loss, epoch)``.  An option, a refusal or a piece of bookkeeping that two commands share belongs here, not in a copy.
"""
from __future__ import annotations

import json
import math
import shutil
import sys
import time
from pathlib import Path
from types import SimpleNamespace

import torch

_DTYPES = {"bf16": torch.bfloat16, "f32": torch.float32}


def mse2psnr(mse):
    return 10 * math.log10(1 / mse)


def add_shared_options(p, stem):
    """The options of every folder training command; ``stem`` names the checkpoint files (``DIR/<stem>.pth.tar``)."""
    p.add_argument("root")
    p.add_argument("-e", "--epochs", type=int, default=100, help="total number of epochs (a resumed run continues up to it)")
    p.add_argument("-lr", "--learning-rate", type=float, default=1e-4)
    p.add_argument("--lambda", dest="lmbda", type=float, default=1e-2)
    p.add_argument("--batch-size", type=int, default=16)
    p.add_argument("--test-batch-size", type=int, default=64)
    p.add_argument("--patch-size", type=int, nargs=2, metavar=("H", "W"), default=(256, 256), help="multiples of 64")
    p.add_argument("-n", "--num-workers", type=int, default=3, help="host threads that decode image files")
    p.add_argument("--save", action="store_true", help=f"write DIR/{stem}.pth.tar (and the best-loss copy) after every epoch")
    p.add_argument("--seed", type=int, default=None, help="default: 0, or the seed of the --resume checkpoint")
    p.add_argument("--homography", choices=("sidecar", "net", "surf"), default="sidecar")
    p.add_argument("--homography-checkpoint", default=None, help="HomographyNet weights for --homography net (default: synthetic weights)")
    p.add_argument("--clip-max-norm", type=float, default=None)
    p.add_argument("--skip-nonfinite", action="store_true")
    p.add_argument("--graphed", action="store_true", help="replay the step as one HIP graph (drops an epoch's ragged last batch)")
    p.add_argument("--cache", choices=("device", "stream"), default="device")
    p.add_argument("--cache-gb", type=float, default=None, help="device-memory budget of the decoded pairs (default: half of the free memory)")
    p.add_argument("--augment", nargs="+", choices=("hflip", "vflip", "swap"), default=(), metavar="hflip|vflip|swap",
                   help="flip both views / exchange them in the training batches, the homography with them (default: none)")
    p.add_argument("--valid-split", default="test")
    p.add_argument("--out", default=".")


def refuse(p, a):
    ph, pw = a.patch_size
    if ph < 64 or pw < 64 or ph % 64 or pw % 64:
        p.error(f"--patch-size must be positive multiples of 64, got {ph} {pw}")
    if a.batch_size < 1 or a.test_batch_size < 1 or a.epochs < 0 or a.num_workers < 1:
        p.error("--batch-size, --test-batch-size and --num-workers must be positive and --epochs not negative")
    if a.homography_checkpoint and a.homography != "net":
        p.error("--homography-checkpoint needs --homography net")
    if a.cache_gb is not None and a.cache_gb <= 0:
        p.error("--cache-gb must be positive")


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


def _kept(cache, homography):
    return [i for i in range(len(cache)) if cache.has_h[i]] if homography == "sidecar" else list(range(len(cache)))


def open_folder(p, a, name, refusal=None):
    """Everything between the parser and the model: the shared refusals, then the command's own ``refusal`` (a message, or None), the listing
    pass, the device check (``None`` without a ROCm device, after a line on stderr), the caches, the ``--resume`` file and the seed."""
    from . import pair_cache
    refuse(p, a)
    if refusal:
        p.error(refusal)
    ph, pw = a.patch_size
    # listing needs no device: a patch that does not fit is refused here, before anything is decoded
    splits = list(dict.fromkeys(("train", a.valid_split)))
    sized = {s: pair_cache.DevicePairCache(a.root, s, mode="stream", workers=a.num_workers) for s in splits}
    for s, c in sized.items():
        for stem, (h, w) in zip(c.stems, c.sizes):
            if ph > h or pw > w:
                p.error(f"--patch-size {ph} {pw} larger than {s}/{stem} ({h}, {w})")
    if not torch.cuda.is_available():
        print(f"{name}: needs a ROCm device (the training kernels have no CPU path)", file=sys.stderr)
        return None
    budget = None if a.cache_gb is None else int(a.cache_gb * 2 ** 30)
    caches = sized if a.cache == "stream" else \
        {s: pair_cache.DevicePairCache(a.root, s, mode="device", budget_bytes=budget, workers=a.num_workers) for s in splits}
    tcache, vcache = caches["train"], caches[a.valid_split]
    keep_t, keep_v = _kept(tcache, a.homography), _kept(vcache, a.homography)
    if not keep_t:
        p.error(f"no training pair has a sidecar under {a.root}/train/H (write them with python -m hesic_amd.stereo_h, or use --homography net|surf)")
    resume = None if a.resume in (None, "none") else torch.load(a.resume, map_location="cpu")
    seed = a.seed if a.seed is not None else (int(resume["seed"]) if resume is not None and "seed" in resume else 0)
    return SimpleNamespace(device=sized["train"].device, tcache=tcache, vcache=vcache, keep_t=keep_t, keep_v=keep_v, resume=resume, seed=seed)


def train_epoch(trainer, cache, plan, ph, pw, keys, name, homography=None):
    """One pass over ``plan``; returns ({key: mean over the steps}, steps, seconds).  The losses stay on the device until the end."""
    total, n, t0 = torch.zeros(len(keys), dtype=torch.float64, device=cache.device), 0, time.time()
    static = getattr(trainer, "static_inputs", None)
    for i, (indices, origins) in enumerate(plan):
        flags = plan.flags[i] if plan.flags else None       # a plan made by hand carries none
        out = static() if static is not None else None
        if out is not None and out[0].shape[0] != len(indices):
            raise RuntimeError(f"{name}: a batch of {len(indices)} for a step captured with {out[0].shape[0]}")
        x1, x2, h = _inputs(cache, indices, origins, ph, pw, homography, plan.rng, out, flags)
        crit = trainer.step(x1, x2, h)
        total += torch.stack([crit[k].reshape(()).double() for k in keys])
        n += 1
    vals = (total / max(n, 1)).tolist()                     # the one read-back of the epoch
    return dict(zip(keys, vals)), n, time.time() - t0


def valid_epoch(cache, plan, ph, pw, keys, batch_values, homography=None):
    """The mean over the batches of ``batch_values(x1, x2, h)`` (an fp64 device vector in ``keys`` order) under ``no_grad``, plus both printed
    forms of the PSNR and the number of batches.  The caller sets the modules' modes."""
    total, n = torch.zeros(len(keys), dtype=torch.float64, device=cache.device), 0
    with torch.no_grad():
        for indices, origins in plan:
            total += batch_values(*_inputs(cache, indices, origins, ph, pw, homography, plan.rng))
            n += 1
    rec = dict(zip(keys, (total / max(n, 1)).tolist()))
    rec["psnr"] = (rec["psnr1"] + rec["psnr2"]) / 2
    rec["psnr_of_mse"] = mse2psnr(rec["mse_loss"] / 2) if n else float("nan")
    rec["batches"] = n
    return rec


def resume_position(resume, resume_path, best, copy_best):
    """``(first epoch, lowest validation loss so far)`` of a run that continues the checkpoint ``resume`` (loaded from ``resume_path``; None: a
    new run).  The best-loss file beside ``resume_path`` counts and, under ``copy_best``, becomes ``best`` where that does not exist yet."""
    if resume is None:
        return 0, float("inf")
    first_epoch, best_loss = int(resume["epoch"]) + 1, float(resume["loss"])
    prev_best = Path(resume_path).with_name(best.name)
    if prev_best.is_file():
        best_loss = min(best_loss, float(torch.load(prev_best, map_location="cpu")["loss"]))
        if copy_best and prev_best.resolve() != best.resolve() and not best.is_file():
            shutil.copyfile(prev_best, best)
    return first_epoch, best_loss


def run_epochs(a, folder, stem, train, valid, save, log):
    """Epochs ``first .. a.epochs - 1``: ``train(plan, homography)`` -> ``(means, steps, seconds)``, ``valid(plan, homography)`` -> the
    validation record, ``save(path, loss, epoch)`` under ``--save``; returns the records, each also logged as one JSON line."""
    from . import pair_cache
    ph, pw = a.patch_size
    tcache, vcache = folder.tcache, folder.vcache
    out = Path(a.out)
    last, best = out / f"{stem}.pth.tar", out / f"{stem}_best_loss.pth.tar"
    if a.save:
        out.mkdir(parents=True, exist_ok=True)
    first_epoch, best_loss = resume_position(folder.resume, a.resume, best, a.save)
    homography = None if a.homography == "sidecar" else _Homography(a.homography, a.homography_checkpoint, folder.device)
    decode = {"decode_seconds": round(tcache.decode_seconds + (vcache.decode_seconds if vcache is not tcache else 0.0), 3)}
    history = []
    for epoch in range(first_epoch, a.epochs):
        tplan = pair_cache.epoch_plan(len(tcache), tcache.sizes, a.batch_size, ph, pw, folder.seed, epoch, True, a.graphed, keep=folder.keep_t,
                                      augment=a.augment)
        vplan = pair_cache.epoch_plan(len(vcache), vcache.sizes, a.test_batch_size, ph, pw, folder.seed, None, False, False, keep=folder.keep_v)
        tr, steps, secs = train(tplan, homography)
        va = valid(vplan, homography)
        if homography is not None:
            homography.flush()
        is_best = va["loss"] < best_loss
        best_loss = min(best_loss, va["loss"])
        if a.save:
            save(last, va["loss"], epoch)
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


def run(p, a, name, stem, build, log, refusal=None):
    """A whole command after its parser: returns the epochs' records, or 2 without a ROCm device.  ``build(a, folder)`` makes the model and the
    trainer (restoring ``folder.resume`` into them) and returns ``run_epochs``' ``(train, valid, save)``; the process's compute dtype, which
    ``build`` may set, is put back at the end."""
    import hesic_amd
    from . import functional as Fn
    folder = open_folder(p, a, name, refusal)
    if folder is None:
        return 2
    keep_dtype = Fn.compute_dtype()
    try:
        return run_epochs(a, folder, stem, *build(a, folder), log)
    finally:
        hesic_amd.set_compute_dtype(keep_dtype)

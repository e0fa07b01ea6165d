"""``python -m hesic_amd.eval_folder ROOT``: one rate-distortion point of a checkpoint on a stereo folder, with per-pair figures.

    ROOT [--split test] [--batch 8] [--model hesic|joint] [--checkpoint PATH] [--dtype f16|bf16|f32]
         [--homography sidecar|net] [--homography-checkpoint PATH] [--enhancer PATH|synthetic] [--coded] [--channels-per-stream 1] [--out FILE]

ROOT/<split>/{left,right}/ + ROOT/<split>/H/<stem>.npy, the layout of ``python -m hesic_amd.codec``; pairs are grouped by image size and
evaluated ``--batch`` at a time, zero-padded to multiples of 64 and measured against the ORIGINAL pixels.  What the reference does in
ywz/mywork/test3real.py at ``--test-batch-size 1`` ("PSNR计算后再平均", :3) is done here on whole batches: ``models.pair_metrics`` reduces
every pair of a batch on its own (bit-identical to evaluating it alone), so the mean of per-pair PSNRs costs no batching.

One JSON line per pair -- stem, height, width, the figures of ``models.pair_metrics_from`` (bpp_loss, bpp, mse1/2, psnr1/2, psnr, and
psnr8_1/2, psnr8: the PSNR of the 8-bit images a decoder writes), ``bits`` per likelihood key, ms_ssim1, ms_ssim2, ms_ssim, ms_ssim_db
(``null`` where the smaller side does not exceed 160) and, with ``--coded``, coded_bpp = len(blob) * 8 / (2 H W) of ``compress_batch`` next
to the estimated ``bpp`` (the comparison of the reference's codec-test/test2_codec.py) -- then one summary line (``summarise``), which
``--out`` also writes to a file: the mean over pairs of every figure (``psnr`` = mean over pairs of (psnr1 + psnr2) / 2, the reference's
number) and ``psnr_of_mean_mse``, the PSNR of the mean MSE that ``metrics_from`` / ``LambdaSweep`` report for a batch, under its own name.

``--enhancer`` runs ``Independent_EN`` on the reconstructions (a ``second_checkpoint*.pth.tar`` with ``state_dict``, or ``synthetic`` for the
deterministic weights): as in test3real.py:184-192 the distortion then comes from the enhanced images and the bits from the first model.
``--homography`` as in ``codec encode``.  Every chunk's figures stay on the device in one table that is read back once per folder.
"""
from __future__ import annotations

import argparse
import json
import math
import os
import sys
import time

import numpy as np
import torch

from . import codec

FIGURES = ("bpp_loss", "bpp", "mse1", "mse2", "psnr1", "psnr2", "psnr", "psnr8_1", "psnr8_2", "psnr8")
MS_SSIM_FIELDS = ("ms_ssim1", "ms_ssim2", "ms_ssim", "ms_ssim_db")
MS_SSIM_MIN_SIDE = 160          # models.ms_ssim: the smaller side must EXCEED this


def parser():
    p = argparse.ArgumentParser(prog="python -m hesic_amd.eval_folder",
                                description="Per-pair bpp / PSNR / MS-SSIM of a HESIC checkpoint on a stereo folder, on the GPU.")
    p.add_argument("root")
    p.add_argument("--split", default="test")
    p.add_argument("--batch", type=int, default=8)
    p.add_argument("--model", choices=("hesic", "joint"), default="hesic", help="hesic: HSIC (default); joint: HESIC+ (HSICJoint)")
    p.add_argument("--checkpoint", default=None, help="model weights (default: the deterministic synthetic weights)")
    p.add_argument("--dtype", choices=sorted(codec._DTYPES), default="f16")
    p.add_argument("--homography", choices=("sidecar", "net"), default="sidecar",
                   help="sidecar: ROOT/<split>/H/<stem>.npy (default), pairs without one are skipped and counted; net: HomographyNet on every pair")
    p.add_argument("--homography-checkpoint", default=None, help="HomographyNet weights for --homography net (default: synthetic weights)")
    p.add_argument("--enhancer", default=None, metavar="PATH|synthetic",
                   help="run Independent_EN on the reconstructions: a second_checkpoint*.pth.tar, or 'synthetic' for the deterministic weights")
    p.add_argument("--coded", action="store_true", help="also range-code every pair (compress_batch) and record coded_bpp")
    p.add_argument("--channels-per-stream", type=int, default=1)
    p.add_argument("--z-coder", choices=("host", "device"), default="host", help="with --coded: who codes the z strings (same bytes)")
    p.add_argument("--out", default=None, help="also write the summary line to this file")
    return p


def plan(root, split, batch, sidecars=True):
    """(chunks, skipped): the folder as ``codec.encode_folder`` walks it -- pairs grouped by image size in first-seen order, cut into chunks
    of at most ``batch``; ``chunks`` = [((width, height), [(stem, left, right, H path or None), ...])].  With ``sidecars`` a pair without
    one is skipped and counted.  Reads file headers only."""
    from .stereo_h import _image_size
    groups, skipped = {}, 0
    for stem, lf, rf, hp in codec._pairs(root, split):
        if hp is None and sidecars:
            skipped += 1
            continue
        sa, sb = _image_size(lf), _image_size(rf)
        if sa != sb:
            raise ValueError(f"{os.path.basename(lf)}: the two views differ in size ({sa} vs {sb})")
        groups.setdefault(sa, []).append((stem, lf, rf, hp))
    chunks = [(size, items[c0:c0 + batch]) for size, items in groups.items() for c0 in range(0, len(items), batch)]
    return chunks, skipped


def _mean(values):
    """AverageMeter over updates of n = 1 (test3real.py:127-139): the running sum in record order, divided by the count."""
    s, n = 0, 0
    for v in values:
        s += v
        n += 1
    return s / n if n else None


def summarise(records):
    """The summary of per-pair records, pure host arithmetic: ``pairs`` and the mean over pairs of every figure, of ``bits`` per key, of the
    MS-SSIM fields (over the pairs that have them; ``None`` when none has) and of ``coded_bpp`` where recorded -- the reference's
    ``--test-batch-size 1`` convention: ``psnr`` is the mean over pairs of (psnr1 + psnr2) / 2.  ``psnr_of_mean_mse`` is the other
    convention of the code base, the one ``metrics_from`` applies to a batch: (PSNR(mean mse1) + PSNR(mean mse2)) / 2."""
    res = {"pairs": len(records)}
    for k in FIGURES:
        res[k] = _mean(r[k] for r in records)
    keys = list(records[0]["bits"]) if records else []
    res["bits"] = {k: _mean(r["bits"][k] for r in records) for k in keys}
    for k in MS_SSIM_FIELDS:
        res[k] = _mean(r[k] for r in records if r.get(k) is not None)
    if any("coded_bpp" in r for r in records):
        res["coded_bpp"] = _mean(r["coded_bpp"] for r in records if "coded_bpp" in r)
    if records and res["mse1"] > 0 and res["mse2"] > 0:
        res["psnr_of_mean_mse"] = (10 * math.log10(1 / res["mse1"]) + 10 * math.log10(1 / res["mse2"])) / 2
    else:
        res["psnr_of_mean_mse"] = None if not records else 100.0 if res["mse1"] == 0 and res["mse2"] == 0 else float("nan")
    return res


def load_enhancer(spec, device="cuda"):
    """``Independent_EN`` in eval mode: ``spec`` a checkpoint with ``state_dict`` (the reference's second_checkpoint*.pth.tar) or "synthetic"."""
    from . import models, synthetic
    en = models.Independent_EN()
    if spec == "synthetic":
        synthetic.fill_state_dict_(en.state_dict())
    else:
        state = torch.load(spec, map_location="cpu")
        en.load_state_dict(state.get("state_dict", state) if isinstance(state, dict) else state)
    return en.to(device).eval()


def evaluate_folder(net, root, split="test", batch=8, homography_net=None, enhancer=None, coded=False, channels_per_stream=1, log=print, z_coder="host"):
    """(records, summary) of ROOT/<split>; every record and the summary are logged as one JSON line each."""
    from . import homography, models
    chunks, skipped = plan(root, split, batch, sidecars=homography_net is None)
    t0 = time.time()
    rows, meta, keys = [], [], None
    with torch.no_grad():
        for (w, h), chunk in chunks:
            x1p = models.pad_to_multiple(torch.stack([codec.read_image(lf) for _, lf, _, _ in chunk])).cuda()
            x2p = models.pad_to_multiple(torch.stack([codec.read_image(rf) for _, _, rf, _ in chunk])).cuda()
            x1, x2 = x1p[..., :h, :w], x2p[..., :h, :w]                 # the images as they are (strided views): the padding is not part of the frame
            if homography_net is not None:
                Hm = homography.h_matrix_from_pair(homography_net, x1, x2, "centre")
            else:
                Hm = torch.from_numpy(np.stack([np.load(hp).astype(np.float64).reshape(3, 3) for _, _, _, hp in chunk])).float().cuda()
            out = net(x1p, x2p, Hm)
            if enhancer is not None:                                    # distortion from the enhanced images, bits from the first model
                en = enhancer(out["x1_hat"], out["x2_hat"], Hm)
                out = {"x1_hat": en["x1_hat"], "x2_hat": en["x2_hat"], "likelihoods": out["likelihoods"]}
            m = models.pair_metrics_from(models.pair_metrics(out, x1, x2))
            if keys is None:
                keys = list(m["bits"])
            cols = [m[k] for k in FIGURES] + [m["bits"][k] for k in keys]
            with_ssim = min(h, w) > MS_SSIM_MIN_SIDE
            if with_ssim:
                s1, s2 = models.ms_ssim(out["x1_hat"][..., :h, :w], x1), models.ms_ssim(out["x2_hat"][..., :h, :w], x2)
                s = (s1 + s2) / 2
                cols += [s1, s2, s, models.ms_ssim_db(s)]
            else:
                cols += [torch.full_like(m["bpp"], float("nan"))] * len(MS_SSIM_FIELDS)
            rows.append(torch.stack(cols, 1))                           # (B, columns) fp64, stays on the device
            blobs = net.compress_batch(x1p, x2p, Hm, channels_per_stream=channels_per_stream, z_coder=z_coder)["blobs"] if coded else [None] * len(chunk)
            for (stem, _, _, _), blob in zip(chunk, blobs):
                meta.append((stem, h, w, with_ssim, None if blob is None else len(blob) * 8 / (2 * h * w)))   # against the ORIGINAL pixels
        table = torch.cat(rows).cpu().tolist() if rows else []          # the one read-back of the folder
    seconds = time.time() - t0
    names = list(FIGURES) + ["bits." + k for k in (keys or [])] + list(MS_SSIM_FIELDS)
    records = []
    for (stem, h, w, with_ssim, coded_bpp), row in zip(meta, table):
        v = dict(zip(names, row))
        rec = {"stem": stem, "height": h, "width": w}
        rec.update({k: v[k] for k in FIGURES})
        rec["bits"] = {k: v["bits." + k] for k in keys}
        rec.update({k: (v[k] if with_ssim else None) for k in MS_SSIM_FIELDS})
        if coded_bpp is not None:
            rec["coded_bpp"] = coded_bpp
        records.append(rec)
        log(json.dumps(rec))
    summary = summarise(records)
    summary.update({"skipped_no_sidecar": skipped, "seconds": seconds, "pairs_per_s": len(records) / seconds if seconds > 0 else 0.0})
    log(json.dumps(summary))
    return records, summary


def main(argv=None, log=print):
    """Returns the per-pair records (each logged as one JSON line, then the summary line); 2 without a ROCm device."""
    p = parser()
    a = p.parse_args(argv)
    if a.batch < 1:
        p.error("--batch must be positive")
    if a.channels_per_stream < 1:
        p.error("--channels-per-stream must be positive")
    if a.homography_checkpoint and a.homography != "net":
        p.error("--homography-checkpoint needs --homography net")
    if not torch.cuda.is_available():
        print("eval_folder: needs a ROCm device (the model and the metric kernels have no CPU path)", file=sys.stderr)
        return 2
    import hesic_amd
    from . import functional as Fn
    keep_dtype = Fn.compute_dtype()
    try:
        net = codec.load_model(a.checkpoint, codec._DTYPES[a.dtype], model=a.model)
        hnet = codec.load_homography_net(a.homography_checkpoint) if a.homography == "net" else None
        enhancer = load_enhancer(a.enhancer) if a.enhancer else None
        records, summary = evaluate_folder(net, a.root, a.split, a.batch, hnet, enhancer, a.coded, a.channels_per_stream, log, z_coder=a.z_coder)
        if a.out:
            with open(a.out, "w") as f:
                f.write(json.dumps(summary) + "\n")
        return records
    finally:
        hesic_amd.set_compute_dtype(keep_dtype)


if __name__ == "__main__":
    r = main()
    sys.exit(r if isinstance(r, int) else 0)

"""``python -m hesic_amd.homography_eval ROOT --checkpoint PATH|synthetic``: how many pixels HomographyNet's corners are off.

    ROOT [--split test] [--batch 16] [--rho 45] [--picsize 256] [--patchsize 128] [--seed 0] [--cache device|stream] [--cache-gb G] [-n 3]
         [--out FILE] [--refine [--refine-levels 3] [--refine-iters 10]]

ROOT/<split>/{left,right}/, the layout of ``python -m hesic_amd.homography_train``.  Every pair's LEFT view is warped by a known random
homography (``homography.draw_deltas`` on ``random.Random(f"{seed}/eval/synth")``, the windows from ``random.Random(f"{seed}/eval")``;
``DevicePairCache.homonet_synth_batch``, include/hesic_homonet_synth.h) and the net, in eval mode, is asked for the corner offsets: the
mean corner error against a known warp that every homography-net paper reports.  Pairs are taken in the listing's order, ``--batch`` at a
time, pairs of all sizes together; a pair's draws and figures do not depend on ``--batch``.

One JSON line per pair -- ``stem``, ``corner_error`` (the mean over the four corners of the distance between the net's and the true
offset, in pixels of the ``picsize`` frame) and ``identity_corner_error`` (the same for an answer of zero: the figure to beat) --, then one
summary line, which ``--out`` also writes to a file: ``pairs``, ``mean_corner_error``, ``median_corner_error``, ``identity_corner_error``
(its mean), ``under_1px`` and ``under_3px`` (the share of pairs below that error) and, on the REAL pairs with the same windows,
``photometric_identity`` and ``photometric_net``: the pair-weighted mean of ``homography.photometric_loss`` per batch with ``delta = 0`` and
with the net's delta (per-batch means, so their last bits move with ``--batch``).  A per-pair photometric table is not written: it would
need a kernel of its own.  The per-pair figures stay on the device and are read back once.

``--refine`` shows what photometric refinement (``homography.refine_h_matrix``) makes of the net's answer: the answer is turned into the
matrix of the window's frame, refined against the known-warp pair of windows the net saw, and turned back into corner offsets
(``refined_delta``; the window rather than the whole frame, where the extrapolated warp moves pixels by several times ``--rho``).  Every pair's line gains ``refined_corner_error`` and the
summary ``refined_mean_corner_error``, ``refined_median_corner_error``, ``refined_under_1px`` and ``refined_under_3px``.  Without the flag
the records are unchanged.

``--checkpoint synthetic`` evaluates the deterministic synthetic weights (an untrained net; the plumbing's smoke test).
"""
from __future__ import annotations

import argparse
import json
import random
import sys

import numpy as np
import torch


def parser():
    p = argparse.ArgumentParser(prog="python -m hesic_amd.homography_eval",
                                description="Mean corner error of a HomographyNet checkpoint against known synthetic warps, on the GPU.")
    p.add_argument("root")
    p.add_argument("--checkpoint", required=True, metavar="PATH|synthetic",
                   help="a checkpoint of python -m hesic_amd.homography_train (or the reference's), or 'synthetic' for the deterministic weights")
    p.add_argument("--split", default="test")
    p.add_argument("--batch", type=int, default=16)
    p.add_argument("--rho", type=int, default=45)
    p.add_argument("--picsize", type=int, default=256)
    p.add_argument("--patchsize", type=int, default=128)
    p.add_argument("--seed", type=int, default=0)
    p.add_argument("--cache", choices=("device", "stream"), default="device")
    p.add_argument("--cache-gb", type=float, default=None, help="device-memory budget of the decoded pairs (default: half of the free memory)")
    p.add_argument("-n", "--num-workers", type=int, default=3, help="host threads that decode image files")
    p.add_argument("--out", default=None, help="also write the summary line to this file")
    p.add_argument("--refine", action="store_true", help="also report the corner error after photometric refinement of the net's answer")
    p.add_argument("--refine-levels", type=int, default=3, help="pyramid levels of --refine")
    p.add_argument("--refine-iters", type=int, default=10, help="candidates per level of --refine")
    return p


def summarise(lines, photometric_identity, photometric_net):
    """The summary record of the per-pair ``lines``; the ``refined_*`` entries where the lines carry ``refined_corner_error``."""
    err = np.array([r["corner_error"] for r in lines], dtype=np.float64)
    ident = np.array([r["identity_corner_error"] for r in lines], dtype=np.float64)
    out = {"summary": True, "pairs": len(lines), "mean_corner_error": float(err.mean()), "median_corner_error": float(np.median(err)),
           "identity_corner_error": float(ident.mean()), "under_1px": float((err < 1.0).mean()), "under_3px": float((err < 3.0).mean()),
           "photometric_identity": photometric_identity, "photometric_net": photometric_net}
    if lines and "refined_corner_error" in lines[0]:
        ref = np.array([r["refined_corner_error"] for r in lines], dtype=np.float64)
        out.update({"refined_mean_corner_error": float(ref.mean()), "refined_median_corner_error": float(np.median(ref)),
                    "refined_under_1px": float((ref < 1.0).mean()), "refined_under_3px": float((ref < 3.0).mean())})
    return out


def refined_delta(delta_hat, corners, patch_a, patch_b, levels=3, iters=10):
    """The corner offsets after refinement: ``delta_hat`` (B,4,2) becomes the matrix of the WINDOW's frame (patch_a pixel -> patch_b pixel:
    the inverse of ``DLT(c0 -> c0 + delta_hat)`` with ``c0 = corners - corners[:, :1]``, since patch_b(p) = patch_a(DLT p) wherever the
    source lies inside the window), is refined on ``(patch_a, patch_b)``, and comes back as where the inverse of the refined matrix takes
    ``c0``, minus ``c0``.  On the device.

    The window and not the whole grey frame: the offsets are drawn at the window's corners, and the warp they define, extrapolated to a
    frame twice the window's side, moves the frame's corners by several times ``rho`` (36 px for ``rho = 6`` in the numpy prototype) -- out of
    a refiner's basin, while inside the window no pixel moves further than the offsets."""
    from . import homography
    c0 = corners - corners[:, :1]
    h = homography.get_perspective_transform(c0, c0 + delta_hat).double()
    Hr, _ = homography.refine_h_matrix(patch_a, patch_b, torch.linalg.inv(h).float(), levels=levels, iters=iters)
    hr = torch.linalg.inv(Hr.double())
    pts = torch.cat([c0.double(), torch.ones_like(c0[..., :1], dtype=torch.float64)], -1) @ hr.transpose(1, 2)
    return (pts[..., :2] / pts[..., 2:] - c0.double()).float()


def main(argv=None, log=print):
    """Returns the records (one per pair, then the summary), each also logged as one JSON line; 2 without a ROCm device."""
    from . import functional as Fn
    from . import homography, homography_train, synthetic
    p = parser()
    a = p.parse_args(argv)
    if a.batch < 1 or a.num_workers < 1 or (a.cache_gb is not None and a.cache_gb <= 0):
        p.error("--batch, --num-workers and --cache-gb must be positive")
    if a.patchsize % 8 or not 8 <= a.patchsize <= a.picsize:
        p.error("--patchsize must be a multiple of 8, at most --picsize")
    if a.rho < 0:
        p.error("--rho must not be negative")
    if not torch.cuda.is_available():
        print("homography_eval: needs a ROCm device (the kernels have no CPU path)", file=sys.stderr)
        return 2
    device = torch.device("cuda", torch.cuda.current_device())
    pairs = homography_train.list_pairs(a.root, a.split)
    net = homography.Net(patch_size=a.patchsize)
    if a.checkpoint == "synthetic":
        synthetic.fill_homography_state_dict_(net.state_dict())
    else:
        homography.load_checkpoint(net, a.checkpoint)
    net = net.to(device).eval()
    cache = homography_train.build_cache(a.root, a.split, pairs, a)
    rng, srng = random.Random(f"{a.seed}/eval"), random.Random(f"{a.seed}/eval/synth")
    errs, idents, refined, photo = [], [], [], torch.zeros(2, dtype=torch.float64, device=device)
    keep_dtype = Fn.compute_dtype()
    Fn.set_compute_dtype(torch.float32)
    try:
        with torch.no_grad():
            for c0 in range(0, len(pairs), a.batch):
                items = pairs[c0:c0 + a.batch]
                indices = [cache.index_of[lf] for lf, _, _ in items]
                origins, sizes, windows = homography_train.draw_batch(items, None, rng, a.picsize, a.patchsize, a.rho)
                deltas = homography.draw_deltas(len(items), windows, a.patchsize, a.rho, srng)
                _, patch_a, scorners, delta, _, _, patch_b = cache.homonet_synth_batch(indices, origins, sizes, windows, deltas, a.picsize, a.patchsize)
                delta_hat = net(patch_a, patch_b)
                errs.append(homography.corner_error(delta_hat, delta))
                if a.refine:
                    refined.append(homography.corner_error(refined_delta(delta_hat, scorners, patch_a, patch_b, a.refine_levels, a.refine_iters), delta))
                idents.append(homography.corner_error(torch.zeros_like(delta), delta))
                grey1, _, patch1, patch2, corners = cache.homonet_batch(indices, origins, sizes, windows, a.picsize, a.patchsize)
                zero = homography.photometric_loss(torch.zeros_like(delta), grey1, patch2, corners)
                mine = homography.photometric_loss(net(patch1, patch2), grey1, patch2, corners)
                photo += torch.stack([zero.double(), mine.double()]) * len(items)
    finally:
        Fn.set_compute_dtype(keep_dtype)
    table = torch.stack([torch.cat(errs), torch.cat(idents)] + ([torch.cat(refined)] if a.refine else [])).double().cpu().tolist()       # the one read-back of the per-pair figures
    photo = (photo / len(pairs)).tolist()
    records = [{"stem": stem, "corner_error": e, "identity_corner_error": i} for stem, e, i in zip(cache.stems, table[0], table[1])]
    if a.refine:
        for r, e in zip(records, table[2]):
            r["refined_corner_error"] = e
    records.append(summarise(records, photo[0], photo[1]))
    for r in records:
        log(json.dumps(r))
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(records[-1]) + "\n")
    return records


if __name__ == "__main__":
    r = main()
    sys.exit(r if isinstance(r, int) else 0)

"""Stereo homography estimation on the GPU: the ``H`` every stereo pair of the HESIC scripts needs, without OpenCV.

The reference computes it per item in its loader with ``get_H`` (compressai/datasets/utils.py:30-66): OpenCV-contrib SURF keypoints,
``BFMatcher().knnMatch(k=2)`` with the 0.7 ratio test, ``cv2.findHomography(RANSAC, 5.0)``.  Here the same pipeline runs on batches of
same-size pairs in the HIP kernels of ``hesic_amd/csrc/stereo_h.hip`` (C ABI ``include/hesic_stereo_h.h``):

1. grey (OpenCV's ``cvtColor(BGR2GRAY)`` of the RGB array the reference hands SURF: channel 0 is read as blue, so the grey level is
   0.114 R + 0.587 G + 0.299 B) and an exact int32 integral image;
2. the Fast-Hessian detector with OpenCV SURF's defaults (4 octaves, 3 layers + 2, box filters 9/15/21/27/33 doubling per octave,
   ``hessianThreshold`` 100), 3x3x3 non-maximum suppression, sub-pixel / sub-scale quadratic fit; the strongest ``max_keypoints``;
3. SURF descriptors, by default **upright** and 64-d (U-SURF).  This departs from the reference, whose ``SURF_create()`` defaults
   to oriented 64-d SURF: the HESIC datasets are rectified side-by-side views with no in-plane rotation, where upright descriptors
   match better.  ``upright=False`` assigns each keypoint OpenCV SURF's dominant direction (109 Haar samples within 6 s, the longest
   sum over 60-degree windows) and describes it in that frame, which makes pairs with in-plane rotation usable; ``extended=True``
   gives the 128-d descriptor (each sum split by the sign of the other response).  ``upright=False, extended=False`` is the
   reference's configuration.  The descriptors keep the integral-image Haar form of U-SURF rather than OpenCV's resampled window;
4. 2-NN matching of view 1 (query) against view 2 (train) on the matrix cores, ratio test d1^2 < 0.49 d2^2;
5. RANSAC with a fixed number of hypotheses drawn by a counter hash of (seed, pair, hypothesis, draw), inlier bar 5 px;
6. a least-squares DLT over the best hypothesis's inliers and 10 Levenberg-Marquardt steps, as ``findHomography`` refines.

Every stage is deterministic: two runs give the same bits, and a pair's result depends only on its images, ``seed`` and its pair
number -- not on the other pairs of the batch.
"""
from __future__ import annotations

import argparse
import os
import sys
from pathlib import Path

import numpy as np
import torch

from . import _lib as L

__all__ = ["estimate_homography", "HipHomography", "write_sidecars", "MAX_KEYPOINTS"]

MAX_KEYPOINTS = 4096          # include/hesic_stereo_h.h HESIC_STEREO_H_MAX_KEYPOINTS


def _images(x, name):
    if x.dim() != 4 or x.shape[1] != 3:
        raise ValueError(f"estimate_homography: {name} must be (B, 3, H, W), got {tuple(x.shape)}")
    if x.dtype == torch.uint8:
        return x, 0
    if x.dtype != torch.float32:
        x = x.float()
    return x, 1


class _Workspace:
    """Device buffers of one batch shape, reused between calls of the same shape."""

    def __init__(self):
        self.key = None
        self.ws = None

    def get(self, B, H, W, max_kp, n_hyp, device):
        key = (B, H, W, max_kp, n_hyp, device)
        if self.key != key:
            nbytes = L.lib().hesic_stereo_h_ws_bytes(B, H, W, max_kp, n_hyp)
            self.ws = torch.empty(nbytes, dtype=torch.uint8, device=device)
            self.key = key
        return self.ws


def estimate_homography(img1, img2, *, max_keypoints=4096, hypotheses=2048, seed=0, first_pair=0, pair_ids=None, upright=True,
                        extended=False, return_details=False, _ws=None):
    """``H`` (left pixel -> right pixel) of B same-size stereo pairs.

    img1, img2: (B, 3, H, W) device tensors, uint8 or float in [0, 1] (quantised to uint8 as rint(x * 255) before the grey step).
    Returns ``(H, valid, inliers)``: (B, 3, 3) float32 with ``H[2, 2] = 1`` (zeros where invalid), (B,) bool, (B,) int32.  A pair is
    invalid where fewer than 4 matches survive the ratio test or no sample of 4 is non-degenerate -- where the reference's
    ``get_H`` returns None.  The RANSAC sampling of pair b is keyed by its pair number: ``pair_ids[b]`` (a sequence of B integers),
    or ``first_pair + b`` when ``pair_ids`` is not given.  Both views must have the same dtype.

    ``upright`` (default True): U-SURF, every keypoint described in the image axes; False: each keypoint gets its dominant direction
    and is described in that frame (rotation-invariant matching).  ``extended`` (default False): 64-d descriptors; True: 128-d.
    ``upright=False, extended=False`` is the reference's ``cv2.xfeatures2d.SURF_create()``; the defaults keep the upright 64-d path.

    ``return_details`` adds a dict of the stages: ``integral`` (2B, H+1, W+1) int32 (view 1, then view 2), ``hessian`` (2B, n) float32,
    ``keypoints`` / ``descriptors`` (lists of 2B tensors: [x, y, size, response] and 64- or 128-d), ``orientations`` (with
    ``upright=False``: list of 2B (n, 2) [cos, sin], x right and y down), ``matches`` (list of B (M, 2) int32 [query, train]),
    ``inlier_mask`` (list of B (M,) bool) and ``best`` (B,) the winning hypothesis."""
    if img1.dtype != img2.dtype:
        raise ValueError(f"estimate_homography: the two views differ in dtype ({img1.dtype} vs {img2.dtype}); pass both as uint8 "
                         "or both as float in [0, 1]")
    L.require_cuda(img1, img2)
    if img1.shape != img2.shape:
        raise ValueError(f"estimate_homography: the two views differ in shape ({tuple(img1.shape)} vs {tuple(img2.shape)})")
    a, fa = _images(img1, "img1")
    b, _ = _images(img2, "img2")
    if not 0 < max_keypoints <= MAX_KEYPOINTS:
        raise ValueError(f"estimate_homography: max_keypoints must be in [1, {MAX_KEYPOINTS}]")
    if hypotheses <= 0:
        raise ValueError("estimate_homography: hypotheses must be positive")
    B, _, H, W = a.shape
    dev = a.device
    K, NH = int(max_keypoints), int(hypotheses)
    s = L.stream()
    lib = L.lib()
    ids = list(range(first_pair, first_pair + B)) if pair_ids is None else [int(i) for i in pair_ids]
    if len(ids) != B:
        raise ValueError(f"estimate_homography: {len(ids)} pair_ids for {B} pairs")
    ws = (_ws or _Workspace()).get(B, H, W, K, NH, dev)
    pid = torch.tensor([i & 0xFFFFFFFF for i in ids], dtype=torch.int64).to(torch.int32).to(dev)
    I = torch.empty((2 * B, H + 1, W + 1), dtype=torch.int32, device=dev)
    for v, x in enumerate((a, b)):
        L.call("hesic_stereo_h_integral", L.ptr(x), fa, *x.stride(), B, H, W, L._vp(I.data_ptr() + v * B * I[0].numel() * 4), s)
    det = torch.empty((2 * B, lib.hesic_stereo_h_det_elems(H, W)), dtype=torch.float32, device=dev)
    L.call("hesic_stereo_h_hessian", L.ptr(I), 2 * B, H, W, L.ptr(det), s)
    kp = torch.empty((2 * B, K, 4), dtype=torch.float32, device=dev)
    n_kp = torch.empty((2 * B,), dtype=torch.int32, device=dev)
    L.call("hesic_stereo_h_keypoints", L.ptr(det), B, H, W, K, NH, L.ptr(ws), ws.numel(), L.ptr(kp), L.ptr(n_kp), s)
    D = 128 if extended else 64
    desc = torch.empty((2 * B, K, D), dtype=torch.float32, device=dev)
    nrm = torch.empty((2 * B, K), dtype=torch.float32, device=dev)
    matches = torch.empty((B, K, 2), dtype=torch.int32, device=dev)
    n_match = torch.empty((B,), dtype=torch.int32, device=dev)
    ori = None
    if upright and not extended:                       # U-SURF 64-d: the original entry points
        L.call("hesic_stereo_h_describe", L.ptr(I), L.ptr(kp), L.ptr(n_kp), 2 * B, H, W, K, L.ptr(desc), L.ptr(nrm), s)
        L.call("hesic_stereo_h_match", L.ptr(desc), L.ptr(nrm), L.ptr(n_kp), B, H, W, K, NH, L.ptr(ws), ws.numel(), L.ptr(matches),
               L.ptr(n_match), s)
    else:
        if not upright:
            ori = torch.empty((2 * B, K, 2), dtype=torch.float32, device=dev)
            L.call("hesic_stereo_h_orient", L.ptr(I), L.ptr(kp), L.ptr(n_kp), 2 * B, H, W, K, L.ptr(ori), s)
        L.call("hesic_stereo_h_describe_ex", L.ptr(I), L.ptr(kp), L.ptr(ori), L.ptr(n_kp), 2 * B, H, W, K, D, L.ptr(desc), L.ptr(nrm), s)
        L.call("hesic_stereo_h_match_ex", L.ptr(desc), L.ptr(nrm), L.ptr(n_kp), B, H, W, K, NH, D, L.ptr(ws), ws.numel(),
               L.ptr(matches), L.ptr(n_match), s)
    Hout = torch.empty((B, 3, 3), dtype=torch.float32, device=dev)
    valid = torch.empty((B,), dtype=torch.int32, device=dev)
    inliers = torch.empty((B,), dtype=torch.int32, device=dev)
    best = torch.empty((B,), dtype=torch.int32, device=dev)
    mask = torch.empty((B, K), dtype=torch.uint8, device=dev)
    L.call("hesic_stereo_h_ransac", L.ptr(kp), L.ptr(matches), L.ptr(n_match), B, H, W, K, NH, int(seed) & 0xFFFFFFFF,
           L.ptr(pid), L.ptr(ws), ws.numel(), L.ptr(Hout), L.ptr(valid), L.ptr(inliers), L.ptr(best), L.ptr(mask), s)
    out = (Hout, valid.bool(), inliers)
    if not return_details:
        return out
    nk, nm = n_kp.tolist(), n_match.tolist()
    details = {
        "integral": I, "hessian": det, "best": best,
        "keypoints": [kp[n, :nk[n]] for n in range(2 * B)],
        "descriptors": [desc[n, :nk[n]] for n in range(2 * B)],
        "matches": [matches[p, :nm[p]] for p in range(B)],
        "inlier_mask": [mask[p, :nm[p]].bool() for p in range(B)],
    }
    if ori is not None:
        details["orientations"] = [ori[n, :nk[n]] for n in range(2 * B)]
    return out + (details,)


class HipHomography:
    """``homography=`` callable of ``compressai.datasets.ImageFolder``: takes the loader's two uint8 (H, W, 3) crops, returns the 3x3
    float32 ``H`` (left crop pixel -> right crop pixel) or None where the estimate is invalid -- where the reference's ``get_H``
    returns None and its loader yields ``(img1, img2)``.  The device workspace is kept between calls of the same crop size.

    It runs on the GPU inside ``__getitem__``: use it with ``DataLoader(num_workers=0)``, or with worker processes started by
    ``multiprocessing_context="spawn"`` (a forked worker cannot use the parent's HIP context).  ``upright`` / ``extended`` select
    the descriptor as in ``estimate_homography``."""

    def __init__(self, device="cuda", max_keypoints=4096, hypotheses=2048, seed=0, upright=True, extended=False):
        self.device = torch.device(device)
        self.max_keypoints, self.hypotheses, self.seed = max_keypoints, hypotheses, seed
        self.upright, self.extended = upright, extended
        self._ws = _Workspace()

    def __call__(self, img1, img2):
        t1 = torch.from_numpy(np.ascontiguousarray(img1)).permute(2, 0, 1).unsqueeze(0).to(self.device)
        t2 = torch.from_numpy(np.ascontiguousarray(img2)).permute(2, 0, 1).unsqueeze(0).to(self.device)
        with torch.cuda.device(self.device):
            H, valid, _ = estimate_homography(t1, t2, max_keypoints=self.max_keypoints, hypotheses=self.hypotheses, seed=self.seed,
                                              upright=self.upright, extended=self.extended, _ws=self._ws)
        if not bool(valid[0]):
            return None
        return H[0].cpu().numpy()


# ---------------------------------------------------------------- sidecar writer
def _image_size(path):
    """(width, height) from the file header: nothing is decoded."""
    from PIL import Image
    with Image.open(path) as im:
        return im.size


def write_sidecars(root, splits=("train", "test"), batch=8, overwrite=False, estimator=None, seed=0, log=print, upright=True,
                   extended=False, refine=None):
    """Write ``root/<split>/H/<stem>.npy`` (fp64, the full images' H) for every pair of the stereo folder that has none (all with
    ``overwrite``).  Pairs are grouped by size from their file headers and estimated ``batch`` at a time; only the pairs of the current
    batch are decoded (with the loader's reader), so memory does not grow with the folder.  The RANSAC pair number of a pair is its
    index in the split's sorted file list, so its ``H`` depends neither on the batching nor on which sidecars already exist.  An invalid
    pair gets no file (the loader then yields ``(img1, img2)`` for it, as the reference does on a RANSAC failure).
    ``estimator(x1, x2, pair_ids) -> (H, valid)`` on (B, 3, H, W) uint8 CPU tensors replaces the GPU estimate; ``upright`` /
    ``extended`` select the descriptor of the GPU estimate as in ``estimate_homography``.
    ``refine``: None (default), or a dict of keyword arguments of ``homography.refine_h_matrix`` (``levels``, ``iters``, ``huber``,
    ``min_overlap``; ``{}`` for its defaults): every estimate is then refined photometrically on the pair's images (fp32 in [0, 1], on the
    GPU) before it is written, so whatever reads the sidecars -- the trainers, ``eval_folder``, ``codec encode`` -- gets the refined matrix.
    A pair the refiner cannot improve keeps its estimate; an invalid pair still gets no file.
    Returns (written, invalid, skipped)."""
    from .compressai.datasets import _read_rgb
    import glob
    written = invalid = skipped = 0
    for split in splits:
        d = Path(root) / split
        if not d.is_dir():
            continue
        lefts = sorted(glob.glob(os.path.join(d / "left", "*")))
        rights = sorted(glob.glob(os.path.join(d / "right", "*")))
        if len(lefts) != len(rights):
            raise RuntimeError(f"{d}: {len(lefts)} left images but {len(rights)} right images")
        hdir = d / "H"
        todo = {}                                      # (width, height) -> [(pair index, stem, left path, right path)]
        for i, (lf, rf) in enumerate(zip(lefts, rights)):
            if os.path.basename(lf) != os.path.basename(rf):
                raise ValueError(f"{d}: cannot pair {os.path.basename(lf)} with {os.path.basename(rf)}")
            stem = Path(lf).stem
            if not overwrite and (hdir / (stem + ".npy")).is_file():
                skipped += 1
                continue
            sa, sb = _image_size(lf), _image_size(rf)
            if sa != sb:
                raise ValueError(f"{os.path.basename(lf)}: the two views differ in size ({sa} vs {sb})")
            todo.setdefault(sa, []).append((i, stem, lf, rf))
        for items in todo.values():
            for c0 in range(0, len(items), batch):
                chunk = items[c0:c0 + batch]
                x1 = torch.from_numpy(np.stack([_read_rgb(lf) for _, _, lf, _ in chunk])).permute(0, 3, 1, 2)
                x2 = torch.from_numpy(np.stack([_read_rgb(rf) for _, _, _, rf in chunk])).permute(0, 3, 1, 2)
                ids = [i for i, _, _, _ in chunk]
                if estimator is not None:
                    Hs, ok = estimator(x1, x2, ids)
                else:
                    Hd, vd, _ = estimate_homography(x1.cuda(), x2.cuda(), seed=seed, pair_ids=ids, upright=upright, extended=extended)
                    Hs, ok = Hd.cpu().numpy(), vd.cpu().tolist()
                if refine is not None:
                    from . import homography
                    Hin = torch.from_numpy(np.asarray(Hs, dtype=np.float32).reshape(-1, 3, 3)).cuda()
                    Hs = homography.refine_h_matrix(x1.cuda().float() / 255.0, x2.cuda().float() / 255.0, Hin, **refine)[0].cpu().numpy()
                hdir.mkdir(exist_ok=True)
                for (_, stem, _, _), Hm, v in zip(chunk, Hs, ok):
                    if not v:
                        invalid += 1
                        continue
                    Hm = np.asarray(Hm, dtype=np.float64).reshape(3, 3)
                    np.save(hdir / (stem + ".npy"), Hm / Hm[2, 2])
                    written += 1
    log(f"stereo_h: {written} sidecars written, {invalid} pairs invalid (no file), {skipped} skipped (already present) under {root}")
    return written, invalid, skipped


def main(argv=None):
    p = argparse.ArgumentParser(prog="python -m hesic_amd.stereo_h",
                                description="Write ROOT/<split>/H/<stem>.npy (the full images' left -> right homography) for a stereo "
                                            "folder ROOT/<split>/{left,right}/, estimated on the GPU (SURF + RANSAC).")
    p.add_argument("root")
    p.add_argument("--split", nargs="+", default=["train", "test"])
    p.add_argument("--batch", type=int, default=8)
    p.add_argument("--overwrite", action="store_true")
    p.add_argument("--seed", type=int, default=0)
    p.add_argument("--oriented", action="store_true",
                   help="oriented SURF (rotation-invariant; the reference's SURF_create() default) instead of upright U-SURF")
    p.add_argument("--extended", action="store_true", help="128-d descriptors instead of 64-d")
    p.add_argument("--refine", action="store_true",
                   help="refine every estimate photometrically before it is written (homography.refine_h_matrix, its defaults); off by default")
    a = p.parse_args(argv)
    if not torch.cuda.is_available():
        print("stereo_h: needs a ROCm device (the estimator has no CPU path)", file=sys.stderr)
        return 2
    write_sidecars(a.root, a.split, a.batch, a.overwrite, seed=a.seed, upright=not a.oriented, extended=a.extended,
                   refine={} if a.refine else None)
    return 0


if __name__ == "__main__":
    sys.exit(main())

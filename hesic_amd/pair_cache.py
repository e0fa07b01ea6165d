"""Training batches from a stereo folder whose decoded pairs live on the device.

The loader's route (``compressai.datasets.ImageFolder`` behind a ``DataLoader``) decodes two image files, crops, divides by 255 and re-bases
the sidecar matrix per item on the host, every epoch.  ``DevicePairCache`` decodes every pair of ``ROOT/<split>/{left,right}/`` ONCE, keeps
the bytes as uint8 HWC in one device arena, the sidecar matrices ``ROOT/<split>/H/<stem>.npy|.txt`` as one fp64 (N, 9) device table, and turns
a list of (pair, crop origin) into ``(x1, x2, h_matrix)`` with one launch (``hesic_pair_batch_gather``, include/hesic_pair_batch.h): the same
bits ``ImageFolder`` + ``ToTensor`` give.  The same launch flips a crop or exchanges its views, the homography with them, where the plan says
so (``epoch_plan(..., augment=...)``, ``batch(..., flags=...)``; ``hesic_pair_batch_gather_aug``, include/hesic_pair_augment.h).  A set that
does not fit the memory budget is served in ``"stream"`` mode instead: per batch the host reads and crops the bytes, uploads them into a
reused staging slab and runs the same kernel on the slab.  The host ``ImageFolder`` loader does not augment.  ``homonet_batch`` serves
HomographyNet the same way: its grey frames, windows and corners straight from the stored bytes in one launch
(``hesic_homonet_prepare_items``, include/hesic_homonet_items.h), any crop per item, pairs of different sizes in one batch.

``crop_origin`` is the loader's crop rule and ``epoch_plan`` the order and crops of one epoch; both depend on nothing but their arguments.
"""
from __future__ import annotations

import os
import random
import time
from concurrent.futures import ThreadPoolExecutor
from pathlib import Path

import numpy as np
import torch

ARENA_ALIGN = 256           # every stored view starts at a multiple of this (the device allocator's own alignment)
H_ROW_BYTES = 9 * 8         # one fp64 3 x 3 matrix of the sidecar table


def _align(n):
    return (int(n) + ARENA_ALIGN - 1) // ARENA_ALIGN * ARENA_ALIGN


def bytes_needed(sizes, n_matrices=0):
    """Device bytes of a ``"device"``-mode cache of pairs with the image sizes ``sizes`` = [(height, width)]: two views of
    ``height * width * 3`` bytes per pair, each rounded up to 256, plus 72 bytes per sidecar matrix.  A pure host function."""
    return sum(2 * _align(h * w * 3) for h, w in sizes) + H_ROW_BYTES * int(n_matrices)


def check_budget(needed, budget):
    """Refuse a set that does not fit, before anything is allocated."""
    if needed > budget:
        raise MemoryError(f"DevicePairCache: the decoded pairs need {needed} bytes of device memory but the budget is {budget} bytes -- "
                          'raise budget_bytes (--cache-gb) or use mode="stream" (--cache stream), which keeps the files on the host')


def crop_origin(rng, Himg, Wimg, ph, pw):
    """``(y0, x0)`` of one item's crop, the loader's rule exactly (``ImageFolder.__getitem__``; reference utils.py:147-152): no offset at
    all when the patch has the image's height, else ``y0 = randint(0, Himg - ph - 1)`` then ``x0 = randint(0, max(Wimg - pw - 1, 0))`` --
    the last row and column offsets are never drawn.  ``rng``: a ``random.Random`` (or the ``random`` module)."""
    if ph > Himg or pw > Wimg:
        raise ValueError(f"crop_origin: patch ({ph}, {pw}) larger than the image ({Himg}, {Wimg})")
    if ph == Himg:
        return 0, 0
    y0 = rng.randint(0, Himg - ph - 1)
    x0 = rng.randint(0, max(Wimg - pw - 1, 0))
    return y0, x0


class Plan(list):
    """``[(indices, origins)]`` of one epoch -- ``origins[i] = (y0, x0)`` of pair ``indices[i]`` -- with ``left_out`` (pairs not in ``keep``),
    ``dropped`` (pairs of a ragged tail batch dropped under ``drop_tail``), ``rng``, the epoch's random stream after the plan's draws, and
    ``flags``: per batch the items' augmentation bits (``AUGMENT_BITS``), a list parallel to the plan, all zeros when nothing is enabled."""
    left_out = 0
    dropped = 0
    rng = None
    flags = ()

    def augmented(self):
        """``{name: items of the plan with that flag set}``, in ``AUGMENT_BITS`` order."""
        return {name: sum(1 for fl in self.flags for f in fl if f & bit) for name, bit in AUGMENT_BITS.items()}


AUGMENT_BITS = {"hflip": 1, "vflip": 2, "swap": 4}      # HESIC_PAIR_HFLIP, HESIC_PAIR_VFLIP, HESIC_PAIR_SWAP (include/hesic_pair_augment.h)


def epoch_plan(n_pairs, sizes, batch_size, ph, pw, seed, epoch, shuffle, drop_tail, keep=None, augment=()):
    """The batches of one epoch over pairs ``0 .. n_pairs - 1`` with the image sizes ``sizes`` = [(height, width)].  The random stream is
    ``random.Random(f"{seed}/{epoch}")``; ``epoch=None`` is the validation stream, keyed by the seed alone (every epoch is judged on the
    same crops).  Order of the draws: the shuffle of the kept pairs (when ``shuffle``), then one ``crop_origin`` per pair in batch order.
    ``keep``: the pair indices that take part (default: all; the folder trainer leaves out pairs without a sidecar).  ``drop_tail``
    drops a last batch of fewer than ``batch_size`` pairs.  The result depends on nothing but the arguments.

    ``augment``: a collection drawn from ``"hflip"``, ``"vflip"``, ``"swap"`` -- the stereo-aware augmentations the gather applies
    (``DevicePairCache.batch(flags=...)``).  The items' flags come from a SECOND stream, ``random.Random(f"{seed}/{epoch}/augment")``: one
    ``getrandbits(1)`` per enabled flag per item, in batch order and in the order hflip, vflip, swap; so the shuffle, the crops and ``rng``
    after the plan are the same with and without augmentation.  Validation (``epoch=None``) is never augmented: the combination is refused."""
    n_pairs, batch_size = int(n_pairs), int(batch_size)
    augment = [augment] if isinstance(augment, str) else list(augment)
    unknown = [a for a in augment if a not in AUGMENT_BITS]
    if unknown:
        raise ValueError(f"epoch_plan: augment names {unknown[0]!r}; it is drawn from {list(AUGMENT_BITS)}")
    if augment and epoch is None:
        raise ValueError("epoch_plan: the validation plan (epoch=None) is never augmented")
    enabled = [bit for name, bit in AUGMENT_BITS.items() if name in augment]
    if len(sizes) != n_pairs:
        raise ValueError(f"epoch_plan: {len(sizes)} sizes for {n_pairs} pairs")
    if batch_size < 1:
        raise ValueError("epoch_plan: batch_size must be positive")
    order = list(range(n_pairs)) if keep is None else sorted({int(i) for i in keep})
    if order and not 0 <= order[0] <= order[-1] < n_pairs:
        raise ValueError(f"epoch_plan: keep names a pair outside [0, {n_pairs})")
    rng = random.Random(f"{seed}/valid" if epoch is None else f"{seed}/{int(epoch)}")
    if shuffle:
        rng.shuffle(order)
    arng = random.Random(f"{seed}/{int(epoch)}/augment") if enabled else None
    plan = Plan()
    plan.flags = []
    plan.left_out = n_pairs - len(order)
    if drop_tail and len(order) % batch_size:
        plan.dropped = len(order) % batch_size
        order = order[:len(order) - plan.dropped]
    for c0 in range(0, len(order), batch_size):
        idx = order[c0:c0 + batch_size]
        plan.append((idx, [crop_origin(rng, sizes[i][0], sizes[i][1], ph, pw) for i in idx]))
        plan.flags.append([sum(bit for bit in enabled if arng.getrandbits(1)) for _ in idx])
    plan.rng = rng
    return plan


def _sidecar_path(hdir, stem):
    for ext in (".npy", ".txt"):
        f = hdir / (stem + ext)
        if f.is_file():
            return f
    return None


def _read_sidecar(path):
    H = np.load(path) if path.suffix == ".npy" else np.loadtxt(path)
    return np.asarray(H, dtype=np.float64).reshape(9)


class DevicePairCache:
    """The pairs of ``ROOT/<split>`` (listed by ``codec._pairs``, decoded by the loader's ``_read_rgb``) behind ``batch()``.

    ``mode="device"``: every pair is decoded once by ``workers`` host threads (the reference's ``-n``, default 3) into one uint8 device
    arena, views at 256-byte-aligned offsets.  ``budget_bytes`` defaults to HALF of the free device memory ``torch.cuda.mem_get_info()``
    reports (the device is shared); a set whose ``bytes_needed`` exceeds it is refused before any allocation.
    ``mode="stream"``: nothing is kept; ``batch()`` reads and crops on the host and uploads the crops into a reused slab.

    Attributes: ``stems``, ``sizes`` [(height, width)], ``has_h`` [bool] (a sidecar exists), ``h_host`` the fp64 (N, 9) table on the host
    (``h_index[i]`` its row for pair i, -1 without a sidecar), ``decode_seconds``."""

    def __init__(self, root, split, mode="device", budget_bytes=None, workers=3, device=None):
        from .codec import _pairs
        from .stereo_h import _image_size
        if mode not in ("device", "stream"):
            raise ValueError(f'DevicePairCache: mode is "device" or "stream", got {mode!r}')
        if int(workers) < 1:
            raise ValueError("DevicePairCache: workers must be positive")
        self.mode, self.workers = mode, int(workers)
        hdir = Path(root) / split / "H"
        self.stems, self.files, self.sizes, self.has_h, self.h_index, rows = [], [], [], [], [], []
        for stem, lf, rf, _ in _pairs(root, split):
            (w, h), sb = _image_size(lf), _image_size(rf)
            if (w, h) != sb:
                raise ValueError(f"{os.path.basename(lf)}: the two views differ in size ({(w, h)} vs {sb})")
            side = _sidecar_path(hdir, stem)
            self.stems.append(stem)
            self.files.append((lf, rf))
            self.sizes.append((h, w))
            self.has_h.append(side is not None)
            self.h_index.append(len(rows) if side is not None else -1)
            if side is not None:
                rows.append(_read_sidecar(side))
        self.h_host = np.stack(rows) if rows else np.zeros((0, 9), dtype=np.float64)
        self.device = None if device is None else torch.device(device)
        self.h_table = self.arena = self.offsets = None
        self.decode_seconds = 0.0
        self._slab = self._slab_host = self._slab_event = None
        if torch.cuda.is_available():
            self._to_device(budget_bytes)
        elif mode == "device":
            raise RuntimeError("hesic_amd: the HIP path needs a ROCm device (no CPU fallback)")

    def __len__(self):
        return len(self.stems)

    def _read(self, i):
        from .compressai.datasets import _read_rgb
        lf, rf = self.files[i]
        a, b = _read_rgb(lf), _read_rgb(rf)
        h, w = self.sizes[i]
        if a.shape != (h, w, 3) or b.shape != (h, w, 3):
            raise ValueError(f"{os.path.basename(lf)}: decoded to {a.shape} / {b.shape}, listed as {(h, w, 3)}")
        return a, b

    def _to_device(self, budget_bytes):
        if self.device is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        if self.mode == "device":
            needed = bytes_needed(self.sizes, len(self.h_host))
            if budget_bytes is None:
                budget_bytes = torch.cuda.mem_get_info(self.device)[0] // 2
            check_budget(needed, int(budget_bytes))
        if len(self.h_host):
            self.h_table = torch.from_numpy(self.h_host).to(self.device)
        if self.mode != "device":
            return
        self.offsets, off = [], 0
        for h, w in self.sizes:
            n = _align(h * w * 3)
            self.offsets.append((off, off + n))
            off += 2 * n
        self.arena = torch.empty(off, dtype=torch.uint8, device=self.device)
        t0 = time.time()
        with ThreadPoolExecutor(max_workers=self.workers) as pool:
            for i, (a, b) in enumerate(pool.map(self._read, range(len(self)))):
                for view, o in zip((a, b), self.offsets[i]):
                    self.arena[o:o + view.size].copy_(torch.from_numpy(view.reshape(-1)))
        torch.cuda.synchronize(self.device)
        self.decode_seconds = time.time() - t0

    def _stream_bytes(self, n):
        """The first ``n`` bytes of the reused device slab and of its pinned host twin, both grown when the batch at hand needs more."""
        if self._slab is None or self._slab.numel() < n:
            self._slab = torch.empty(n, dtype=torch.uint8, device=self.device)
            self._slab_host = torch.empty(n, dtype=torch.uint8).pin_memory()
            self._slab_event = torch.cuda.Event()
        else:
            self._slab_event.synchronize()              # the previous batch's upload has left the pinned buffer
        return self._slab[:n], self._slab_host[:n]

    def batch(self, indices, origins, ph, pw, out=None, flags=None):
        """``(x1, x2, h, has_h)`` of the pairs ``indices`` cropped at ``origins`` = [(y0, x0)]: fp32 (B,3,ph,pw) twice, the crop-frame
        homographies (B,3,3) -- the identity where a pair has no sidecar -- and a (B,) bool host tensor telling which rows came from a
        sidecar.  Pairs of different image sizes share a batch.  ``out``: dense fp32 ``(x1, x2, h)`` to write into.
        ``flags``: per item a combination of ``AUGMENT_BITS`` (``epoch_plan(..., augment=...)``'s ``plan.flags[k]``): the crop is flipped and
        / or its views exchanged, the homography with them, by the same single launch (``hesic_pair_batch_gather_aug``,
        include/hesic_pair_augment.h; in ``"stream"`` mode the host uploads the plain crops and the kernel flips them on the slab).  ``None``
        or all zeros is the plain gather, the same call as without the argument."""
        from . import functional as Fn
        indices, ph, pw = [int(i) for i in indices], int(ph), int(pw)
        B = len(indices)
        if B < 1 or len(origins) != B:
            raise ValueError(f"DevicePairCache.batch: {B} indices and {len(origins)} origins")
        flags = [0] * B if flags is None else [int(f) for f in flags]
        if len(flags) != B:
            raise ValueError(f"DevicePairCache.batch: {B} indices and {len(flags)} flags")
        geo = self._crops("batch", indices, origins, [(ph, pw)] * B, sized=False)      # a patch of no pixels: the gather's "bad shape"
        items = Fn.pair_items(B)
        items["reserved"] = flags
        pairs, items["hy"], items["hx"], _, _ = zip(*geo)
        items["h_index"] = [self.h_index[i] for i in pairs]
        self._place(items, geo, (0, 1), ("left", "right"))
        gather = Fn.pair_batch_gather_aug if any(flags) else Fn.pair_batch_gather
        x1, x2, hm = gather(items, self.h_table, ph, pw, out=out)
        return x1, x2, hm, torch.tensor([self.has_h[i] for i in indices], dtype=torch.bool)

    def _crops(self, name, indices, origins, sizes, sized=True):
        """``[(pair, y0, x0, ch, cw)]`` of a batch, checked against the listing: every pair listed, every crop inside its pair's image and,
        when ``sized``, of at least one pixel each way (``name``: the calling method).  ``sizes=None``: every whole image at (0, 0)."""
        geo = []
        for b, i in enumerate(indices):
            if not 0 <= i < len(self):
                raise IndexError(f"DevicePairCache.{name}: pair {i} outside [0, {len(self)})")
            h, w = self.sizes[i]
            (y0, x0), (ch, cw) = ((0, 0), (h, w)) if sizes is None else (origins[b], sizes[b])
            y0, x0, ch, cw = int(y0), int(x0), int(ch), int(cw)
            if not ((not sized or (ch >= 1 and cw >= 1)) and 0 <= x0 and x0 + cw <= w and 0 <= y0 and y0 + ch <= h):
                raise ValueError(f"DevicePairCache.{name}: crop ({ch}, {cw}) at ({y0}, {x0}) outside pair {i}'s image ({h}, {w})")
            geo.append((i, y0, x0, ch, cw))
        return geo

    def _place(self, items, geo, views, fields):
        """Point the descriptors at their crops: per item the address of each of ``views`` (0: left, 1: right) in the field of ``fields`` that
        goes with it, and the geometry of what that address holds -- the stored image in the arena, or the crop packed into the slab."""
        if self.mode != "device":
            return self._stream_crops(items, geo, views, fields)
        base, (pairs, y0, x0, _, _) = self.arena.data_ptr(), zip(*geo)          # a column per field: an assignment per item costs twice the time
        for f, v in zip(fields, views):
            items[f] = [base + self.offsets[i][v] for i in pairs]
        items["pitch_px"], items["rows"] = [self.sizes[i][1] for i in pairs], [self.sizes[i][0] for i in pairs]
        items["x0"], items["y0"] = x0, y0

    def _homonet_geometry(self, name, indices, origins, sizes, windows):
        """The crops of a HomographyNet batch (``_crops``) after the count check its two methods share."""
        indices = [int(i) for i in indices]
        B = len(indices)
        if B < 1 or len(windows) != B or (sizes is None and origins is not None and len(origins) != B) or \
                (sizes is not None and (len(sizes) != B or len(origins) != B)):
            raise ValueError(f"DevicePairCache.{name}: {B} indices need as many origins, sizes and windows")
        return self._crops(name, indices, origins, sizes)

    def _homonet_place(self, items, geo, windows, views, fields):
        """The crop sizes and windows of a HomographyNet batch into its descriptors, then ``_place``."""
        _, _, _, items["ch"], items["cw"] = zip(*geo)
        items["wx"], items["wy"] = zip(*((int(wx), int(wy)) for wx, wy in windows))
        self._place(items, geo, views, fields)

    def homonet_batch(self, indices, origins, sizes, windows, pic_size, patch_size, out=None):
        """HomographyNet's inputs ``(grey1, grey2, patch1, patch2, corners)`` of the pairs ``indices``, straight from the stored bytes in
        one launch (``hesic_homonet_prepare_items``, include/hesic_homonet_items.h): pair ``indices[i]`` cropped at ``origins[i]`` =
        (y0, x0) to ``sizes[i]`` = (ch, cw) -- ``sizes=None``: every whole image, at origin (0, 0) whatever ``origins`` holds --, resized to
        ``pic_size``², with the ``patch_size``² window at ``windows[i]`` = (wx, wy).  Pairs and crops of different sizes share a batch.
        ``"stream"`` mode reads and crops on the host, packs the crops back to back into the reused slab and runs the same kernel on it.
        ``out``: five dense fp32 tensors to write into."""
        from . import functional as Fn
        from .compressai.datasets import MEAN, STD
        geo = self._homonet_geometry("homonet_batch", indices, origins, sizes, windows)
        items = Fn.homonet_items(len(geo))
        self._homonet_place(items, geo, windows, (0, 1), ("left", "right"))
        return Fn.homonet_prepare_items(items, pic_size, patch_size, float(MEAN), float(STD), out=out)

    def _stream_crops(self, items, geo, views, fields):
        """``"stream"`` mode: read the batch's pairs on the host, pack the crops of ``views`` (0: left, 1: right) back to back into the reused
        slab, start the upload, put each crop's address into the descriptor field of ``fields`` that goes with its view, and re-base the
        descriptors' geometry onto the packed crops."""
        nbytes = [ch * cw * 3 for _, _, _, ch, cw in geo]
        slab, host = self._stream_bytes(len(fields) * sum(nbytes))
        flat = host.numpy()
        with ThreadPoolExecutor(max_workers=self.workers) as pool:
            off = 0
            for it, (_, y0, x0, ch, cw), n, pair in zip(items, geo, nbytes, pool.map(self._read, [g[0] for g in geo])):
                for f, v in zip(fields, views):
                    flat[off:off + n].reshape(ch, cw, 3)[...] = pair[v][y0:y0 + ch, x0:x0 + cw]
                    it[f] = slab.data_ptr() + off
                    off += n
                it["pitch_px"], it["rows"], it["x0"], it["y0"] = cw, ch, 0, 0
        slab.copy_(host, non_blocking=True)
        self._slab_event.record()

    def homonet_synth_batch(self, indices, origins, sizes, windows, deltas, pic_size, patch_size, view="left", out=None):
        """Synthetic-warp pairs ``(grey_a, patch_a, corners, delta, h, grey_b, patch_b)`` from ONE view of the pairs ``indices``, straight from
        the stored bytes (``hesic_homonet_synth_items``, include/hesic_homonet_synth.h): crops, sizes and windows as in ``homonet_batch``,
        ``deltas[i]`` the eight integer corner offsets of item i (``homography.draw_deltas``), ``view`` = ``"left"`` or ``"right"``; the
        sampling convention is ``geometry.DEFAULT_ALIGN_CORNERS``, what ``homography.photometric_loss`` samples in.  ``"stream"`` mode reads
        on the host and uploads only that view's crops.  ``out``: seven dense tensors to write into."""
        from . import functional as Fn
        from . import geometry
        from .compressai.datasets import MEAN, STD
        if view not in ("left", "right"):
            raise ValueError(f'DevicePairCache.homonet_synth_batch: view is "left" or "right", got {view!r}')
        geo = self._homonet_geometry("homonet_synth_batch", indices, origins, sizes, windows)
        if len(deltas) != len(geo) or any(len(d) != 8 for d in deltas):
            raise ValueError(f"DevicePairCache.homonet_synth_batch: {len(geo)} indices need as many deltas of eight integers")
        items = Fn.homonet_synth_items(len(geo))
        items["delta"] = [[int(v) for v in d] for d in deltas]
        self._homonet_place(items, geo, windows, (int(view == "right"),), ("view",))
        return Fn.homonet_synth(items, pic_size, patch_size, float(MEAN), float(STD), geometry.DEFAULT_ALIGN_CORNERS, out=out)

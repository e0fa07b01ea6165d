"""``python -m hesic_amd.codec``: code a stereo folder to ``.hsd`` blobs and back, on the GPU.

    encode ROOT OUT [--split test] [--batch 8] [--checkpoint PATH] [--model hesic|joint] [--homography sidecar|net] [--homography-checkpoint PATH]
                    [--refine-homography [--refine-levels 3] [--refine-iters 10] [--refine-huber DELTA]]
                                                                      ROOT/<split>/{left,right}/ + ROOT/<split>/H/<stem>.npy
                                                                      (the sidecars ``python -m hesic_amd.stereo_h`` writes)
                                                                      -> OUT/<stem>.hsd + OUT/<stem>.json, one JSON line of totals
    decode OUT RECON [--batch 8] [--checkpoint PATH] [--model hesic|joint]
                                                                      -> RECON/<stem>_left.png, RECON/<stem>_right.png

``.hsd`` is the container of ``hesic_amd.bitstream`` (``HSIC.compress_batch``; with ``--model joint`` HESIC+, ``HSICJoint.compress_batch``:
the blob names its kind, and a decoder of the other model refuses it).  The homography is side information of the codec, as
in the reference's flow: it travels in ``<stem>.json`` next to the blob, with the original image size (images are zero-padded to
multiples of 64 for coding and cropped back).  Pairs without a sidecar are skipped and counted.  Without ``--checkpoint`` the
deterministic synthetic weights are used (both sides must use the same weights and the same ``--dtype``).

``--homography net`` takes the matrix from HomographyNet instead, as the reference's final configuration does for every pair
(``homography.h_matrix_from_pair``: the centre window of the unpadded images, on the device): no sidecars are needed and no pair is skipped.
``--homography-checkpoint`` names the net's weights (a ``homo_best.pth.tar`` or what ``python -m hesic_amd.homography_train`` writes); without
it the deterministic synthetic weights.  The decoder reads the matrix from ``<stem>.json`` either way.

``--refine-homography`` refines the matrix -- the sidecar's or the net's -- photometrically on the unpadded originals before it is used
(``homography.refine_h_matrix``: Gauss-Newton / Levenberg-Marquardt on the grey residual, ``--refine-levels`` pyramid levels of
``--refine-iters`` candidates, ``--refine-huber`` for a robust weight).  ``<stem>.json`` then carries the refined matrix with
``"h_refined": true`` and the pair's mean squared grey residual before and after (``photometric_before``, ``photometric_after``; equal where
the refinement kept the input).  Off by default; ``decode`` needs no option.
"""
from __future__ import annotations

import argparse
import glob
import json
import os
import struct
import sys
import time
from pathlib import Path

import numpy as np
import torch

_DTYPES = {"f16": torch.float16, "bf16": torch.bfloat16, "f32": torch.float32}


def load_model(checkpoint=None, dtype=torch.float16, device="cuda", model="hesic"):
    import hesic_amd
    from . import models, synthetic
    hesic_amd.set_compute_dtype(dtype)
    net = {"hesic": models.HSIC, "joint": models.HSICJoint}[model]()
    if checkpoint:
        state = torch.load(checkpoint, map_location="cpu")
        net.load_state_dict(state.get("state_dict", state) if isinstance(state, dict) else state)
    else:
        synthetic.fill_state_dict_(net.state_dict())
    net = net.to(device).eval()
    net.update(force=True)
    return net


def load_homography_net(checkpoint=None, device="cuda"):
    """HomographyNet for ``encode --homography net``: fp32 maps, eval mode; the checkpoint's weights or the deterministic synthetic ones."""
    from . import homography, synthetic
    hnet = homography.Net()
    if checkpoint:
        homography.load_checkpoint(hnet, checkpoint)
    else:
        synthetic.fill_homography_state_dict_(hnet.state_dict())
    return hnet.to(device).eval()


def _pairs(root, split):
    """[(stem, left path, right path, H path or None)] of ROOT/<split>, in sorted order."""
    d = Path(root) / split
    lefts, rights = sorted(glob.glob(str(d / "left" / "*"))), sorted(glob.glob(str(d / "right" / "*")))
    if not lefts or len(lefts) != len(rights):
        raise RuntimeError(f"{d}: {len(lefts)} left and {len(rights)} right images")
    out = []
    for lf, rf in zip(lefts, rights):
        if os.path.basename(lf) != os.path.basename(rf):
            raise ValueError(f"{d}: cannot pair {os.path.basename(lf)} with {os.path.basename(rf)}")
        hp = d / "H" / (Path(lf).stem + ".npy")
        out.append((Path(lf).stem, lf, rf, hp if hp.is_file() else None))
    return out


def read_image(path):
    """(3, H, W) float32 in [0, 1] of an image file (the loader's reader)."""
    from .compressai.datasets import _read_rgb
    return torch.from_numpy(_read_rgb(path)).permute(2, 0, 1).float() / 255.0


def quantise(x):
    """Reconstruction -> (B, H, W, 3) uint8, what the PNGs hold."""
    return (x.float().clamp(0, 1) * 255).round().to(torch.uint8).permute(0, 2, 3, 1).cpu().numpy()


def encode_folder(net, root, out, split="test", batch=8, channels_per_stream=8, log=print, homography_net=None, z_coder="host", refine=None):
    """``homography_net=None``: the matrices come from the sidecars; a ``homography.Net``: from the net, for every pair.  ``z_coder``: who
    codes the z strings (``compress_batch``); the files are the same bytes either way.  ``refine``: None, or the keyword arguments of
    ``homography.refine_h_matrix`` (``levels``, ``iters``, ``huber``) to refine every matrix on the unpadded pair first."""
    from . import homography
    from .models import pad_to_multiple
    from .stereo_h import _image_size
    out = Path(out)
    out.mkdir(parents=True, exist_ok=True)
    groups, skipped = {}, 0
    for stem, lf, rf, hp in _pairs(root, split):
        if hp is None and homography_net is None:
            skipped += 1
            continue
        sa, sb = _image_size(lf), _image_size(rf)
        if sa != sb:
            raise ValueError(f"{os.path.basename(lf)}: the two views differ in size ({sa} vs {sb})")
        groups.setdefault(sa, []).append((stem, lf, rf, hp))
    n, bpp_sum, nbytes, t0 = 0, 0.0, 0, time.time()
    for (w, h), items in groups.items():
        for c0 in range(0, len(items), batch):
            chunk = items[c0:c0 + batch]
            x1 = pad_to_multiple(torch.stack([read_image(lf) for _, lf, _, _ in chunk])).cuda()
            x2 = pad_to_multiple(torch.stack([read_image(rf) for _, _, rf, _ in chunk])).cuda()
            if homography_net is not None:             # on the images as they are (a strided view): the padding is not part of the frame
                Hm = homography.h_matrix_from_pair(homography_net, x1[..., :h, :w], x2[..., :h, :w], "centre")
                Hs = list(Hm.double().cpu().numpy())
            else:
                Hs = [np.load(hp).astype(np.float64).reshape(3, 3) for _, _, _, hp in chunk]
                Hm = torch.from_numpy(np.stack(Hs)).float().cuda()
            extra = [{}] * len(chunk)
            if refine is not None:
                Hm, info = homography.refine_h_matrix(x1[..., :h, :w], x2[..., :h, :w], Hm, **refine)
                Hs = list(Hm.double().cpu().numpy())
                extra = [{"h_refined": True, "photometric_before": b, "photometric_after": a}
                         for b, a in zip(info["cost_before"].cpu().tolist(), info["cost_after"].cpu().tolist())]
            enc = net.compress_batch(x1, x2, Hm, channels_per_stream=channels_per_stream, z_coder=z_coder)
            for (stem, _, _, _), blob, Hn, ex in zip(chunk, enc["blobs"], Hs, extra):
                (out / (stem + ".hsd")).write_bytes(blob)
                (out / (stem + ".json")).write_text(json.dumps({"height": h, "width": w, "h_matrix": Hn.reshape(-1).tolist(), **ex}))
                n += 1
                nbytes += len(blob)
                bpp_sum += len(blob) * 8 / (2 * h * w)               # against the ORIGINAL pixels of the two views
    torch.cuda.synchronize()
    dt = time.time() - t0
    res = {"pairs": n, "skipped_no_sidecar": skipped, "bytes": nbytes, "mean_bpp": bpp_sum / max(n, 1), "seconds": dt, "pairs_per_s": n / dt if dt > 0 else 0.0}
    log(json.dumps(res))
    return res


def decode_folder(net, src, recon, batch=8, log=print, z_coder="host"):
    from PIL import Image
    src, recon = Path(src), Path(recon)
    recon.mkdir(parents=True, exist_ok=True)
    groups = {}
    for f in sorted(src.glob("*.hsd")):
        blob = f.read_bytes()
        side = f.with_suffix(".json")
        if len(blob) < 10 or not side.is_file():
            raise ValueError(f"{f}: not an .hsd blob with its .json side file")
        groups.setdefault(struct.unpack("<HH", blob[6:10]), []).append((f.stem, blob, json.loads(side.read_text())))
    n, t0 = 0, time.time()
    for items in groups.values():
        for c0 in range(0, len(items), batch):
            chunk = items[c0:c0 + batch]
            Hm = torch.tensor([s["h_matrix"] for _, _, s in chunk], dtype=torch.float64).reshape(-1, 3, 3).float().cuda()
            dec = net.decompress_batch([b for _, b, _ in chunk], Hm, z_coder=z_coder)
            q1, q2 = quantise(dec["x1_hat"]), quantise(dec["x2_hat"])
            for i, (stem, _, s) in enumerate(chunk):
                h, w = int(s["height"]), int(s["width"])
                Image.fromarray(q1[i, :h, :w]).save(recon / (stem + "_left.png"))
                Image.fromarray(q2[i, :h, :w]).save(recon / (stem + "_right.png"))
                n += 1
    dt = time.time() - t0
    res = {"pairs": n, "seconds": dt, "pairs_per_s": n / dt if dt > 0 else 0.0}
    log(json.dumps(res))
    return res


def main(argv=None):
    p = argparse.ArgumentParser(prog="python -m hesic_amd.codec", description="HESIC stereo folder <-> .hsd blobs, range-coded on the GPU.")
    sub = p.add_subparsers(dest="cmd", required=True)
    e = sub.add_parser("encode", help="ROOT/<split>/{left,right,H}/ -> OUT/<stem>.hsd")
    e.add_argument("root")
    e.add_argument("out")
    e.add_argument("--split", default="test")
    e.add_argument("--channels-per-stream", type=int, default=8)
    e.add_argument("--homography", choices=("sidecar", "net"), default="sidecar",
                   help="sidecar: ROOT/<split>/H/<stem>.npy (default); net: HomographyNet on every pair (no sidecars needed)")
    e.add_argument("--homography-checkpoint", default=None, help="HomographyNet weights for --homography net (default: synthetic weights)")
    e.add_argument("--refine-homography", action="store_true",
                   help="refine every matrix photometrically on the unpadded pair before coding (homography.refine_h_matrix); off by default")
    e.add_argument("--refine-levels", type=int, default=3, help="pyramid levels of --refine-homography")
    e.add_argument("--refine-iters", type=int, default=10, help="candidates per level of --refine-homography")
    e.add_argument("--refine-huber", type=float, default=None, help="Huber threshold of --refine-homography in grey levels of [0, 1] (default: plain L2)")
    d = sub.add_parser("decode", help="OUT/<stem>.hsd -> RECON/<stem>_{left,right}.png")
    d.add_argument("out")
    d.add_argument("recon")
    for s in (e, d):
        s.add_argument("--batch", type=int, default=8)
        s.add_argument("--checkpoint", default=None)
        s.add_argument("--dtype", choices=sorted(_DTYPES), default="f16")
        s.add_argument("--model", choices=("hesic", "joint"), default="hesic", help="hesic: HSIC (default); joint: HESIC+ (HSICJoint)")
        s.add_argument("--z-coder", choices=("host", "device"), default="host",
                       help="who codes the z strings: the host rANS coder (default) or the device one; same bytes, same reconstructions")
    a = p.parse_args(argv)
    if not torch.cuda.is_available():
        print("codec: needs a ROCm device (the range coder has no CPU path)", file=sys.stderr)
        return 2
    if a.batch < 1:
        p.error("--batch must be positive")
    net = load_model(a.checkpoint, _DTYPES[a.dtype], model=a.model)
    if a.cmd == "encode":
        if a.homography_checkpoint and a.homography != "net":
            p.error("--homography-checkpoint needs --homography net")
        if not a.refine_homography and (a.refine_levels != 3 or a.refine_iters != 10 or a.refine_huber is not None):
            p.error("--refine-levels, --refine-iters and --refine-huber need --refine-homography")
        hnet = load_homography_net(a.homography_checkpoint) if a.homography == "net" else None
        refine = {"levels": a.refine_levels, "iters": a.refine_iters, "huber": a.refine_huber} if a.refine_homography else None
        encode_folder(net, a.root, a.out, a.split, a.batch, a.channels_per_stream, homography_net=hnet, z_coder=a.z_coder, refine=refine)
    else:
        decode_folder(net, a.out, a.recon, a.batch, z_coder=a.z_coder)
    return 0


if __name__ == "__main__":
    sys.exit(main())

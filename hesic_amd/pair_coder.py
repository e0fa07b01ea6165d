"""The real bit-streams of HESIC (``models.HSIC``) and HESIC+ (``models.HSICJoint``): the ``.bin`` payload container, the z-string helpers
and ``PairCoder``, the mixin that gives both models ``compress`` / ``decompress`` (one pair, host range coder; reference
ywz/mywork/newnet1.py:823-1273 and newnet1_joint.py:793-1321) and ``compress_batch`` / ``decompress_batch`` (B pairs, device range coder,
one ``bitstream`` blob per pair).  Every chain is written once; what differs between the codecs is a handful of per-model hooks that live
next to the model (``models.py``): the hyper-analysis, the entropy parameters, the quantiser of y, and how one view's y is coded.

``models`` imports this module and re-exports its public names; nothing here imports ``models``.
"""
import contextlib

import torch

from . import functional as Fn
from .geometry import warp_perspective


# ---- what the forward passes of ``models`` and the coders both use
def _check_pair(x1, x2, h_matrix):
    """Argument errors up front, with a usable message (the reference fails deep inside with a size mismatch: SURVEY.md 5)."""
    if x1.dim() != 4 or x1.shape != x2.shape or x1.shape[1] != 3:
        raise RuntimeError(f"HSIC.forward: x1 and x2 must be (B, 3, H, W) tensors of one shape, got {tuple(x1.shape)} and {tuple(x2.shape)}")
    B, _, H, W = x1.shape
    if B == 0:
        raise RuntimeError("HSIC.forward: empty batch")
    if H % 64 or W % 64:
        raise RuntimeError(f"HSIC.forward: H and W must be multiples of 64 (the hyper path down-samples by 64), got {H}x{W}; "
                           "zero-pad with hesic_amd.models.pad_to_multiple and crop the reconstructions")
    if h_matrix.shape[-2:] != (3, 3) or h_matrix.dim() != 3 or h_matrix.shape[0] not in (1, B):
        raise RuntimeError(f"HSIC.forward: h_matrix must be (B, 3, 3) (or (1, 3, 3)), got {tuple(h_matrix.shape)}")


def _round_latent(model, y_hi):
    """``_quantize(y, "dequantize")`` without means at inference: an fp32 latent of the bf16 mode is rounded in fp32 and
    stored in the storage dtype (integers: exact) for the convs that read it."""
    cdt = Fn.compute_dtype()
    if y_hi.is_cuda and y_hi.dtype == torch.float32 and cdt != torch.float32:
        return Fn.round_to(y_hi, cdt)
    return model._quantize(y_hi, "dequantize")


# ---- the .bin payload container (this repository's own file: the reference's third-party `range_coder` is absent).
# A payload can only be decoded by a decoder that forms the SAME cumulative-frequency tables, bit for bit: they come out of the
# hyper-synthesis (and, for view 2, the decoder1 -> warp -> encoder1 pass) run in the encoder's storage format.  Since round 4 every payload
# starts with 4 magic bytes + one MODE byte naming what the tables depend on; a decoder in another mode raises instead of desynchronising.
PAYLOAD_MAGIC = b"HSC\x03"               # format 3 (round 5: two mode bytes).  Format 2 (round 4) had one; format 1 (rounds 2-3) no header
TABLE_KERNEL_VERSION = 2                  # bump when hesic_gmm_cdf / the table-producing launches change their arithmetic
_MODE_BYTES = 2


def payload_mode_bytes():
    """Everything the cumulative-frequency tables depend on besides the weights (round 4's single byte left out the warp convention
    and the summation-order switches, so a decoder differing in one of them passed the check and desynchronised on view 2).
    byte 0 -- bits 0-1: storage format of the maps (0 fp32, 1 bfloat16, 2 float16); bit 2: error-feedback weight rounding on the
    single-operand analysis launches (the third analysis pass feeds view 2's tables); bit 3: fp32 latents; bits 4-7: table-kernel version.
    byte 1 -- bit 0: warp convention (``geometry.DEFAULT_ALIGN_CORNERS``: x1_hat_warp, hence round(encoder1(warp(x1_hat))), hence view 2's
    tables); bit 1: split-K launches allowed (``Fn.SPLIT_K``); bit 2: grouped hyper-synthesis launches (``Fn.GROUP_HYPER``) -- both reorder
    the fp32 sums of the hyper-synthesis; bits 3-4: analysis precision of the third pass' producer chain (0 x3, 1 x3c2, 2 x1, 3 x2: x1_hat is
    decoded from y1_hat alone, but the mode is recorded so that a mismatch is reported rather than argued about)."""
    from . import geometry as _geo
    dt = {torch.float32: 0, torch.bfloat16: 1, torch.float16: 2}[Fn.compute_dtype()]
    b0 = dt | (int(bool(Fn.SHAPED_WEIGHTS) and dt != 0) << 2) | (int(bool(Fn.FP32_LATENTS)) << 3) | (TABLE_KERNEL_VERSION << 4)
    an = 0 if dt == 0 else {"x3": 0, "x3c2": 1, "x1": 2, "x2": 3}[Fn.analysis_precision()]
    b1 = int(bool(_geo.DEFAULT_ALIGN_CORNERS)) | (int(bool(Fn.SPLIT_K)) << 1) | (int(bool(Fn.GROUP_HYPER)) << 2) | (an << 3)
    return bytes([b0, b1])


def payload_mode_byte():
    """Byte 0 of ``payload_mode_bytes()`` (the round-4 name; tests and tools that look at the storage format use it)."""
    return payload_mode_bytes()[0]


def describe_mode_bytes(b):
    b0, b1 = b[0], b[1]
    return (f"{('float32', 'bfloat16', 'float16', '?')[b0 & 3]} maps, error-feedback analysis weights {'on' if b0 & 4 else 'off'}, "
            f"fp32 latents {'on' if b0 & 8 else 'off'}, table kernels v{b0 >> 4}, warp align_corners={'True' if b1 & 1 else 'False'}, "
            f"split-K {'on' if b1 & 2 else 'off'}, grouped hyper-synthesis {'on' if b1 & 4 else 'off'}, analysis {('x3', 'x3c2', 'x1', 'x2')[(b1 >> 3) & 3]}")


def payload_header(extra=b""):
    return PAYLOAD_MAGIC + payload_mode_bytes() + extra


def mode_mismatch_message(mode, here):
    """What a decoder in mode ``here`` says about a payload written in ``mode`` (the .bin payload and the .hsd container)."""
    return (f"decompress: the payload was written with [{describe_mode_bytes(mode)}] but this process decodes with "
            f"[{describe_mode_bytes(here)}]; the cumulative-frequency tables would differ in the last count and the range decoder "
            "would desynchronise.  Select the writer's mode (hesic_amd.set_compute_dtype, set_analysis_precision, "
            "geometry.use_reference_era_warp / HESIC_WARP_ALIGN_CORNERS, HESIC_SHAPED_WEIGHTS, HESIC_BF16_LATENTS, HESIC_NO_GROUP_HYPER)")


def check_payload(payload, n_extra=0):
    """Validate the container header; returns (extra bytes, offset of the range-coder stream)."""
    n = len(PAYLOAD_MAGIC)
    if len(payload) < n + _MODE_BYTES + n_extra or payload[:n] != PAYLOAD_MAGIC:
        raise ValueError("decompress: the .bin payload does not start with this coder's format-3 header (a file written by rounds 2-4 of "
                         "this package, or not one of its payloads): re-encode it -- the header names the mode the tables were formed in")
    mode, here = bytes(payload[n:n + _MODE_BYTES]), payload_mode_bytes()
    if mode != here:
        raise ValueError(mode_mismatch_message(mode, here))
    return payload[n + _MODE_BYTES:n + _MODE_BYTES + n_extra], n + _MODE_BYTES + n_extra


# ---- the z strings
def _decompress_z(bottleneck, strings, size):
    """``EntropyBottleneck.decompress`` for a batch.  The reference's form holds its (1, C, 1, 1) medians against an (N, C, H, W) index
    map and refuses N > 1; here the medians are expanded over the batch and the strings go through ``EntropyModel.decompress`` in one
    call (each string is its own rANS stream, the values are those of N single calls)."""
    if len(strings) == 1:
        return bottleneck.decompress(strings, size)
    from .compressai.entropy_models.entropy_models import EntropyModel
    shape = (len(strings), bottleneck._quantized_cdf.size(0), int(size[0]), int(size[1]))
    medians = bottleneck._medians().detach().view(1, -1, 1, 1).expand(shape[0], -1, -1, -1)
    return EntropyModel.decompress(bottleneck, list(strings), bottleneck._build_indexes(shape), medians)


Z_CODERS = ("host", "device")


def _check_z_coder(who, z_coder):
    if z_coder not in Z_CODERS:
        raise ValueError(f'{who}: z_coder must be "host" or "device", got {z_coder!r}')
    return z_coder == "device"


def _code_z(bottleneck, z, device, cdt):
    """The z side of one view in the analysis chain: -> (strings, z_hat).  Host coder: the strings of ``bottleneck.compress`` and what
    decoding them yields (two synchronising round trips).  Device coder (csrc/rans.hip): the same bytes stay on the device as a pending
    (data, counts, status) triple for ``_read_z_strings``, z_hat comes from the symbols that were coded, and nothing synchronises."""
    if not device:
        strings = bottleneck.compress(z)
        return strings, _decompress_z(bottleneck, strings, z.size()[-2:]).to(cdt)
    data, counts, status, z_hat = bottleneck.compress_device(z, cdt, launch_only=True)
    return (data, counts, status), z_hat


def _read_z_strings(who, pending):
    """The pending device z strings of both views -> per view the list of B ``bytes``: one read of the counts and status words, one of
    the bytes of both views."""
    host = torch.cat([t for _d, counts, status in pending for t in (status, counts)]).cpu().tolist()
    blocks, lens, pos = [], [], 0
    for vi, (data, counts, _status) in enumerate(pending):
        B = counts.numel()
        Fn.rans_check_status(f"{who}: z string of view {vi + 1}", host[pos:pos + B])
        lens.append(host[pos + B:pos + 2 * B])
        blocks.append(data[:sum(lens[-1])])
        pos += 2 * B
    raw = torch.cat(blocks).cpu().numpy().tobytes()
    out, pos = [], 0
    for ls in lens:
        strings = []
        for n in ls:
            strings.append(raw[pos:pos + n])
            pos += n
        out.append(strings)
    return out


def _decode_z_device(who, bottlenecks, per_view, zs, dev, cdt):
    """The z strings of both views of a batch, uploaded in one copy and decoded on the device: -> (z1_hat, z2_hat, status) with the
    per-stream status words of both launches for ``Fn.rans_check_status`` at the end of the call (no synchronisation here).  The lengths
    are validated on the host first."""
    strings = [list(per_view[vi][2]) for vi in range(2)]
    for vi in range(2):
        for b, s_ in enumerate(strings[vi]):
            if len(s_) < 8 or len(s_) % 4:
                raise ValueError(f"{who}: the z string of pair {b}, view {vi + 1} has {len(s_)} bytes: not whole 32-bit words of a rANS stream")
    buf = torch.frombuffer(bytearray(b"".join(strings[0] + strings[1])), dtype=torch.uint8).to(dev)
    cut = sum(len(s_) for s_ in strings[0])
    outs = [bottlenecks[vi].decompress_device(part, [len(s_) for s_ in strings[vi]], zs, cdt, check=False)
            for vi, part in enumerate((buf[:cut], buf[cut:]))]
    return outs[0][0], outs[1][0], torch.cat([outs[0][1], outs[1][1]])


# ---- the blobs of a batch, the side-information file of one pair
def _batch_blobs(who, kind, blobs, h_matrix, M):
    """The host-side validation of ``decompress_batch`` (both codecs), before anything is launched: every blob parses
    (``bitstream.parse_pair``), is of ``kind``, and they agree on size and channels_per_stream; alphabets and channel lists are what the
    device coder takes.  Returns (B, H, W, cps, per view (minmax, channels, z strings, stream bytes back to back, (B, S) lengths))."""
    from . import bitstream
    blobs = list(blobs)
    if not blobs:
        raise ValueError(f"{who}: no blobs")
    pairs = [bitstream.parse_pair(bl) for bl in blobs]
    for p in pairs:
        bitstream.require_kind(p, kind, who)
    B, p0 = len(pairs), pairs[0]
    H, W, cps = p0["height"], p0["width"], p0["channels_per_stream"]
    for p in pairs:
        if (p["height"], p["width"]) != (H, W):
            raise ValueError(f"{who}: all blobs of one call must have the same size, got {H}x{W} and {p['height']}x{p['width']}; "
                             "decode each size in a call of its own")
        if p["channels_per_stream"] != cps:
            raise ValueError(f"{who}: all blobs of one call must have the same channels_per_stream")
        if p["channels"] != M:
            raise ValueError(f"{who}: the blob codes {p['channels']} latent channels, this model has {M}")
    if H % 64 or W % 64:
        raise ValueError(f"{who}: the header's size {H}x{W} is not a multiple of 64")
    per_view = []
    for vi in range(2):
        vs = [p["views"][vi] for p in pairs]
        minmax = [v["minmax"] for v in vs]
        channels = [[c for c, f in enumerate(v["flags"]) if f] for v in vs]
        Fn.rc_check(minmax, channels, M)                   # alphabets beyond the kernels' limit: refused here
        S = (M + cps - 1) // cps
        counts = [[len(s) for s in v["streams"]] + [0] * (S - len(v["streams"])) for v in vs]
        per_view.append((minmax, channels, [v["z"] for v in vs], b"".join(s for v in vs for s in v["streams"]), counts))
    if h_matrix.dim() != 3 or h_matrix.shape[-2:] != (3, 3) or h_matrix.shape[0] not in (1, B):
        raise ValueError(f"{who}: h_matrix must be ({B}, 3, 3) (or (1, 3, 3)), got {tuple(h_matrix.shape)}")
    if not h_matrix.is_cuda:
        raise RuntimeError(f"{who}: the device range coder needs h_matrix on a ROCm device (no CPU fallback)")
    return B, H, W, cps, per_view


def _nhwc_rows(t):
    """(1, C, H, W) map -> (H * W, C) rows, one per pixel (a view when the map is channels_last)."""
    return t.permute(0, 2, 3, 1).reshape(t.shape[2] * t.shape[3], t.shape[1])


def _header_view(who, y_hat, z_strings):
    """One view's part of the ``.npz`` side-information file (the reference's raw header: uint16 length of the z string, uint16 minmax,
    the packed channel flags, the z string) -> (bytes, minmax, coded channels)."""
    import numpy as np
    yi = y_hat[0].float()
    flag = (yi.abs().sum(dim=(1, 2)) > 0).cpu().numpy().astype(np.uint8)
    minmax = int(max(float(yi.abs().max()), 1.0))
    if len(z_strings[0]) > 65535 or minmax > 32767:
        raise ValueError(f"{who}: z string longer than the uint16 header field or latent range beyond the table kernel's 32767")
    head = np.array([len(z_strings[0]), minmax], dtype=np.uint16).tobytes() + np.packbits(flag).tobytes() + z_strings[0]
    return head, minmax, [int(c) for c in np.nonzero(flag)[0]]


def _parse_side_info(blob, M):
    """The ``.npz`` file of ``compress`` -> ((H, W), per view (minmax, coded channels, z string))."""
    import numpy as np
    H, W = (int(v) for v in np.frombuffer(blob[:4], dtype=np.uint16))
    pos, views = 4, []
    for _ in range(2):
        length, minmax = (int(v) for v in np.frombuffer(blob[pos:pos + 4], dtype=np.uint16))
        pos += 4
        flag = np.unpackbits(np.frombuffer(blob[pos:pos + (M + 7) // 8], dtype=np.uint8))[:M]
        pos += (M + 7) // 8
        views.append((minmax, [int(c) for c in np.nonzero(flag)[0]], blob[pos:pos + length]))
        pos += length
    return (H, W), views


class PairCoder:
    """``compress`` / ``decompress`` / ``compress_batch`` / ``decompress_batch`` of a stereo model with two entropy bottlenecks, ``encoder1/2``,
    ``decoder1/2`` and ``gaussian1``.  The model supplies:

      _CODER            its name in the batched calls' messages, _PAIR_WHO the prefix of ``compress``' messages
      _BLOB_KIND        the ``bitstream`` kind of its blobs
      _ORDERS           the pixel orders of its ``.bin`` payload: name -> order byte (empty: no such byte), with ``_order`` below
      _TIMES_ANALYSIS   whether ``compress``' enctime includes the analysis chain
      _hyper_analysis(which, y_lo) -> z                       view ``which``'s hyper-analysis
      _entropy_params(which, z_hat, y_hat, extra) -> params   the view's entropy parameters, a tuple of maps (``extra``: y1_hat_w for view 2)
      _y_quantiser(which)                                     the entropy model that rounds y (and bounds its scales)
      _encode_y(enc, which, y_hat, params, minmax, channels, order)            one view's y into the host range encoder
      _decode_y(dec, which, z_hat, extra, minmax, channels, yh, yw, order)     ... and back: -> y_hat
      _rc_encode(which, y_hat, params, minmax, channels, cps, order) -> (data, counts)    the device encoder's launches for B images
      _rc_decode(which, z_hat, extra, view, cps, yh, yw) -> y_hat                         ... and back
    """
    _ORDERS = {}
    _TIMES_ANALYSIS = False

    @contextlib.contextmanager
    def _coding(self):
        """What every coding call runs under (HESIC+ adds to it)."""
        with torch.no_grad():
            yield

    def _order(self):
        """(pixel order, its payload byte) of a ``compress`` call.  A model with several orders takes ``order=...`` here."""
        return None, b""

    def _rc_order(self, yh, yw, dev):
        """The pixel order of the device encoder's streams (None: raster)."""
        return None

    def _ready(self):
        if self.entropy_bottleneck1._offset.numel() == 0:
            self.update()

    # ------------------------------------------------------------------------------------------ the two chains
    def _analysis(self, x1, x2, h_matrix, device_z=False):
        """The encoder's side of the real bit-stream for B pairs, shared by ``compress`` and ``compress_batch`` (their streams must be
        formed from the same numbers): per view (y_hat, z_hat, z strings, entropy parameters).  Call it under ``_coding()``.  y1 is rounded
        BEFORE view 1's parameters are evaluated (HESIC+'s context model reads y1_hat); for HESIC that only moves the hyper-synthesis
        launches behind the rounding kernel on the same stream -- they share no data, so the numbers are the same (the byte tests pin them)."""
        size = (x1.shape[-2], x1.shape[-1])
        cdt = Fn.compute_dtype()
        y1_lo, y1 = self.encoder1.latent(x1, exact=True, lo_abs=self._LO_ABS)
        z1_strings, z1_hat = _code_z(self.entropy_bottleneck1, self._hyper_analysis(1, y1_lo), device_z, cdt)
        y1_hat = _round_latent(self._y_quantiser(1), y1)
        params1 = self._entropy_params(1, z1_hat, y1_hat, None)
        x1_hat = self.decoder1(y1_hat)
        x1_warp = warp_perspective(x1, h_matrix, size)
        y2_lo, y2 = self.encoder2.latent(x1_warp, x2, exact=True, lo_abs=self._LO_ABS)
        z2_strings, z2_hat = _code_z(self.entropy_bottleneck2, self._hyper_analysis(2, y2_lo), device_z, cdt)
        x1_hat_warp = warp_perspective(x1_hat, h_matrix, size)
        y1_hat_w = _round_latent(self.gaussian1, self.encoder1.latent(x1_hat_warp, want_lo=False)[1])
        y2_hat = _round_latent(self._y_quantiser(2), y2)
        params2 = self._entropy_params(2, z2_hat, y2_hat, y1_hat_w)
        return (y1_hat, z1_hat, z1_strings, params1), (y2_hat, z2_hat, z2_strings, params2)

    def _z_hats(self, who, per_view, zs, dev, cdt, device_z):
        """The z front end of a decoder: per_view[v][2] holds view v's z strings -> (z1_hat, z2_hat, status).  ``status`` (device coder
        only, else None) is checked by ``_synthesis`` after its last launch."""
        bottlenecks = (self.entropy_bottleneck1, self.entropy_bottleneck2)
        if device_z:
            return _decode_z_device(who, bottlenecks, per_view, zs, dev, cdt)
        return tuple(_decompress_z(bottlenecks[vi], per_view[vi][2], zs).to(dev, cdt) for vi in range(2)) + (None,)

    def _synthesis(self, who, z_hats, h_matrix, size, decode_view):
        """The decoder's chain: ``decode_view(which, z_hat, extra) -> y_hat`` decodes view 1, then (given round(encoder1(warp(x1_hat))))
        view 2."""
        z1_hat, z2_hat, z_status = z_hats
        y1_hat = decode_view(1, z1_hat, None)
        x1_hat = self.decoder1(y1_hat)
        x1_hat_warp = warp_perspective(x1_hat, h_matrix, size)
        y1_hat_w = _round_latent(self.gaussian1, self.encoder1.latent(x1_hat_warp, want_lo=False)[1])
        y2_hat = decode_view(2, z2_hat, y1_hat_w)
        x2_hat = self.decoder2(y2_hat, x1_hat_warp)
        if z_status is not None:
            Fn.rans_check_status(f"{who}: z string", z_status.cpu())
        return {"x1_hat": x1_hat, "x2_hat": x2_hat, "y1_hat": y1_hat, "y2_hat": y2_hat, "z1_hat": z1_hat, "z2_hat": z2_hat}

    # ------------------------------------------------------------------------------------------ one pair, host range coder
    # compress / decompress of the reference.  Same flow and the same header file (the reference's name for its raw side-information file is
    # ``.npz``); the per-pixel Python loops of the reference are table launches + passes of the host range coder.  The .bin payload is coded
    # by libhesic_host's own carry-less range coder: the reference's `range_coder` package is third party, absent and unpinned, so
    # byte-compatibility of that file is not claimed (round trips are exact).  Batch size 1, like the reference.
    def compress(self, x1, x2, h_matrix, output_name, output_path="", device=None, **order):
        """``order="wavefront"`` (HESIC+ only, by keyword): the sequence in which the pixels' symbols enter the range coder.  "raster" is the reference's (rows,
        then columns; newnet1_joint.py:903-1040) and forces a decoder to walk the map pixel by pixel; "wavefront" (default) codes the
        pixels group by group of ``_wavefronts`` so the decoder evaluates every group in one batch.  Same symbols, same tables; the
        first payload byte says which (the payload is this repository's own range coder either way)."""
        import os
        import time
        import numpy as np
        from ._host import RangeEncoder
        who = self._PAIR_WHO
        if x1.shape[0] != 1:
            raise ValueError(f"{who} codes one stereo pair per call (batch size 1, as the reference)")
        order, extra = self._order(**order)
        self._ready()
        start = time.time()
        with self._coding():
            v1, v2 = self._analysis(x1, x2, h_matrix)
            if not self._TIMES_ANALYSIS:
                start = time.time()
            head = bytearray(np.array(x1.shape[2:], dtype=np.uint16).tobytes())
            enc = RangeEncoder()
            for which, (y_hat, _z_hat, z_strings, params) in ((1, v1), (2, v2)):
                hv, minmax, channels = _header_view(who, y_hat, z_strings)
                head += hv
                self._encode_y(enc, which, y_hat, params, minmax, channels, order)
        payload = payload_header(extra) + enc.finish()
        with open(os.path.join(output_path, str(output_name) + ".npz"), "wb") as f:
            f.write(bytes(head))
        with open(os.path.join(output_path, str(output_name) + ".bin"), "wb") as f:
            f.write(payload)
        num_pixels = x1.shape[2] * x1.shape[3] * 2
        return {"bpp_real": (len(head) + len(payload)) * 8 / num_pixels, "bpp_side": len(head) * 8 / num_pixels,
                "enctime": time.time() - start, "y1_hat": v1[0], "y2_hat": v2[0], "z1_hat": v1[1], "z2_hat": v2[1]}

    def decompress(self, x1, x2, h_matrix, output_name, output_path="", device=None):
        """x1 / x2 are unused (the reference only reads their size, which the header carries); kept for its signature."""
        import os
        import time
        from ._host import RangeDecoder
        self._ready()
        dev, cdt = h_matrix.device, Fn.compute_dtype()
        with open(os.path.join(output_path, str(output_name) + ".npz"), "rb") as f:
            size, views = _parse_side_info(f.read(), self.M)
        with open(os.path.join(output_path, str(output_name) + ".bin"), "rb") as f:
            payload = f.read()
        extra, off = check_payload(payload, 1 if self._ORDERS else 0)
        order = {byte: name for name, byte in self._ORDERS.items()}.get(extra[0]) if extra else None
        if extra and order is None:
            raise ValueError("decompress: not a HESIC+ payload of this coder (unknown pixel-order byte)")
        dec = RangeDecoder(payload[off:])
        yh, yw = size[0] // 16, size[1] // 16
        start = time.time()

        def decode_view(which, z_hat, extra):
            minmax, channels, _z = views[which - 1]
            return self._decode_y(dec, which, z_hat, extra, minmax, channels, yh, yw, order)

        with self._coding():
            z_hats = self._z_hats("decompress", [(None, None, [v[2]]) for v in views], (yh // 4, yw // 4), dev, cdt, False)
            out = self._synthesis("decompress", z_hats, h_matrix, size, decode_view)
        out["dectime"] = time.time() - start
        return out

    # ------------------------------------------------------------------------------- batched bit-stream, coded on the device
    # The same flow for a whole batch, with the range coder on the GPU (csrc/codec.hip): per view one launch for the coding intervals of
    # every latent of every image, one for the streams (one per ``channels_per_stream`` coded channels), one to compact them -- no table
    # and no symbol of y leaves the device.  One self-contained blob per pair (hesic_amd/bitstream.py).  The z strings are coded by the host
    # rANS coder (``z_coder="host"``, the default: z is quantised, copied to the host, coded one image at a time and decoded again for
    # z_hat -- two synchronising round trips inside the analysis chain) or by the device rANS coder (``z_coder="device"``, csrc/rans.hip:
    # the same bytes, no round trip; the z bytes are read back after the y streams).  Pairs are independent: blob i does not depend on what
    # else is in the batch.
    def compress_batch(self, x1, x2, h_matrix, channels_per_stream=1, z_coder="host"):
        """(B, 3, H, W) pairs -> dict(blobs: one ``bytes`` per pair (``bitstream.pack_pair``, of the model's kind), bpp_real: one figure per
        pair over its 2 H W pixels, y1_hat, y2_hat, z1_hat, z2_hat).  ``channels_per_stream``: coded channels per range-coder stream -- 1
        gives the shortest serial chains (fastest), larger values fewer stream terminations and lengths (smaller blobs).  An image whose
        latents need an alphabet beyond the device coder's 1024 symbols raises ``ValueError``: code that pair with ``compress``.
        ``z_coder``: "host" or "device", who codes the z strings -- the blobs are the same bytes either way."""
        from . import bitstream
        who = self._CODER + ".compress_batch"
        _check_pair(x1, x2, h_matrix)
        device_z = _check_z_coder(who, z_coder)
        if not x1.is_cuda:
            raise RuntimeError(f"{who}: the device range coder needs tensors on a ROCm device (no CPU fallback)")
        cps = int(channels_per_stream)
        if not 1 <= cps <= min(self.M, 255):
            raise ValueError(f"{who}: channels_per_stream must be in [1, {min(self.M, 255)}], got {channels_per_stream}")
        self._ready()
        B, _, H, W = x1.shape
        with self._coding():
            v1, v2 = self._analysis(x1, x2, h_matrix, device_z)
            order = self._rc_order(H // 16, W // 16, x1.device)
            # one small device -> host read: per image, view and channel max |y_hat| (minmax and the flags follow from it)
            peak = torch.stack([v[0].float().abs().amax(dim=(2, 3)) for v in (v1, v2)]).cpu()
            views = [[None, None] for _ in range(B)]
            for vi, (y_hat, _z_hat, z_strings, params) in enumerate((v1, v2)):
                flags = (peak[vi] > 0).tolist()
                minmax = [int(max(float(peak[vi, b].max()), 1.0)) for b in range(B)]
                channels = [[c for c, f in enumerate(flags[b]) if f] for b in range(B)]
                data, counts = self._rc_encode(vi + 1, y_hat, params, minmax, channels, cps, order)
                data, counts = data.cpu().numpy().tobytes(), counts.cpu().tolist()
                pos = 0
                for b in range(B):
                    streams = []
                    for n in counts[b][:bitstream.n_streams(flags[b], cps)]:
                        streams.append(data[pos:pos + n])
                        pos += n
                    views[b][vi] = {"minmax": minmax[b], "flags": tuple(int(f) for f in flags[b]), "z": None if device_z else z_strings[b],
                                    "streams": streams}
            if device_z:
                for vi, strings in enumerate(_read_z_strings(who, (v1[2], v2[2]))):
                    for b in range(B):
                        views[b][vi]["z"] = strings[b]
        kind = {} if self._BLOB_KIND == "hesic" else {"kind": self._BLOB_KIND}          # a HESIC blob's dict carries no kind
        blobs = [bitstream.pack_pair({**kind, "mode": payload_mode_bytes(), "height": H, "width": W, "channels": self.M,
                                      "channels_per_stream": cps, "views": views[b]}) for b in range(B)]
        return {"blobs": blobs, "bpp_real": [len(bl) * 8 / (H * W * 2) for bl in blobs],
                "y1_hat": v1[0], "y2_hat": v2[0], "z1_hat": v1[1], "z2_hat": v2[1]}

    def decompress_batch(self, blobs, h_matrix, z_coder="host"):
        """``blobs``: what ``compress_batch`` returned, in any grouping and order (all of one image size and channels_per_stream);
        ``h_matrix`` (B, 3, 3) the matching homographies.  Everything is validated on the host before the first launch.  ``z_coder``: "host"
        decodes the 2 B z strings on the host before the first launch, "device" uploads them in one copy and decodes them there; either
        reads the blobs of either encoder setting."""
        who = self._CODER + ".decompress_batch"
        device_z = _check_z_coder(who, z_coder)
        B, H, W, cps, per_view = _batch_blobs(who, self._BLOB_KIND, blobs, h_matrix, self.M)
        self._ready()
        dev, cdt = h_matrix.device, Fn.compute_dtype()
        yh, yw = H // 16, W // 16

        def decode_view(which, z_hat, extra):
            return self._rc_decode(which, z_hat, extra, per_view[which - 1], cps, yh, yw)

        with self._coding():
            z_hats = self._z_hats(who, per_view, (yh // 4, yw // 4), dev, cdt, device_z)
            return self._synthesis(who, z_hats, h_matrix, (H, W), decode_view)

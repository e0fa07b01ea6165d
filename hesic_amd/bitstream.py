"""The ``.hsd`` container of ``HSIC.compress_batch`` / ``decompress_batch`` (HESIC) and of ``HSICJoint.compress_batch`` /
``decompress_batch`` (HESIC+): one self-contained blob per stereo pair.

Pure Python (no GPU, no kernels): ``pack_pair`` and ``parse_pair`` are inverses, and ``parse_pair`` validates everything a decoder
relies on -- magic, the mode bytes the cumulative-frequency tables depend on, every length, the CRC -- before anything is launched.

Layout (little endian; ``varint`` = unsigned LEB128)::

    b"HSD\\x01" | b"HSJ\\x01"       magic + format version: the KIND of the blob -- "hesic" (HSD) or "joint" (HSJ, HESIC+)
    mode        2 bytes            pair_coder.payload_mode_bytes() of the writer (as in the .bin payload of HSIC.compress)
    H, W        2 x uint16         image size (multiples of 64)
    M           uint16             latent channels
    cps         uint8              channels_per_stream
    per view (1, 2):
        minmax      uint16         the alphabet is 2 * minmax + 1
        flags       ceil(M / 8)    bit set = channel coded (numpy.packbits order: channel 0 is the top bit of byte 0)
        len(z)      varint
        z           bytes          the hyper-latents' rANS string
        stream lengths             ceil(n_flagged / cps) varints
    stream bytes                   view 1's streams, then view 2's, back to back
    crc32       uint32             zlib.crc32 of everything before it

Stream s of a view carries the coded channels [s * cps, (s + 1) * cps) of that view's flagged channels (ascending), symbols
channel-major, then rows, then columns; see DESIGN.md 7 for the coder.

The two kinds share every field; they differ in the magic and in the order of the symbols inside a stream.  A "joint" blob's streams
walk the latent map in wavefront groups (t = w + 3 h ascending, raster order inside a group), pixel-major: for each pixel the
stream's channels in ascending order (include/hesic_codec.h).  ``pack_pair`` writes the kind named by ``pair["kind"]`` (absent:
"hesic"); ``parse_pair`` takes either magic and returns ``"kind": "joint"`` for a HESIC+ blob -- a parsed HESIC blob is the dict it
always was, without the key; ``kind_of`` reads both.  A decoder checks the kind before anything is launched (``require_kind``).
"""
from __future__ import annotations

import struct
import zlib

MAGIC = b"HSD\x01"
MAGIC_JOINT = b"HSJ\x01"
KINDS = {"hesic": MAGIC, "joint": MAGIC_JOINT}
_MAX_VARINT_BYTES = 5            # lengths below 2^35: far beyond any stream
_ONE_BYTE = [bytes((i,)) for i in range(0x80)]


def _varint(n):
    n = int(n)
    if 0 <= n < 0x80:
        return _ONE_BYTE[n]
    if n < 0 or n >= 1 << (7 * _MAX_VARINT_BYTES):
        raise ValueError(f"bitstream: length {n} does not fit the container's varint")
    out = bytearray()
    while True:
        b = n & 0x7F
        n >>= 7
        if n:
            out.append(b | 0x80)
        else:
            out.append(b)
            return bytes(out)


class _Reader:
    def __init__(self, data, end):
        self.data, self.pos, self.end = data, 0, end

    def take(self, n, what):
        if n < 0 or self.pos + n > self.end:
            raise ValueError(f"bitstream: truncated blob ({what} needs {n} bytes at offset {self.pos}, {self.end - self.pos} left)")
        v = self.data[self.pos:self.pos + n]
        self.pos += n
        return v

    def varint(self, what):
        data, pos, v = self.data, self.pos, 0          # a blob holds a length per stream: no slices, no calls per byte
        for shift in range(0, 7 * _MAX_VARINT_BYTES, 7):
            if pos >= self.end:
                raise ValueError(f"bitstream: truncated blob ({what} needs 1 bytes at offset {pos}, 0 left)")
            b = data[pos]
            pos += 1
            v |= (b & 0x7F) << shift
            if b < 0x80:
                self.pos = pos
                return v
        raise ValueError(f"bitstream: malformed length ({what}) at offset {pos}")


def _current_mode():
    from . import pair_coder
    return pair_coder.payload_mode_bytes()


def n_streams(flags, channels_per_stream):
    n = sum(1 for f in flags if f)
    return (n + channels_per_stream - 1) // channels_per_stream


def kind_of(pair):
    """"hesic" or "joint": the kind of a parsed pair (or of a dict about to be packed)."""
    return pair.get("kind") or "hesic"


def require_kind(pair, kind, who):
    """The check a decoder makes before anything is launched: ``ValueError`` naming both kinds."""
    got = kind_of(pair)
    if got != kind:
        names = {"hesic": "HESIC (HSIC, magic b'HSD\\x01')", "joint": "HESIC+ (HSICJoint, magic b'HSJ\\x01')"}
        raise ValueError(f"{who}: this decoder takes {names[kind]} blobs, the blob is a {names[got]} blob; decode it with the other model "
                         "(python -m hesic_amd.codec decode --model " + got + ")")


def pack_pair(pair) -> bytes:
    """``pair``: dict(mode: 2 bytes | None = this process' mode, height, width, channels, channels_per_stream, views: two dicts(minmax,
    flags: ``channels`` 0/1 values, z: bytes, streams: list of bytes, one per stream)[, kind: "hesic" (default) | "joint"]) -> the blob."""
    kind = kind_of(pair)
    if kind not in KINDS:
        raise ValueError(f"bitstream: unknown kind {kind!r} (\"hesic\" or \"joint\")")
    mode = bytes(pair["mode"]) if pair.get("mode") is not None else _current_mode()
    H, W, M, cps = int(pair["height"]), int(pair["width"]), int(pair["channels"]), int(pair["channels_per_stream"])
    if len(mode) != 2:
        raise ValueError("bitstream: the mode is two bytes")
    if not (0 < H < 65536 and 0 < W < 65536 and 0 < M < 65536 and 1 <= cps <= min(M, 255)):
        raise ValueError(f"bitstream: size {H}x{W}, {M} channels, {cps} channels per stream do not fit the header")
    if len(pair["views"]) != 2:
        raise ValueError("bitstream: a pair has two views")
    head = bytearray(KINDS[kind] + mode + struct.pack("<HHHB", H, W, M, cps))
    body = bytearray()
    for v in pair["views"]:
        minmax, flags, z, streams = int(v["minmax"]), [1 if f else 0 for f in v["flags"]], bytes(v["z"]), [bytes(s) for s in v["streams"]]
        if not 1 <= minmax < 65536 or len(flags) != M:
            raise ValueError(f"bitstream: minmax {minmax} / {len(flags)} flags for {M} channels")
        if len(streams) != n_streams(flags, cps):
            raise ValueError(f"bitstream: {len(streams)} streams for {sum(flags)} coded channels at {cps} per stream")
        bits = bytearray((M + 7) // 8)
        for c, f in enumerate(flags):
            if f:
                bits[c >> 3] |= 0x80 >> (c & 7)
        head += struct.pack("<H", minmax) + bits + _varint(len(z)) + z
        for s in streams:
            head += _varint(len(s))
            body += s
    blob = bytes(head) + bytes(body)
    return blob + struct.pack("<I", zlib.crc32(blob) & 0xFFFFFFFF)


def parse_pair(blob, mode=None):
    """Inverse of ``pack_pair``.  ``mode``: the two mode bytes the decoder runs in (default: this process').  Raises ``ValueError`` on a
    wrong magic, a mode mismatch (the text of ``pair_coder.check_payload``), a truncated blob, lengths that do not add up and a CRC mismatch."""
    blob = bytes(blob)
    if len(blob) < len(MAGIC) or blob[:len(MAGIC)] not in (MAGIC, MAGIC_JOINT):
        raise ValueError("bitstream: not an .hsd blob of this package (bad magic; format 1 starts with b'HSD\\x01', HESIC+ blobs with "
                         "b'HSJ\\x01')")
    joint = blob[:len(MAGIC)] == MAGIC_JOINT
    r = _Reader(blob, len(blob) - 4 if len(blob) >= len(MAGIC) + 4 else len(blob))
    r.take(len(MAGIC), "magic")
    got = bytes(r.take(2, "mode bytes"))
    here = bytes(mode) if mode is not None else _current_mode()
    if got != here:
        from . import pair_coder
        raise ValueError(pair_coder.mode_mismatch_message(got, here))
    H, W, M, cps = struct.unpack("<HHHB", r.take(7, "size header"))
    if H == 0 or W == 0 or M == 0 or cps == 0 or cps > M:
        raise ValueError(f"bitstream: header fields out of range ({H}x{W}, {M} channels, {cps} per stream)")
    views, lengths = [], []
    for i in range(2):
        minmax, = struct.unpack("<H", r.take(2, f"view {i + 1} minmax"))
        if minmax < 1:
            raise ValueError(f"bitstream: view {i + 1} has minmax 0")
        bits = r.take((M + 7) // 8, f"view {i + 1} flags")
        flags = tuple((bits[c >> 3] >> (7 - (c & 7))) & 1 for c in range(M))
        if M & 7 and bits[-1] & (0xFF >> (M & 7)):
            raise ValueError(f"bitstream: view {i + 1} flags channels beyond {M}")
        z = bytes(r.take(r.varint(f"view {i + 1} z length"), f"view {i + 1} z string"))
        lens = [r.varint(f"view {i + 1} stream length") for _ in range(n_streams(flags, cps))]
        views.append({"minmax": minmax, "flags": flags, "z": z})
        lengths.append(lens)
    left = r.end - r.pos
    want = sum(sum(l) for l in lengths)
    if len(blob) - r.pos < 4 or left != want:
        raise ValueError(f"bitstream: lengths do not add up (the streams claim {want} bytes, the blob holds {max(left, 0)}): truncated or damaged")
    for v, lens in zip(views, lengths):
        v["streams"] = [bytes(r.take(n, "stream")) for n in lens]
    crc, = struct.unpack("<I", blob[-4:])
    if crc != zlib.crc32(blob[:-4]) & 0xFFFFFFFF:
        raise ValueError("bitstream: CRC mismatch -- the blob is damaged")
    pair = {"mode": got, "height": H, "width": W, "channels": M, "channels_per_stream": cps, "views": views}
    if joint:
        pair["kind"] = "joint"
    return pair

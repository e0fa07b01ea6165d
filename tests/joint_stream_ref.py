"""The HESIC+ stream of the device range coder (include/hesic_codec.h, "HESIC+ streams") restated with NumPy / Python on top of
``codec_stream_ref``: the coded channels cut into streams of ``cps`` channels, the pixels walked group by group of equal t = w + 3 h
(raster index ascending inside a group), pixel-major -- for each pixel the stream's channels in ascending order.  A helper module of the
tests, not a test."""
import numpy as np

import codec_stream_ref as R


def wavefront_groups(H, W):
    """Raster indices h * W + w grouped by t = w + 3 h ascending, ascending inside a group (written out, not taken from the package)."""
    groups = {}
    for h in range(H):
        for w in range(W):
            groups.setdefault(w + 3 * h, []).append(h * W + w)
    return [np.array(sorted(groups[t]), dtype=np.int64) for t in sorted(groups)]


def pixel_order(H, W):
    return np.concatenate(wavefront_groups(H, W))


def stream_elements(H, W, n_coded, cps):
    """Per stream s the (listed-channel index j, raster pixel) of its symbols in coding order: int arrays (n, 2)."""
    order = pixel_order(H, W)
    out = []
    for j0 in range(0, n_coded, cps):
        js = np.arange(j0, min(j0 + cps, n_coded))
        out.append(np.stack([np.tile(js, len(order)), np.repeat(order, len(js))], 1))
    return out


def encode_streams(sym, tab, H, W, cps):
    """``sym`` (C, H W) symbols and ``tab`` (C, H W, A + 1) table rows of the C coded channels -> [(body, flush)] per stream."""
    return [R.encode_stream(sym[e[:, 0], e[:, 1]], tab[e[:, 0], e[:, 1]]) for e in stream_elements(H, W, sym.shape[0], cps)]


def decode_streams(streams, tab, H, W, cps):
    """Inverse of ``encode_streams`` (bytes per stream; zeros are read past the end of each) -> (C, H W) symbols."""
    C = tab.shape[0]
    sym = np.zeros((C, H * W), dtype=np.int32)
    for data, e in zip(streams, stream_elements(H, W, C, cps)):
        sym[e[:, 0], e[:, 1]] = R.decode_stream(data, tab[e[:, 0], e[:, 1]])
    return sym


def container_pair(M=192, cps=8, seed=0, kind=None, mode=bytes([0x2A, 0x07])):
    """A random but deterministic pair dict for ``bitstream.pack_pair`` (the generator of tests/test_device_codec_cpu.py)."""
    r = np.random.Generator(np.random.PCG64(seed))
    views = []
    for v in range(2):
        flags = tuple(int(f) for f in (r.random(M) < 0.6))
        n = (sum(flags) + cps - 1) // cps
        streams = [bytes(r.integers(0, 256, int(r.integers(0, 300)), dtype=np.uint8)) for _ in range(n)]
        if n > 2:
            streams[1] = b""
        views.append({"minmax": int(r.integers(1, 512)), "flags": flags, "z": bytes(r.integers(0, 256, 37 + v, dtype=np.uint8)), "streams": streams})
    pair = {"mode": mode, "height": 256, "width": 320, "channels": M, "channels_per_stream": cps, "views": views}
    if kind is not None:
        pair["kind"] = kind
    return pair

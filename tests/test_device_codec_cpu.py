"""Device range coder, the parts that need no GPU: the stream definition (short flush) against the trusted host coder, the ``.hsd``
container, the C ABI of include/hesic_codec.h."""
import os
import struct
import subprocess
import zlib

import numpy as np
import pytest
import torch

import codec_stream_ref as R
from hesic_amd import _host, bitstream


def _check_against_host(sym, cdf):
    """The issue's claim: body == host bytes minus the 8 flush bytes; the short-flushed stream decodes with the host decoder."""
    enc = _host.RangeEncoder()
    enc.encode(sym, cdf)
    host = enc.finish()
    body, flush = R.encode_stream(sym, cdf)
    assert body == host[:-8]
    assert len(flush) <= 2
    data = body + flush
    assert np.array_equal(_host.RangeDecoder(data).decode(cdf), sym)
    return len(data)


def test_short_flush_streams_equal_the_host_coder_on_model_tables():
    """Tables of the recorded reference compress run's model (tests/golden/codec_model_64.npz: same weights and input), formed by the
    oracle: one stream per coded channel of view 1, and one over eight channels."""
    from oracle import hesic_oracle as O
    from test_codec_stream import _ref_compress_case
    g, _P, out = _ref_compress_case()
    y = out["y1_hat"][0].numpy().astype(np.int64)
    minmax = int(max(np.abs(y).max(), 1))
    assert minmax == int(g["minmax"][0])
    channels = [c for c in range(192) if np.abs(y[c]).sum() > 0]
    s_, m_, w_ = out["gmm1"]
    tables = O.compress_cdf_tables(s_, m_, w_, channels, minmax, 5, 192)          # (C, H, W, A + 1)
    hw = tables.shape[1] * tables.shape[2]
    sym = (y[channels] + minmax).reshape(len(channels), hw).astype(np.int32)
    tab = tables.reshape(len(channels), hw, -1)
    for j in range(0, len(channels), 7):
        _check_against_host(sym[j], tab[j])
    _check_against_host(sym[:8].reshape(-1), tab[:8].reshape(8 * hw, -1))
    # the pure-Python decoder agrees too (it is the arithmetic the device decoder restates)
    assert np.array_equal(R.decode_stream(R.encode_bytes(sym[0], tab[0]), tab[0]), sym[0])


@pytest.mark.parametrize("A", [3, 21, 141, 1023])
def test_short_flush_streams_equal_the_host_coder_on_random_tables(A):
    worst = 0.0
    for seed in range(12):
        n = 1 + (seed * 97) % 400
        sym, cdf = R.random_tables(n, A, 100 * A + seed, least_likely=seed % 3 == 0)
        worst = max(worst, _check_against_host(sym, cdf) / n)
    assert worst <= 4.0 + 16.0          # the slot of 4 bytes per symbol + 16 is never the limit (2^-16 floor: 2 bytes per symbol + flush)
    sym, cdf = R.random_tables(50, A, 7)
    assert np.array_equal(R.decode_stream(R.encode_bytes(sym, cdf), cdf), sym)
    # host-coded streams (8-byte termination) decode by the same arithmetic
    enc = _host.RangeEncoder()
    enc.encode(sym, cdf)
    assert np.array_equal(R.decode_stream(enc.finish(), cdf), sym)


def test_a_stream_is_at_most_two_bytes_per_symbol_plus_flush():
    """Every frequency is at least 1 of ~2^16: 2 bytes per symbol at worst, far inside the encoder's slot of 4 n + 16."""
    sym, cdf = R.random_tables(1200, 1023, 5, least_likely=True)
    body, flush = R.encode_stream(sym, cdf)
    assert len(body) + len(flush) <= 2 * len(sym) + 16 < 4 * len(sym) + 16


# ------------------------------------------------------------------------------------------------------------ container
_MODE = bytes([0x2A, 0x07])


def _pair(M=192, cps=8, seed=0):
    r = np.random.Generator(np.random.PCG64(seed))
    views = []
    for v in range(2):
        flags = tuple(int(f) for f in (r.random(M) < 0.6))
        n = bitstream.n_streams(flags, cps)
        streams = [bytes(r.integers(0, 256, int(r.integers(0, 300)), dtype=np.uint8)) for _ in range(n)]
        if n > 2:
            streams[1] = b""                    # an empty stream is legal (every symbol certain)
        views.append({"minmax": int(r.integers(1, 512)), "flags": flags, "z": bytes(r.integers(0, 256, 37 + v, dtype=np.uint8)), "streams": streams})
    return {"mode": _MODE, "height": 256, "width": 320, "channels": M, "channels_per_stream": cps, "views": views}


@pytest.mark.parametrize("M,cps", [(192, 1), (192, 8), (21, 5), (8, 8)])
def test_container_round_trip(M, cps):
    pair = _pair(M, cps, seed=M + cps)
    blob = bitstream.pack_pair(pair)
    assert blob[:4] == b"HSD\x01" and blob[4:6] == _MODE
    assert bitstream.parse_pair(blob, mode=_MODE) == pair
    assert struct.unpack("<I", blob[-4:])[0] == zlib.crc32(blob[:-4])


def test_container_default_mode_is_this_process_mode():
    from hesic_amd import models
    pair = _pair()
    pair["mode"] = None
    blob = bitstream.pack_pair(pair)
    assert blob[4:6] == models.payload_mode_bytes()
    assert bitstream.parse_pair(blob)["mode"] == models.payload_mode_bytes()


def test_container_errors():
    from hesic_amd import models
    pair = _pair()
    blob = bitstream.pack_pair(pair)
    with pytest.raises(ValueError, match="bad magic"):
        bitstream.parse_pair(b"HSD\x02" + blob[4:], mode=_MODE)
    with pytest.raises(ValueError, match="bad magic"):
        bitstream.parse_pair(b"", mode=_MODE)
    # a mode mismatch reads like the .bin payload's (models.check_payload): both modes are named
    other = bytes([0x29, 0x07])
    with pytest.raises(ValueError) as e:
        bitstream.parse_pair(blob, mode=other)
    assert str(e.value) == models.mode_mismatch_message(_MODE, other)
    assert "float16 maps" in str(e.value) and "bfloat16 maps" in str(e.value) and "desynchronise" in str(e.value)
    # truncation, anywhere
    for cut in (5, 8, 12, 40, len(blob) // 2, len(blob) - 5, len(blob) - 1):
        with pytest.raises(ValueError, match="truncated|do not add up"):
            bitstream.parse_pair(blob[:cut], mode=_MODE)
    with pytest.raises(ValueError, match="do not add up"):
        bitstream.parse_pair(blob[:-4] + b"\x00" + blob[-4:], mode=_MODE)           # a byte too many
    # a stream length that does not add up (with a matching CRC, so the length check itself is what fires)
    p2 = _pair()
    b2 = bytearray(bitstream.pack_pair(p2))
    z_end = 13 + 2 + 24 + 1 + 37             # fixed header, minmax, flags, len(z), z of view 1: the first stream length follows
    assert b2[z_end] == len(p2["views"][0]["streams"][0]) & 0x7F | (0x80 if len(p2["views"][0]["streams"][0]) > 127 else 0)
    b2[z_end] ^= 0x01
    b2[-4:] = struct.pack("<I", zlib.crc32(bytes(b2[:-4])))
    with pytest.raises(ValueError, match="do not add up"):
        bitstream.parse_pair(bytes(b2), mode=_MODE)
    # a flipped payload byte is caught by the CRC
    flipped = bytearray(blob)
    flipped[-10] ^= 0x40
    with pytest.raises(ValueError, match="CRC"):
        bitstream.parse_pair(bytes(flipped), mode=_MODE)
    # pack_pair refuses what the header cannot hold
    bad = _pair()
    bad["views"][0]["streams"] = bad["views"][0]["streams"][:-1]
    with pytest.raises(ValueError, match="streams"):
        bitstream.pack_pair(bad)


# ------------------------------------------------------------------------------------------------------------------ ABI
def _L():
    from hesic_amd import _lib as L
    if not os.path.exists(L.LIB_PATH):
        import __graft_entry__ as ge
        ge.build()
    return L


@pytest.mark.parametrize("fmt", ["bf16", "f16"])
def test_library_exports_every_codec_symbol(fmt):
    L = _L()
    declared = L.declared_symbols("hesic_codec.h")
    assert len(declared) >= 4 and "hesic_gmm_rc_decode" in declared and "hesic_rc_encode_streams" in declared
    path = L.LIB_PATH_F16 if fmt == "f16" else L.LIB_PATH
    L.lib(torch.float16 if fmt == "f16" else torch.bfloat16)
    exported = subprocess.check_output(["nm", "-D", "--defined-only", path], text=True)
    missing = [s for s in declared if f" T {s}\n" not in exported]
    assert not missing, missing
    assert set(declared) == set(L._CODEC_SIGS), set(declared) ^ set(L._CODEC_SIGS)
    assert not set(declared) & set(L.declared_symbols())          # a header of its own: the main header's list is unchanged


def test_codec_entry_points_validate_their_arguments():
    import ctypes as C
    L = _L()
    l = L.lib()
    assert l.hesic_rc_stream_cap(100) == 416
    p = C.c_void_p(16)
    # slots smaller than a stream's worst case are refused on the host
    assert l.hesic_rc_encode_streams(p, p, 1, 192, 64, 8, p, 100, p, p, None) == -1 and b"slots" in l.hesic_last_error()
    assert l.hesic_rc_encode_streams(None, p, 1, 192, 64, 8, p, 4096, p, p, None) == -1
    g = L.GmmDesc(1, 4, 8, 9, L.F32, 0, 72, 0, 0, 0.11, 0.0)          # K = 9 > 8
    assert l.hesic_gmm_rc_ranges(C.byref(g), p, p, p, p, L.F32, p, p, None) == -1
    g = L.GmmDesc(1, 4, 8, 5, L.F32, 0, 40, 0, 0, 0.11, 0.0)
    assert l.hesic_gmm_rc_decode(C.byref(g), p, p, p, p, 9, p, 0, p, p, p, L.F32, None) == -1 and b"channels_per_stream" in l.hesic_last_error()


def test_alphabets_beyond_the_limit_are_refused_on_the_host():
    from hesic_amd import functional as Fn
    Fn.rc_check([511], [[0, 1]], 192)
    with pytest.raises(ValueError, match="1024.*HSIC.compress"):
        Fn.rc_check([3, 512], [[0], [1]], 192)
    with pytest.raises(ValueError, match="ascending"):
        Fn.rc_check([3], [[4, 4]], 192)
    with pytest.raises(ValueError, match="ascending"):
        Fn.rc_check([3], [[192]], 192)

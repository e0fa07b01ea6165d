"""Batched HESIC+ bit-stream (HSICJoint.compress_batch / decompress_batch), the parts that need no GPU: the stream definition against
the trusted host coder, the "joint" kind of the container, the C ABI of the three new entry points of include/hesic_codec.h, the host-side
refusals of ``decompress_batch``."""
import ctypes as C
import hashlib
import os
import struct
import subprocess
import zlib

import numpy as np
import pytest
import torch

import codec_stream_ref as R
import joint_stream_ref as J
from hesic_amd import _host, bitstream

NEW_SYMBOLS = ["hesic_rc_encode_streams_ordered", "hesic_joint_gather_batch", "hesic_gmm_rc_decode_step"]


# ------------------------------------------------------------------------------------------------------------ the stream
def _tables(C_, HW, A, seed):
    sym, cdf = R.random_tables(C_ * HW, A, seed, least_likely=seed % 3 == 0)
    return sym.reshape(C_, HW), cdf.reshape(C_, HW, A + 1)


@pytest.mark.parametrize("A", [3, 21, 141, 1023])
@pytest.mark.parametrize("size", [(8, 12), (16, 20), (4, 4)], ids=["8x12", "16x20", "4x4"])
def test_reference_stream_equals_the_host_coder(A, size):
    H, W = size
    M = 10                                              # cps = 8 cuts it into a stream of 8 channels and a short last one of 2
    sym, tab = _tables(M, H * W, A, 31 * A + H)
    for cps in (1, 8, M):
        streams = J.encode_streams(sym, tab, H, W, cps)
        assert len(streams) == (M + cps - 1) // cps
        assert [len(e) // (H * W) for e in J.stream_elements(H, W, M, cps)] == {1: [1] * 10, 8: [8, 2], 10: [10]}[cps]
        for (body, flush), e in zip(streams, J.stream_elements(H, W, M, cps)):
            sy, tb = sym[e[:, 0], e[:, 1]], np.ascontiguousarray(tab[e[:, 0], e[:, 1]])
            enc = _host.RangeEncoder()
            enc.encode(sy, tb)
            assert body == enc.finish()[:-8] and len(flush) <= 2
            assert np.array_equal(_host.RangeDecoder(body + flush).decode(tb), sy)
        assert np.array_equal(J.decode_streams([b + f for b, f in streams], tab, H, W, cps), sym)


@pytest.mark.parametrize("size", [(8, 12), (16, 20), (4, 4), (32, 32)], ids=["8x12", "16x20", "4x4", "32x32"])
def test_symbol_order_is_the_per_pair_wavefront_order(size):
    """cps = M: the one stream's symbol sequence is what HSICJoint.compress(order="wavefront") feeds its encoder -- the pixels of
    ``_wavefronts`` concatenated, per pixel the listed channels ascending (models.py: ``y_rows[pix][:, ch_t].reshape(-1)``)."""
    from hesic_amd.models import HSICJoint
    H, W = size
    groups = HSICJoint._wavefronts(H, W)
    mine = J.wavefront_groups(H, W)
    assert len(groups) == len(mine) == W + 3 * (H - 1) and all(np.array_equal(a, b) for a, b in zip(groups, mine))
    Cn = 7
    y_rows = np.arange(H * W * Cn).reshape(H * W, Cn)                     # element id = pixel * Cn + listed channel
    fed = y_rows[np.concatenate(groups)][:, np.arange(Cn)].reshape(-1)
    e, = J.stream_elements(H, W, Cn, Cn)
    assert np.array_equal(e[:, 1] * Cn + e[:, 0], fed)
    # every pixel of a group depends on earlier groups only: its mask-'A' context has a smaller t
    t = lambda p: p % W + 3 * (p // W)
    for g in mine:
        assert len({t(int(p)) for p in g}) == 1


def test_truncated_stream_decodes_to_the_end():
    """Loop counts come from the header: half the bytes decode to H W symbols inside the alphabet (zeros are read past the end)."""
    H, W, M, A = 8, 12, 4, 21
    sym, tab = _tables(M, H * W, A, 9)
    streams = [b + f for b, f in J.encode_streams(sym, tab, H, W, 2)]
    cut = [s[:len(s) // 2] for s in streams]
    out = J.decode_streams(cut, tab, H, W, 2)
    assert out.shape == sym.shape and int(out.min()) >= 0 and int(out.max()) < A
    assert not np.array_equal(out, sym)
    assert np.array_equal(J.decode_streams(streams, tab, H, W, 2), sym)


# ------------------------------------------------------------------------------------------------------------ container
_MODE = bytes([0x2A, 0x07])


@pytest.mark.parametrize("M,cps", [(192, 1), (192, 8), (21, 5), (8, 8)])
def test_container_round_trip_of_both_kinds(M, cps):
    hesic = J.container_pair(M, cps, seed=M + cps)
    joint = J.container_pair(M, cps, seed=M + cps, kind="joint")
    bh, bj = bitstream.pack_pair(hesic), bitstream.pack_pair(joint)
    assert bh[:4] == b"HSD\x01" and bj[:4] == b"HSJ\x01" and bh[4:-4] == bj[4:-4]          # same fields
    assert bitstream.pack_pair(dict(hesic, kind="hesic")) == bh
    ph, pj = bitstream.parse_pair(bh, mode=_MODE), bitstream.parse_pair(bj, mode=_MODE)
    assert ph == hesic and "kind" not in ph and bitstream.kind_of(ph) == "hesic"
    assert pj == joint and pj["kind"] == "joint" and bitstream.kind_of(pj) == "joint"
    assert struct.unpack("<I", bj[-4:])[0] == zlib.crc32(bj[:-4])


def test_hesic_blobs_are_byte_for_byte_what_they_were():
    """SHA-256 of one blob packed with an explicit mode, computed with the bitstream module of the commit before the "joint" kind."""
    blob = bitstream.pack_pair(J.container_pair(192, 8, seed=5))
    assert len(blob) == 4832
    assert hashlib.sha256(blob).hexdigest() == "d00f1666e039d4303bff14e2740dc011a1f0157f800bb77efd9669dd18808fe3"


def test_container_errors_of_the_joint_kind():
    from hesic_amd import models
    blob = bitstream.pack_pair(J.container_pair(kind="joint"))
    with pytest.raises(ValueError, match="bad magic"):
        bitstream.parse_pair(b"HSJ\x02" + blob[4:], mode=_MODE)
    with pytest.raises(ValueError, match="unknown kind"):
        bitstream.pack_pair(J.container_pair(kind="both"))
    other = bytes([0x29, 0x07])
    with pytest.raises(ValueError) as e:
        bitstream.parse_pair(blob, mode=other)
    assert str(e.value) == models.mode_mismatch_message(_MODE, other)
    for cut in (5, 8, 12, 40, len(blob) // 2, len(blob) - 5, len(blob) - 1):
        with pytest.raises(ValueError, match="truncated|do not add up"):
            bitstream.parse_pair(blob[:cut], mode=_MODE)
    flipped = bytearray(blob)
    flipped[-10] ^= 0x40
    with pytest.raises(ValueError, match="CRC"):
        bitstream.parse_pair(bytes(flipped), mode=_MODE)
    # the kind is part of what the CRC covers: a blob relabelled as the other kind is refused
    with pytest.raises(ValueError, match="CRC"):
        bitstream.parse_pair(b"HSD\x01" + blob[4:], mode=_MODE)
    # the kind mismatch names both kinds
    for kind, pair in (("hesic", bitstream.parse_pair(blob, mode=_MODE)), ("joint", J.container_pair())):
        with pytest.raises(ValueError, match=r"HSD.*HSJ|HSJ.*HSD") as e:
            bitstream.require_kind(pair, kind, "X.decompress_batch")
        assert "HESIC+ (HSICJoint" in str(e.value) and "HESIC (HSIC," in str(e.value)
    bitstream.require_kind(J.container_pair(kind="joint"), "joint", "X")


# ------------------------------------------------------------------------------------------------------------------ ABI
def _L():
    from hesic_amd import _lib as L
    if not os.path.exists(L.LIB_PATH):
        import __graft_entry__ as ge
        ge.build()
    return L


@pytest.mark.parametrize("fmt", ["bf16", "f16"])
def test_both_libraries_export_the_new_symbols(fmt):
    L = _L()
    declared = L.declared_symbols("hesic_codec.h")
    assert all(s in declared for s in NEW_SYMBOLS)
    path = L.LIB_PATH_F16 if fmt == "f16" else L.LIB_PATH
    L.lib(torch.float16 if fmt == "f16" else torch.bfloat16)
    exported = subprocess.check_output(["nm", "-D", "--defined-only", path], text=True)
    assert not [s for s in NEW_SYMBOLS if f" T {s}\n" not in exported]
    assert set(declared) == set(L._CODEC_SIGS)
    assert L.lib().hesic_abi_version() == 3


def test_new_entry_points_validate_their_arguments():
    """HESIC_EINVAL before anything is launched (no GPU is needed to ask)."""
    L = _L()
    l = L.lib()
    p = C.c_void_p(16)
    cap = l.hesic_rc_stream_cap(8 * 64)
    # ordered encoder: null pointers, cps out of range, too-small cap
    ok = [p, p, 1, 192, 64, 8, p, p, cap, p, p, None]
    for i in (0, 1, 6, 7, 9, 10):
        assert l.hesic_rc_encode_streams_ordered(*[None if j == i else a for j, a in enumerate(ok)]) == -1, i
    assert b"null" in l.hesic_last_error()
    assert l.hesic_rc_encode_streams_ordered(p, p, 1, 192, 64, 0, p, p, cap, p, p, None) == -1
    assert l.hesic_rc_encode_streams_ordered(p, p, 1, 192, 64, 193, p, p, cap, p, p, None) == -1 and b"geometry" in l.hesic_last_error()
    assert l.hesic_rc_encode_streams_ordered(p, p, 1, 192, 64, 8, p, p, cap - 1, p, p, None) == -1 and b"slots" in l.hesic_last_error()
    # gather: null pointers, P <= 0, a group outside the map, rows that are not whole 16-byte chunks
    def gather(**kw):
        a = dict(y=p, dt=L.F32, M=192, Wp=12, rows=144, centre=p, raster=p, off=0, P=3, HW=64, B=2, crops=p, par=p, c_par=384, ext=None, e_off=768,
                 feat=p, c_feat=768)
        a.update(kw)
        return l.hesic_joint_gather_batch(a["y"], a["dt"], a["M"], a["Wp"], a["rows"], a["centre"], a["raster"], a["off"], a["P"], a["HW"], a["B"],
                                          a["crops"], a["par"], a["c_par"], a["ext"], a["e_off"], a["feat"], a["c_feat"], None)
    for k in ("y", "centre", "raster", "crops", "par", "feat"):
        assert gather(**{k: None}) == -1, k
    assert gather(P=0) == -1 and gather(P=-1) == -1 and b"P > 0" in l.hesic_last_error()
    assert gather(off=62) == -1 and gather(off=-1) == -1 and gather(B=0) == -1
    assert gather(dt=7) == -1 and gather(M=190) == -1 and gather(c_par=770) == -1 and b"16-byte" in l.hesic_last_error()
    assert gather(ext=p, e_off=768) == -1                      # view 2's rows would not fit behind e_off
    # step decoder: null pointers, cps out of range, P <= 0, K != 1, a group outside the map
    def step(d=None, **kw):
        d = d or L.GmmDesc(2, 3, 192, 1, L.F32, 0, 384, 0, 192, 0.11, 0.0)
        a = dict(sc=p, mu=p, meta=p, cps=8, data=p, n=100, offs=p, cnt=p, state=p, first=1, centre=p, off=0, n_pix=64, y=p, ydt=L.F32, rows=144)
        a.update(kw)
        return l.hesic_gmm_rc_decode_step(C.byref(d), a["sc"], a["mu"], a["meta"], a["cps"], a["data"], a["n"], a["offs"], a["cnt"], a["state"],
                                          a["first"], a["centre"], a["off"], a["n_pix"], a["y"], a["ydt"], a["rows"], None)
    for k in ("sc", "mu", "meta", "data", "offs", "cnt", "state", "centre", "y"):
        assert step(**{k: None}) == -1, k
    assert step(cps=0) == -1 and step(cps=193) == -1 and b"channels_per_stream" in l.hesic_last_error()
    assert step(L.GmmDesc(2, 0, 192, 1, L.F32, 0, 384, 0, 192, 0.11, 0.0)) == -1
    assert step(L.GmmDesc(2, -2, 192, 1, L.F32, 0, 384, 0, 192, 0.11, 0.0)) == -1
    assert step(L.GmmDesc(2, 3, 192, 5, L.F32, 0, 384, 0, 192, 0.11, 0.0)) == -1 and b"K = 1" in l.hesic_last_error()
    assert step(L.GmmDesc(2, 3, 192, 1, L.H16, 0, 384, 0, 192, 0.11, 0.0)) == -1
    assert step(off=62) == -1 and step(off=-1) == -1 and step(rows=0) == -1 and step(n=-1) == -1 and step(ydt=9) == -1


# ----------------------------------------------------------------------------------------------------------- host refusals
def _forged(kind="joint", minmax=9, H=64, W=64, M=192, cps=8):
    flags = (1,) * M
    n = (M + cps - 1) // cps
    view = {"minmax": minmax, "flags": flags, "z": b"\x01\x02\x03", "streams": [b"\x10\x20"] * n}
    pair = {"mode": None, "height": H, "width": W, "channels": M, "channels_per_stream": cps, "views": [dict(view), dict(view)]}
    if kind == "joint":
        pair["kind"] = "joint"
    return bitstream.pack_pair(pair)


def test_decompress_batch_refuses_on_the_host():
    """Alphabet beyond 1024 in a forged header, mixed sizes, the wrong kind, CPU tensors: raised before anything is launched (asserted
    through the call hook), without a device."""
    import hesic_amd
    from hesic_amd import models
    Hm = torch.eye(3).reshape(1, 3, 3)
    launched = []
    with hesic_amd._lib.call_hook(lambda name, args: launched.append(name)):
        joint, hesic = models.HSICJoint(), models.HSIC()
        with pytest.raises(ValueError, match="1024.*compress"):
            joint.decompress_batch([_forged(minmax=600)], Hm)
        with pytest.raises(ValueError, match="same size"):
            joint.decompress_batch([_forged(), _forged(W=128)], Hm.expand(2, 3, 3))
        with pytest.raises(ValueError, match="same channels_per_stream"):
            joint.decompress_batch([_forged(), _forged(cps=1)], Hm.expand(2, 3, 3))
        with pytest.raises(ValueError, match=r"HSICJoint.decompress_batch.*HSJ.*HSD"):
            joint.decompress_batch([_forged(kind="hesic")], Hm)
        with pytest.raises(ValueError, match=r"HSIC.decompress_batch.*HSD.*HSJ"):
            hesic.decompress_batch([_forged()], Hm)
        with pytest.raises(ValueError, match="no blobs"):
            joint.decompress_batch([], Hm)
        with pytest.raises(ValueError, match="h_matrix"):
            joint.decompress_batch([_forged()], torch.eye(3))
        bad = bytearray(_forged())
        bad[-9] ^= 1
        with pytest.raises(ValueError, match="CRC"):
            joint.decompress_batch([bytes(bad)], Hm)
        # no CPU fallback
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            joint.decompress_batch([_forged()], Hm)
        x = torch.zeros(1, 3, 64, 64)
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            joint.compress_batch(x, x, Hm)
    assert launched == [], launched

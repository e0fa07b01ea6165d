"""The numpy restatement of the device rANS coder (tests/rans_device_ref.py) against the host coder, byte for byte, and the slot
bound of 8 n + 16 bytes on every case.  No GPU: this pins the ALGORITHM the kernels of hesic_amd/csrc/rans.hip run (items, backward
fold into a slot filled from its end, exact division through a double reciprocal, lane-count search, zeros past the end, nibble cap);
tests/test_gpu_rans_device.py pins the kernels."""
import numpy as np
import pytest

import rans_device_ref as ref
from hesic_amd import _host

ROWS = (5, 40, 92)
NS = (1, 2, 63, 64, 65, 1000, 8192)


def _case(rows, n, escapes, seed, shuffled=False):
    lengths = [rows, max(3, rows // 2), rows, 3]
    table, sizes, offsets, _med = ref.make_table(lengths, seed)
    C = len(lengths)
    if shuffled or n < C:
        idx = np.random.default_rng(seed + 1).integers(0, C, n).astype(np.int32)
    else:
        idx = np.resize(ref.channel_indexes(C, (n + C - 1) // C), n).astype(np.int32)
        idx.sort()
    sym = ref.make_symbols(n, idx, sizes, offsets, escapes, seed + 2)
    return sym, idx, table, sizes, offsets


@pytest.mark.parametrize("escapes", [0.0, 0.1, 1.0])
@pytest.mark.parametrize("rows,n", [(r, n) for r in ROWS for n in NS if n < 8192 or r == 40])      # the large size for one row length
def test_restatement_matches_host_coder_byte_for_byte(rows, n, escapes):
    sym, idx, table, sizes, offsets = _case(rows, n, escapes, 7 * rows + n)
    want = _host.rans_encode_arrays(sym, idx, table, sizes, offsets)
    slot, count, st = ref.fold(*ref.itemise(sym, idx, table, sizes, offsets))
    assert st == 0
    assert len(want) <= ref.slot_bytes(n) == len(slot)                    # the slot bound
    assert count == len(want) and bytes(slot[len(slot) - count:]) == want
    got, st = ref.decode(want, idx, table, sizes, offsets)
    assert st == 0 and np.array_equal(got, sym)
    assert np.array_equal(_host.rans_decode_arrays(want, idx, table, sizes, offsets), sym)


def test_shuffled_indexes_and_row_of_two_entries():
    """Per-symbol row changes (the explicit index form) and a row that is its escape bin only."""
    sym, idx, table, sizes, offsets = _case(66, 500, 0.1, 11, shuffled=True)
    want = _host.rans_encode_arrays(sym, idx, table, sizes, offsets)
    assert ref.encode(sym, idx, table, sizes, offsets) == (want, 0)
    assert np.array_equal(ref.decode(want, idx, table, sizes, offsets)[0], sym)
    table, sizes, offsets, _ = ref.make_table([2], 3)
    idx = np.zeros(200, np.int32)
    sym = ref.make_symbols(200, idx, sizes, offsets, 1.0, 4)
    want = _host.rans_encode_arrays(sym, idx, table, sizes, offsets)
    assert ref.encode(sym, idx, table, sizes, offsets) == (want, 0)
    assert np.array_equal(ref.decode(want, idx, table, sizes, offsets)[0], sym)


def test_every_nibble_count_occurs_and_worst_case_rate():
    """Escapes of 0 .. 8 data nibbles are all produced by the case generator; with every symbol an escape the stream stays below
    8 bytes per symbol (52 bits at most)."""
    sym, idx, table, sizes, offsets = _case(40, 8192, 1.0, 5)
    _sf, _raw, flag = ref.itemise(sym, idx, table, sizes, offsets)
    assert set(range(2, 10)) <= set(np.unique(flag).tolist())
    want = _host.rans_encode_arrays(sym, idx, table, sizes, offsets)
    assert len(want) <= 6.5 * len(sym) + 8


def test_exact_division_at_the_edges():
    """The double-reciprocal quotient is within one of the true quotient over the encoder's whole range (x < freq << 47 < 2^63).  This
    checks the ARITHMETIC of the claim in IEEE double precision, through the restatement alone: it needs neither the library nor the
    kernels and says nothing about the kernel's ``divmod_exact`` itself, which only the byte-equality tests on the GPU pin."""
    rng = np.random.default_rng(0)
    for f in (1, 2, 3, 255, 256, 257, 32767, 32768, 65535, 65536):
        top = f << 47
        for x in [ref.LOW, top - 1, top - f, top - f - 1, (top // f) * f, (top // f) * f - 1] + [int(v) % top for v in rng.integers(0, 1 << 62, 200)]:
            x = max(x, 1)
            assert ref.divmod_exact(x, f) == divmod(x, f)


def test_slot_too_small_sets_overflow_and_writes_nothing_outside():
    sym, idx, table, sizes, offsets = _case(40, 300, 1.0, 9)
    items = ref.itemise(sym, idx, table, sizes, offsets)
    slot, count, st = ref.fold(*items, cap=64)
    assert st == ref.OVERFLOW and count == 0 and len(slot) == 64


def test_truncated_streams_read_zeros_like_the_host_decoder():
    sym, idx, table, sizes, offsets = _case(92, 1000, 0.1, 13)
    full = _host.rans_encode_arrays(sym, idx, table, sizes, offsets)
    for cut in (8, len(full) - 4, len(full) // 2 // 4 * 4):
        want = _host.rans_decode_arrays(full[:cut], idx, table, sizes, offsets)
        got, st = ref.decode(full[:cut], idx, table, sizes, offsets)
        assert st in (0, ref.BAD_ESCAPE)
        if st == 0:
            assert np.array_equal(got, want)
    assert ref.decode(full[:6], idx, table, sizes, offsets)[1] == ref.BAD_STREAM


def test_nibble_cap():
    """A stream whose first escape claims 15 + c data nibbles: the host decoder would shift by >= 32; the device rule stops there."""
    table, sizes, offsets, _ = ref.make_table([2], 3)
    # a state whose low 16 bits are any slot (one bin: the escape), followed by count nibbles 15, 15: built by hand from put_bits
    x = ref.LOW
    for nibble in (3, 15, 15):
        x = (x << 4) | nibble
    x = (x << 16) | 0x1234                                       # freq 2^16, start 0: x = (x // 65536 << 16) + x % 65536 + 0
    stream = np.array([x & ref.M32, x >> 32], np.uint32).tobytes()
    got, st = ref.decode(stream, np.zeros(4, np.int32), table, sizes, offsets)
    assert st == ref.BAD_ESCAPE

"""The device rANS coder (hesic_amd/csrc/rans.hip, include/hesic_rans.h) restated in numpy / Python integers, step for step as the
kernels run it: the itemise phase, the backward fold with the emitted words written downwards into a slot of 8 n + 16 bytes, the
decoder's lane-count search over a row spread over 64 lanes, its 64-word stream window that reads zeros past the end, and the cap on
the nibble count.  tests/test_rans_device_cpu.py holds it byte for byte to the host coder; tests/test_gpu_rans_device.py holds the
kernels to the host coder directly and uses the case table below."""
import numpy as np

PRECISION, BYPASS = 16, 4
LOW = 1 << 31
ITEM_BAD = 0xFF
OVERFLOW, BAD_TABLE, BAD_ESCAPE, BAD_STREAM = 1, 2, 4, 8
M32, M64 = (1 << 32) - 1, (1 << 64) - 1


def require_full_range_host_coder():
    """The case table below holds rows of two entries and escapes of eight data nibbles.  The host coder before revision 2
    (``hesic_rans_coder_revision``, hesic_host.h) divides by zero on the first and never returns from the second, so a test that takes it
    as its yardstick fails in ``make_table`` against such a library instead of hanging the run."""
    from hesic_amd import _host
    if getattr(_host, "rans_coder_revision", lambda: 1)() < 2:               # a package from before the entry point has no such helper either
        raise AssertionError("libhesic_host.so is the rANS coder of revision 1: it cannot code the rows of two entries and the eight-nibble "
                             "escapes of this case table (rebuild it: make -C hesic_amd/csrc)")


def slot_bytes(n):
    return 8 * n + 16


def itemise(symbols, indexes, table, sizes, offsets):
    """rans_itemise_kernel: per symbol (start | (freq - 1) << 16, raw, flag); flag 0 modelled only, 1 + nib an escape, ITEM_BAD a bad row."""
    n = len(symbols)
    sf, raw_out, flag = np.zeros(n, np.uint32), np.zeros(n, np.uint32), np.full(n, ITEM_BAD, np.uint8)
    for i in range(n):
        ci = int(indexes[i])
        size = int(sizes[ci]) if 0 <= ci < len(sizes) else 0
        if not 2 <= size <= table.shape[1]:
            continue
        last = size - 2
        v = (int(symbols[i]) - int(offsets[ci])) & M32
        v = v - (1 << 32) if v >> 31 else v                      # the int32 wrap of the kernel
        raw, fl = 0, 0
        if v < 0:
            raw, v = ~((v & M32) << 1) & M32, last
        elif v >= last:
            raw, v = ((v - last) << 1) & M32, last
        if v == last:
            nib = 0
            while nib < 8 and raw >> (nib * BYPASS):
                nib += 1
            fl = 1 + nib
        start, freq = int(table[ci, v]) & 0xFFFF, (int(table[ci, v + 1]) - int(table[ci, v])) & M32
        if freq == 0 or freq > 65536:
            fl = ITEM_BAD
        sf[i], raw_out[i], flag[i] = start | (((freq - 1) & 0xFFFF) << 16), raw, fl
    return sf, raw_out, flag


def divmod_exact(x, f):
    """x // f, x % f the kernel's way: the truncated double product with 1.0 / f, then one remainder check."""
    inv = np.float64(1.0) / np.float64(f)
    q = int(np.float64(x) * inv)
    r = x - q * f
    if r < 0:
        q, r = q - 1, r + f
    elif r >= f:
        q, r = q + 1, r - f
    assert 0 <= r < f and q * f + r == x, (x, f)                 # the estimate was within one of the quotient
    return q, r


def fold(sf, raw, flag, cap=None):
    """rans_fold_kernel: -> (slot bytes (uint8, cap), count, status); the stream is the last ``count`` bytes of the slot."""
    n = len(sf)
    cap = slot_bytes(n) if cap is None else cap
    words = np.zeros(cap // 4, np.uint32)
    state = {"x": LOW, "wp": len(words), "st": 0}

    def emit():
        if state["wp"] == 0:
            state["st"] |= OVERFLOW
            return
        state["wp"] -= 1
        words[state["wp"]] = state["x"] & M32
        state["x"] >>= 32

    def put_bits(val):
        if state["x"] >= 1 << 59:
            emit()
        state["x"] = ((state["x"] << BYPASS) | val) & M64

    for i in range(n - 1, -1, -1):
        if state["st"]:
            break
        fl = int(flag[i])
        if fl == ITEM_BAD:
            state["st"] |= BAD_TABLE
            break
        if fl:
            nib = fl - 1
            for k in range(nib - 1, -1, -1):
                put_bits((int(raw[i]) >> (k * BYPASS)) & 15)
            put_bits(nib)
        start, freq = int(sf[i]) & 0xFFFF, (int(sf[i]) >> 16) + 1
        if state["x"] >= freq << 47:
            emit()
        if state["st"]:
            break
        q, r = divmod_exact(state["x"], freq)
        state["x"] = (q << PRECISION) + r + start
    if not state["st"]:
        if state["wp"] < 2:
            state["st"] |= OVERFLOW
        else:
            state["wp"] -= 2
            words[state["wp"]], words[state["wp"] + 1] = state["x"] & M32, state["x"] >> 32
    count = 0 if state["st"] else (len(words) - state["wp"]) * 4
    return words.view(np.uint8), count, state["st"]


def encode(symbols, indexes, table, sizes, offsets):
    """One stream: -> (bytes, status), the slot's tail."""
    slot, count, st = fold(*itemise(symbols, indexes, table, sizes, offsets))
    return bytes(slot[len(slot) - count:]), st


def decode(stream, indexes, table, sizes, offsets):
    """rans_decode_kernel for one stream: -> (int32 symbols, status).  The row lives in 64 lanes x KPL registers padded with 0xFFFFFFFF,
    the symbol is the number of entries <= slot minus one, start / next come from lanes s and s + 1; the stream is read through a window
    of 64 words that holds zeros past the end."""
    n = len(indexes)
    out = np.zeros(n, np.int32)
    nb = len(stream)
    if nb < 8 or nb % 4:
        return out, BAD_STREAM
    words = np.frombuffer(bytes(stream), np.uint32)
    kpl = (table.shape[1] + 63) // 64
    state = {"x": int(words[0]) | (int(words[1]) << 32), "pos": 2}

    def next_word():
        w = int(words[state["pos"]]) if state["pos"] < len(words) else 0
        state["pos"] += 1
        return w

    def get_bits():
        v = state["x"] & 15
        state["x"] >>= BYPASS
        if state["x"] < LOW:
            state["x"] = (state["x"] << 32) | next_word()
        return v

    cur, row, last, off = None, None, 0, 0
    for i in range(n):
        ci = int(indexes[i])
        if ci != cur:
            size = int(sizes[ci]) if 0 <= ci < len(sizes) else 0
            if not 2 <= size <= table.shape[1]:
                return out, BAD_TABLE
            row = np.full(64 * kpl, 0xFFFFFFFF, np.uint64)
            row[:size] = table[ci, :size].astype(np.int64) & M32
            cur, last, off = ci, size - 2, int(offsets[ci])
        slot = state["x"] & 0xFFFF
        s = int(np.count_nonzero(row <= slot)) - 1               # the ballots' popcounts
        s = min(max(s, 0), last)
        start, nxt = int(row[s]), int(row[s + 1])
        state["x"] = (((nxt - start) & M32) * (state["x"] >> PRECISION) + slot - start) & M64
        if state["x"] < LOW:
            state["x"] = (state["x"] << 32) | next_word()
        v = s
        if s == last:
            c = get_bits()
            nib = c
            while c == 15 and nib <= 8:
                c = get_bits()
                nib += c
            if nib > 8:
                return out, BAD_ESCAPE
            raw = 0
            for k in range(nib):
                raw |= get_bits() << (k * BYPASS)
            h = raw >> 1
            v = (~h & M32) if raw & 1 else (h + last) & M32
        sym = (v + off) & M32
        out[i] = sym - (1 << 32) if sym >> 31 else sym
    return out, 0


# ------------------------------------------------------------------------------------------------------------------ cases
def make_table(lengths, seed):
    """A (rows, max(lengths)) int32 table of valid quantised CDFs: row r has lengths[r] entries 0 = c[0] < ... < c[last + 1] = 2^16
    (every bin, the escape bin included, has a non-zero frequency), zeros behind; offsets around zero, medians with fractional parts.
    Every case begins here, so this is where a host coder that cannot serve as the yardstick of the case table is turned away."""
    require_full_range_host_coder()
    rng = np.random.default_rng(seed)
    stride = max(lengths)
    table = np.zeros((len(lengths), stride), np.int32)
    for r, size in enumerate(lengths):
        bins = size - 1
        w = rng.random(bins) ** 3 + 1e-3
        f = np.maximum(1, np.floor(w / w.sum() * (65536 - bins)).astype(np.int64))
        f[int(np.argmax(f))] += 65536 - int(f.sum())
        assert f.min() >= 1 and f.sum() == 65536
        table[r, 1:size] = np.cumsum(f)
    sizes = np.asarray(lengths, np.int32)
    offsets = (-(sizes - 2) // 2 + rng.integers(-3, 4, len(lengths))).astype(np.int32)
    medians = (rng.random(len(lengths)) * 8 - 4).astype(np.float32) + np.float32(0.37)
    return table, sizes, offsets, medians


def make_symbols(n, indexes, sizes, offsets, escapes, seed):
    """n symbols for the rows ``indexes``: ``escapes`` = 0 all inside the support, 0.1 a tenth outside (both signs), 1 all outside (a row of
    two entries has no support: its symbols are escapes whatever ``escapes`` says).
    Escape magnitudes (the distance from the support) are spread over 1 .. 7 data nibbles up to 2^27 - 1, which is planted at every
    (n // 4)-th place; raw = 2 * magnitude (- 1) of those is below 2^28, so an EIGHTH data nibble needs a magnitude of 2^27 or more:
    2^30 is planted next to each of them, the largest the int32 symbols leave room for."""
    rng = np.random.default_rng(seed)
    idx = np.asarray(indexes)
    last = sizes[idx].astype(np.int64) - 2
    inside = np.where(last > 0, rng.integers(0, 1 << 30, n) % np.maximum(last, 1), 0)
    mag = rng.integers(0, 1 << 62, n) % (1 << rng.integers(1, 28, n))
    step = max(1, n // 4)
    mag[::step] = (1 << 27) - 1
    mag[1::step] = 1 << 30
    sign = rng.random(n) < 0.5
    outside = np.where(sign, -1 - mag, last + mag)
    esc = (rng.random(n) < escapes) | (last == 0)
    v = np.where(esc, outside, inside)
    sym = v + offsets[idx]
    assert np.abs(sym).max() < 1 << 31
    return sym.astype(np.int32)


def channel_indexes(C, P):
    return np.repeat(np.arange(C, dtype=np.int32), P)

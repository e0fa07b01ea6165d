"""The stream coder of the device range coder (csrc/codec.hip) restated with Python integers: the state machine of
``hesic_rc_encoder_encode`` (64-bit low / range, TOP = 2^56, BOT = 2^48) with the SHORT flush -- the top two bytes of ``low`` rounded up
to a multiple of 2^48, trailing zero bytes dropped; a decoder reads zeros past the end.  A helper module of the tests, not a test."""
import numpy as np

TOP, BOT, MASK = 1 << 56, 1 << 48, (1 << 64) - 1


def _renorm(low, rng):
    """One evaluation of the coder's loop condition: (emit?, range after the underflow clamp)."""
    if (low ^ ((low + rng) & MASK)) < TOP:
        return True, rng
    if rng < BOT:
        return True, (-low) & (BOT - 1)
    return False, rng


def encode_stream(symbols, cdf):
    """(body, flush): the bytes in front of the flush and the 0-2 flush bytes of one stream coded under the rows of ``cdf`` (n, A + 1)."""
    low, rng, out = 0, MASK, bytearray()
    for s, c in zip(symbols, cdf):
        s, tot = int(s), int(c[-1])
        freq = int(c[s + 1]) - int(c[s])
        assert 0 < freq and 0 < tot < BOT
        rng //= tot
        low = (low + int(c[s]) * rng) & MASK
        rng *= freq
        while True:
            emit, rng = _renorm(low, rng)
            if not emit:
                break
            out.append(low >> 56)
            low = (low << 8) & MASK
            rng = (rng << 8) & MASK
    assert rng >= BOT and low + rng <= 1 << 64          # what the flush relies on
    v = (low + BOT - 1) & ~(BOT - 1)
    assert low <= v < low + rng and v < 1 << 64
    flush = bytes([v >> 56, (v >> 48) & 0xFF]).rstrip(b"\x00")
    return bytes(out), flush


def encode_bytes(symbols, cdf):
    body, flush = encode_stream(symbols, cdf)
    return body + flush


def decode_stream(data, cdf):
    """Symbols of one stream (zeros are read past its end), by the arithmetic of ``hesic_rc_decoder_decode_grid``."""
    data = bytes(data)
    pos = 0

    def nxt():
        nonlocal pos
        b = data[pos] if pos < len(data) else 0
        pos += 1
        return b

    low, rng, code = 0, MASK, 0
    for _ in range(8):
        code = (code << 8) | nxt()
    out = np.empty(len(cdf), dtype=np.int32)
    for i, c in enumerate(cdf):
        tot = int(c[-1])
        rng //= tot
        v = min(((code - low) & MASK) // rng, tot - 1)
        idx = int(np.searchsorted(np.asarray(c[:-1], dtype=np.int64), v, side="right")) - 1
        out[i] = idx
        low = (low + int(c[idx]) * rng) & MASK
        rng *= int(c[idx + 1]) - int(c[idx])
        while True:
            emit, rng = _renorm(low, rng)
            if not emit:
                break
            code = ((code << 8) | nxt()) & MASK
            low = (low << 8) & MASK
            rng = (rng << 8) & MASK
    return out


def random_tables(n, A, seed, least_likely=False):
    """(symbols, cdf): n rows over an alphabet of A symbols, quantised as the table kernels do (clip at 2^-16, total ~2^16)."""
    r = np.random.Generator(np.random.PCG64(seed))
    pm = r.dirichlet(np.ones(A) * 0.3, size=n).astype(np.float32)
    pc = np.clip(pm, 1.0 / 65536, 1.0)
    q = np.round(pc / pc.sum(1, keepdims=True) * 65536)
    cdf = np.concatenate([np.zeros((n, 1)), np.add.accumulate(q, 1)], 1).astype(np.uint32)
    if least_likely:
        sym = q.argmin(1).astype(np.int32)
    else:
        u = r.random(n) * q.sum(1)
        sym = np.minimum((np.add.accumulate(q, 1) <= u[:, None]).sum(1), A - 1).astype(np.int32)
    return sym, cdf

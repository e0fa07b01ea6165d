"""The C++ host coder (hesic_amd/csrc/host) against the REFERENCE's own extensions on randomised inputs: CDF tables equal, rANS streams
byte-identical, and they decode.  The reference's answers are recorded in tests/golden/codec_random.npz (tests/golden/make_golden.py
codec_random: the same generators and draws as the cases were once drawn here live, every recorded stream checked to decode by the
reference's own decoder)."""
import numpy as np

from conftest import load_golden

import hesic_amd  # noqa: F401
from compressai import ans as my_ans
from compressai._CXX import pmf_to_quantized_cdf as my_cdf


def _split(flat, lens):
    return np.split(flat, np.cumsum(lens)[:-1])


def test_pmf_to_quantized_cdf_random():
    g = load_golden("codec_random.npz")
    pmfs, cdfs = _split(g["pmf"], g["pmf_len"]), _split(g["cdf"], g["cdf_len"])
    assert len(pmfs) >= 190
    for trial, (p, c) in enumerate(zip(pmfs, cdfs)):
        assert my_cdf(p.tolist(), 16) == c.tolist(), trial


def test_rans_streams_random():
    g = load_golden("codec_random.npz")
    ntab, L, n = g["rans_ntab"], g["rans_L"], g["rans_n"]
    tables = _split(g["rans_table"], ntab * L)
    sizes, offsets = _split(g["rans_sizes"], ntab), _split(g["rans_offsets"], ntab)
    idxs, syms = _split(g["rans_idx"], n), _split(g["rans_sym"], n)
    streams = _split(g["rans_bytes"], g["rans_nbytes"])
    assert len(streams) == 40
    for trial in range(len(streams)):
        table = tables[trial].reshape(int(ntab[trial]), int(L[trial])).tolist()
        sz, off, idx, sym = sizes[trial].tolist(), offsets[trial].tolist(), idxs[trial].tolist(), syms[trial].tolist()
        ref = streams[trial].tobytes()
        a = my_ans.RansEncoder().encode_with_indexes(sym, idx, table, sz, off)
        assert a == ref, trial
        assert my_ans.RansDecoder().decode_with_indexes(ref, idx, table, sz, off) == sym

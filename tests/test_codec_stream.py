"""Real bit-stream of HSIC.compress / decompress (ywz/mywork/newnet1.py:823-1273).

CPU: the host range coder (libhesic_host) -- exact round trips, code length against the ideal, a pure-Python restatement
of the same published algorithm producing the same bytes.  GPU: the per-element CDF kernel against the oracle's
restatement of the reference's numpy/torch arithmetic, and a whole compress -> files -> decompress round trip."""
import numpy as np
import pytest
import torch

from conftest import T, load_golden
from hesic_amd import synthetic, _host


def _tables(n, A, seed):
    r = np.random.Generator(np.random.PCG64(seed))
    pm = r.dirichlet(np.ones(A) * 0.3, size=n).astype(np.float32)
    pc = np.clip(pm, 1.0 / 65536, 1.0)
    q = np.round(pc / pc.sum(1, keepdims=True) * 65536)
    cdf = np.concatenate([np.zeros((n, 1)), np.add.accumulate(q, 1)], 1).astype(np.uint32)
    sym = np.array([r.choice(A, p=q[i] / q[i].sum()) for i in range(n)], dtype=np.int32)
    return sym, cdf, q


def _py_range_encode(symbols, cdf):
    """The carry-less range coder of hesic_host.cpp restated with Python integers (64-bit low, 2^56 / 2^48)."""
    TOP, BOT, MASK = 1 << 56, 1 << 48, (1 << 64) - 1
    low, rng, out = 0, MASK, bytearray()
    for s, c in zip(symbols, cdf):
        tot = int(c[-1])
        rng //= tot
        low = (low + int(c[s]) * rng) & MASK
        rng *= int(c[s + 1]) - int(c[s])
        while True:
            if (low ^ ((low + rng) & MASK)) < TOP:
                pass
            elif rng < BOT:
                rng = (-low) & (BOT - 1)
            else:
                break
            out.append(low >> 56)
            low = (low << 8) & MASK
            rng = (rng << 8) & MASK
    for _ in range(8):
        out.append(low >> 56)
        low = (low << 8) & MASK
    return bytes(out)


def test_range_coder_round_trip_and_length():
    sym, cdf, q = _tables(6000, 33, 3)
    enc = _host.RangeEncoder()
    enc.encode(sym[:2500], cdf[:2500])          # two calls = the two views sharing one stream
    enc.encode(sym[2500:], cdf[2500:])
    data = enc.finish()
    dec = _host.RangeDecoder(data)
    back = np.concatenate([dec.decode(cdf[:2500]), dec.decode(cdf[2500:])])
    assert np.array_equal(back, sym)
    ideal = -np.log2(q[np.arange(len(sym)), sym] / q.sum(1)).sum() / 8
    assert ideal <= len(data) < ideal * 1.01 + 16
    assert data == _py_range_encode(sym, cdf)


def test_range_coder_edge_cases():
    # totals that are not powers of two, zero-frequency neighbours, a 2-symbol alphabet, an empty call
    cdf = np.array([[0, 0, 5, 5, 7], [0, 65535, 65536, 65536, 65540], [0, 1, 2, 3, 4]], dtype=np.uint32)
    sym = np.array([1, 0, 3], dtype=np.int32)
    enc = _host.RangeEncoder()
    enc.encode(sym, cdf)
    enc.encode(np.zeros(0, np.int32), np.zeros((0, 5), np.uint32))
    data = enc.finish()
    assert np.array_equal(_host.RangeDecoder(data).decode(cdf), sym)
    with pytest.raises(ValueError):             # a symbol whose table gives it zero frequency cannot be coded
        _host.RangeEncoder().encode(np.array([0], np.int32), cdf[:1])
    two = np.tile(np.array([[0, 3, 4]], np.uint32), (500, 1))
    s2 = (np.arange(500) % 7 == 0).astype(np.int32)
    e2 = _host.RangeEncoder()
    e2.encode(s2, two)
    assert np.array_equal(_host.RangeDecoder(e2.finish()).decode(two), s2)


def test_oracle_cdf_tables_shape_and_monotone():
    from oracle import hesic_oracle as O
    K, M, H, W = 3, 4, 2, 3
    sc = synthetic._uniform("cdf.s", (1, K * M, H, W), 0.05, 2.0)
    mu = synthetic._uniform("cdf.m", (1, K * M, H, W), -3, 3)
    w = torch.softmax(synthetic._uniform("cdf.w", (1, K, M), -1, 1), 1).reshape(1, K * M, 1, 1)
    t = O.compress_cdf_tables(sc, mu, w, [0, 2], 4, K, M)
    assert t.shape == (2, H, W, 10) and (t[..., 0] == 0).all()
    assert (np.diff(t.astype(np.int64), axis=-1) >= 1).all()          # clip at 2^-16 keeps every symbol codable
    assert (np.abs(t[..., -1].astype(np.int64) - 65536) <= 9).all()


def _ref_compress_case():
    from conftest import load_golden
    from oracle import hesic_oracle as O
    from test_oracle_golden import _model_params
    g = load_golden("codec_model_64.npz")
    P = _model_params("hsic")
    x1, x2, Hm = synthetic.stereo_batch(0, 1, 64, 64)
    with torch.no_grad():
        out = O.hsic_forward(P, x1, x2, Hm, return_gmm=True)
    return g, P, out


def test_oracle_tables_and_symbols_match_the_reference_compress_run():
    """tests/golden/codec_model_64.npz is a run of the reference's own HSIC.compress (newnet1.py:823-1066) with a recording
    stand-in for its third-party range-coder object: every encode([symbol], cdf) call in order.  The oracle reproduces the
    latent range, the coding order (channel-major over the non-zero channels, rows, columns; view 1 then view 2), every symbol
    and every cumulative-frequency table of view 1 (every third of view 2) -- exactly on the build container's CPU."""
    from oracle import hesic_oracle as O
    g, P, out = _ref_compress_case()
    n1, pos = int(g["n_view1"]), 0
    for v, (yk, gk) in enumerate((("y1_hat", "gmm1"), ("y2_hat", "gmm2"))):
        y = out[yk][0].numpy().astype(np.int64)
        minmax = int(max(np.abs(y).max(), 1))
        assert minmax == int(g["minmax"][v])
        channels = [c for c in range(192) if np.abs(y[c]).sum() > 0]
        sym = (y[channels] + minmax).reshape(-1)
        want = g["symbols"][pos:pos + sym.size]
        assert np.array_equal(sym, want)
        s_, m_, w_ = out[gk]
        tables = O.compress_cdf_tables(s_, m_, w_, channels, minmax, 5, 192).reshape(-1, 2 * minmax + 2)
        ref = (g["tables1"] if v == 0 else g["tables2_every3"]).astype(np.int64)
        got = (tables if v == 0 else tables[::3]).astype(np.int64)
        # exact on the CPU the fixture was made on; another CPU's conv kernels may move sigma / mu by an ulp and with it a frequency
        # on a rounding boundary by one count of 65536
        dfreq = np.abs(np.diff(got, axis=-1) - np.diff(ref, axis=-1))
        assert dfreq.max() <= 1 and (dfreq.max(axis=1) > 0).mean() < 0.02
        pos += sym.size
    assert pos == g["symbols"].size and n1 == 192 * 16


def test_oracle_joint_tables_and_symbols_match_the_reference_compress_run():
    """tests/golden/codec_model_joint_64.npz: the reference's own HESIC+ ``HSIC.compress`` (newnet1_joint.py:793-1079) recorded call
    by call.  The oracle's full-map context model reproduces what the reference computes crop by crop: the latent range, the
    coding order (raster over the pixels, the non-zero channels of a pixel together; view 1 then view 2), every symbol and every
    cumulative-frequency table."""
    from oracle import hesic_oracle as O
    g = load_golden("codec_model_joint_64.npz")
    from hesic_amd import models
    net = models.HSICJoint()
    synthetic.fill_state_dict_(net.state_dict())
    P = {k: v.clone() for k, v in net.state_dict().items()}
    x1, x2, Hm = synthetic.stereo_batch(0, 1, 64, 64)
    with torch.no_grad():
        out = O.hsic_joint_forward(P, x1, x2, Hm, return_params=True)
    pos = 0
    for v, (yk, gk) in enumerate((("y1_hat", "gauss1"), ("y2_hat", "gauss2"))):
        y = out[yk][0].numpy().astype(np.int64)
        minmax = int(max(np.abs(y).max(), 1))
        assert minmax == int(g["minmax"][v])
        channels = [c for c in range(192) if np.abs(y[c]).sum() > 0]
        sym = (y[channels] + minmax).transpose(1, 2, 0).reshape(-1)            # pixel-major, channels inside
        assert np.array_equal(sym, g["symbols"][pos:pos + sym.size])
        sc, mu = out[gk]
        tables = O.compress_cdf_tables(sc, mu, torch.ones(1, 192, 1, 1), channels, minmax, 1, 192)      # (C, H, W, n)
        got = tables.transpose(1, 2, 0, 3).reshape(-1, 2 * minmax + 2).astype(np.int64)
        ref = g["tables1" if v == 0 else "tables2"].astype(np.int64)
        dfreq = np.abs(np.diff(got, axis=-1) - np.diff(ref, axis=-1))
        # the reference evaluates the masked conv on 5x5 crops, the oracle on the whole map: the same sums in another blocking -- a
        # frequency on a rounding boundary may move by one count of 65536
        assert dfreq.max() <= 1 and (dfreq.max(axis=1) > 0).mean() < 0.05, (v, dfreq.max(), (dfreq.max(axis=1) > 0).mean())     # measured: 3 % of the rows
        pos += sym.size
    assert pos == g["symbols"].size


def test_side_information_file_matches_the_reference_byte_for_byte():
    """The header file the reference writes (uint16 H, W; per view uint16 len(z), uint16 minmax, M/8 flag bytes, the
    EntropyBottleneck rANS string; newnet1.py:876-906) rebuilt from the oracle's latents with THIS repository's
    EntropyBottleneck.update / compress (host C++ coder): identical bytes."""
    from compressai.entropy_models import EntropyBottleneck
    g, P, out = _ref_compress_case()
    head = bytearray(np.array([64, 64], dtype=np.uint16).tobytes())
    for v in (1, 2):
        eb = EntropyBottleneck(128)
        eb.load_state_dict({k.split(".", 1)[1]: t for k, t in P.items() if k.startswith(f"entropy_bottleneck{v}.") and "_offset" not in k
                            and "_quantized_cdf" not in k and "_cdf_length" not in k}, strict=False)
        eb.update(force=True)
        z_string = eb.compress(out[f"z{v}"])[0]
        y = out[f"y{v}_hat"][0].numpy().astype(np.int64)
        flag = (np.abs(y).sum(axis=(1, 2)) > 0).astype(np.uint8)
        head += np.array([len(z_string), max(int(np.abs(y).max()), 1)], dtype=np.uint16).tobytes() + np.packbits(flag).tobytes() + z_string
        assert len(z_string) == int(g["zlen"][v - 1])
        back = eb.decompress([z_string], out[f"z{v}"].shape[-2:])
        assert torch.equal(back, out[f"z{v}_hat"])
    assert bytes(head) == g["header"].tobytes()


# ----------------------------------------------------------------------------------------------- GPU
@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_gpu_cdf_tables_match_oracle(dtype):
    from hesic_amd import functional as Fn
    from oracle import hesic_oracle as O
    K, M, H, W = 5, 16, 6, 5
    sc = synthetic._uniform("gcdf.s", (1, K * M, H, W), 0.02, 3.0).to(dtype)
    mu = synthetic._uniform("gcdf.m", (1, K * M, H, W), -6, 6).to(dtype)
    w = torch.softmax(synthetic._uniform("gcdf.w", (1, K, M), -1, 1), 1).reshape(1, K * M, 1, 1)
    ch = [0, 3, 7, 15]
    for minmax in (1, 7, 70):                   # alphabets of 3, 15 and 141 (> 128: numpy's recursive pairwise sum)
        want = O.compress_cdf_tables(sc.float(), mu.float(), w, ch, minmax, K, M).astype(np.int64)
        got = Fn.gmm_cdf_tables(sc.cuda(), mu.cuda(), w.cuda(), ch, minmax, K).cpu().numpy().view(np.uint32).astype(np.int64)
        assert got.shape == want.shape
        # the erfc of the device library and of torch's CPU build differ in the last ulp of some pmf values: a frequency
        # sitting on a rounding boundary then moves by one count (of 65536) in a few tables; anything beyond is a bug
        dfreq = np.abs(np.diff(got, axis=-1) - np.diff(want, axis=-1))
        rows_off = (dfreq.reshape(-1, dfreq.shape[-1]).max(1) > 0).mean()
        assert dfreq.max() <= 1 and rows_off < 0.05, (minmax, dfreq.max(), rows_off)
        assert (got[..., 0] == 0).all() and (np.diff(got, axis=-1) >= 1).all()


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16], ids=["f32", "bf16", "f16"])
def test_gpu_compress_decompress_round_trip(tmp_path, dtype):
    import hesic_amd
    from hesic_amd import models
    prev = hesic_amd.functional.compute_dtype()
    hesic_amd.set_compute_dtype(dtype)
    try:
        net = models.HSIC()
        synthetic.fill_state_dict_(net.state_dict())
        net = net.cuda().eval()
        net.update(force=True)
        x1, x2, Hm = (t.cuda() for t in synthetic.stereo_batch(3, 1, 256, 256))
        with torch.no_grad():
            fwd = net(x1, x2, Hm)
        enc = net.compress(x1, x2, Hm, "pair", str(tmp_path))
        head, payload = (tmp_path / "pair.npz").read_bytes(), (tmp_path / "pair.bin").read_bytes()
        # header layout of newnet1.py:876-906
        assert np.frombuffer(head[:4], np.uint16).tolist() == [256, 256]
        len1, minmax1 = np.frombuffer(head[4:8], np.uint16)
        assert minmax1 == max(int(fwd["y1_hat"].abs().max()), 1)
        assert len(head) == 4 + 2 * (4 + net.M // 8) + int(len1) + int(np.frombuffer(head[8 + net.M // 8 + len1:][:2], np.uint16)[0])
        assert torch.equal(enc["y1_hat"].float(), fwd["y1_hat"].float()) and torch.equal(enc["y2_hat"].float(), fwd["y2_hat"].float())
        dec = net.decompress(None, None, Hm, "pair", str(tmp_path))
        assert torch.equal(dec["y1_hat"].float().cpu(), fwd["y1_hat"].float().cpu())
        assert torch.equal(dec["y2_hat"].float().cpu(), fwd["y2_hat"].float().cpu())
        assert torch.equal(dec["x1_hat"].float().cpu(), fwd["x1_hat"].float().cpu())
        assert torch.equal(dec["x2_hat"].float().cpu(), fwd["x2_hat"].float().cpu())
        # the real stream costs what the likelihoods promise once every symbol probability is floored at 2^-16, the
        # resolution of the coder's tables (with synthetic weights many latents sit far in the tails, so the unfloored
        # estimate is higher); range-coder termination, header and table quantisation are the slack
        L = fwd["likelihoods"]
        est = sum(float(-torch.log2(L[k].float().clamp_min(2.0 ** -16)).sum()) for k in ("y1", "y2"))
        est += sum(float(-torch.log2(L[k].float()).sum()) for k in ("z1", "z2"))
        est /= 2 * 256 * 256
        assert abs(enc["bpp_real"] - est) < 0.03 * est + 0.02, (enc["bpp_real"], est)
        assert len(payload) > 0
    finally:
        hesic_amd.set_compute_dtype(prev)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16], ids=["f32", "bf16", "f16"])
def test_gpu_joint_compress_decompress_round_trip(tmp_path, dtype):
    """HESIC+ (newnet1_joint.py:793-1321): the decoder re-derives every pixel's (scale, mean) from the latents decoded so
    far (5x5 crop -> masked conv -> 1x1 net), the encoder evaluates the same model on the whole map at once -- the
    stream only decodes if the two agree bit for bit."""
    import hesic_amd
    from hesic_amd import models
    prev = hesic_amd.functional.compute_dtype()
    hesic_amd.set_compute_dtype(dtype)
    try:
        net = models.HSICJoint()
        synthetic.fill_state_dict_(net.state_dict())
        net = net.cuda().eval()
        net.update(force=True)
        x1, x2, Hm = (t.cuda() for t in synthetic.stereo_batch(4, 1, 128, 192))
        enc = net.compress(x1, x2, Hm, "pair", str(tmp_path))
        head = (tmp_path / "pair.npz").read_bytes()
        assert np.frombuffer(head[:4], np.uint16).tolist() == [128, 192]
        dec = net.decompress(None, None, Hm, "pair", str(tmp_path))
        assert torch.equal(dec["y1_hat"].float().cpu(), enc["y1_hat"].float().cpu())
        assert torch.equal(dec["y2_hat"].float().cpu(), enc["y2_hat"].float().cpu())
        with torch.no_grad(), hesic_amd.functional.no_split_k():
            fwd = net(x1, x2, Hm)
        assert torch.equal(fwd["y1_hat"].float().cpu(), enc["y1_hat"].float().cpu())
        assert torch.equal(dec["x1_hat"].float().cpu(), fwd["x1_hat"].float().cpu())
        assert torch.equal(dec["x2_hat"].float().cpu(), fwd["x2_hat"].float().cpu())
        L = fwd["likelihoods"]
        est = sum(float(-torch.log2(L[k].float().clamp_min(2.0 ** -16)).sum()) for k in ("y1", "y2"))
        est += sum(float(-torch.log2(L[k].float()).sum()) for k in ("z1", "z2"))
        est /= 2 * 128 * 192
        # loose: the forward's likelihood is evaluated at round(y - mu) + mu (GaussianConditional quantises around the mean,
        # newnet1_joint.py:689-691) while the stream, like the reference's, codes round(y) under the same Gaussian
        assert abs(enc["bpp_real"] - est) < 0.15 * est + 0.05, (enc["bpp_real"], est)
    finally:
        hesic_amd.set_compute_dtype(prev)


@pytest.mark.gpu
def test_gpu_compress_matches_the_reference_compress_run(tmp_path):
    """HSIC.compress on the HIP path (fp32) against the recorded reference run: the side-information file byte for byte, and the
    cumulative-frequency tables of hesic_gmm_cdf in the reference's coding order (a frequency on a rounding boundary may move
    by one count of 65536 where the device erfc differs in the last ulp)."""
    import hesic_amd
    from conftest import load_golden
    from hesic_amd import models
    g = load_golden("codec_model_64.npz")
    prev = hesic_amd.functional.compute_dtype()
    hesic_amd.set_compute_dtype(torch.float32)
    try:
        net = models.HSIC()
        synthetic.fill_state_dict_(net.state_dict())
        net.update(force=True)           # the z tables built where the recorded run built them (host), then carried like a
        net = net.cuda().eval()          # checkpoint's _quantized_cdf buffers: a device sigmoid may move a frequency by one count
        x1, x2, Hm = (t.cuda() for t in synthetic.stereo_batch(0, 1, 64, 64))
        net.compress(x1, x2, Hm, "pair0", str(tmp_path))
        assert open(tmp_path / "pair0.npz", "rb").read() == g["header"].tobytes()
        with torch.no_grad():
            v1, v2 = net._analysis(x1, x2, Hm)
        n1, pos = int(g["n_view1"]), 0
        for v, (y_hat, _z, _s, gmm) in enumerate((v1, v2)):
            minmax = int(g["minmax"][v])
            chans = list(range(192))
            sym, tabs = [], []
            for _ch, s_, cdf in net._cdf_chunks(gmm, chans, minmax, net.gaussian1._bound(), y_hat):
                sym.append(s_)
                tabs.append(cdf.astype(np.int64))
            sym, tabs = np.concatenate(sym), np.concatenate(tabs)
            assert np.array_equal(sym, g["symbols"][pos:pos + sym.size])
            ref = (g["tables1"] if v == 0 else g["tables2_every3"]).astype(np.int64)
            got = tabs if v == 0 else tabs[::3]
            dfreq = np.abs(np.diff(got, axis=-1) - np.diff(ref, axis=-1))
            assert dfreq.max() <= 1 and (dfreq.max(axis=1) > 0).mean() < 0.05
            pos += sym.size
    finally:
        hesic_amd.set_compute_dtype(prev)


@pytest.mark.gpu
def test_gpu_joint_compress_matches_the_reference_compress_run(tmp_path):
    """HSICJoint.compress(order="raster") on the HIP path (fp32) against the recorded reference run of newnet1_joint.HSIC.compress:
    the side-information file byte for byte, the symbols in the reference's coding order, the tables within one count of 65536."""
    import hesic_amd
    from conftest import load_golden
    from hesic_amd import functional as Fn, models
    g = load_golden("codec_model_joint_64.npz")
    prev = Fn.compute_dtype()
    hesic_amd.set_compute_dtype(torch.float32)
    try:
        net = models.HSICJoint()
        synthetic.fill_state_dict_(net.state_dict())
        net.update(force=True)           # host-built z tables, carried like a checkpoint's buffers (see the HESIC test above)
        net = net.cuda().eval()
        x1, x2, Hm = (t.cuda() for t in synthetic.stereo_batch(0, 1, 64, 64))
        calls = []
        from hesic_amd import _host
        real = _host.RangeEncoder

        class Spy(real):
            def encode(self, sym, cdf):
                calls.append((np.array(sym), np.array(cdf)))
                return super().encode(sym, cdf)

        _host.RangeEncoder = Spy
        try:
            net.compress(x1, x2, Hm, "pair0", str(tmp_path), order="raster")
        finally:
            _host.RangeEncoder = real
        assert open(tmp_path / "pair0.npz", "rb").read() == g["header"].tobytes()
        sym = np.concatenate([c[0].reshape(-1) for c in calls])
        assert np.array_equal(sym, g["symbols"])
        n1 = int(g["n_view1"])
        tabs = [np.concatenate([c[1] for c in calls if c[1].shape[-1] == 2 * int(g["minmax"][v]) + 2]) for v in (0, 1)]
        if int(g["minmax"][0]) == int(g["minmax"][1]):
            both = tabs[0]
            tabs = [both[:n1], both[n1:]]
        for v in (0, 1):
            got, ref = tabs[v].astype(np.int64), g["tables1" if v == 0 else "tables2"].astype(np.int64)
            assert got.shape == ref.shape
            dfreq = np.abs(np.diff(got, axis=-1) - np.diff(ref, axis=-1))
            assert dfreq.max() <= 1 and (dfreq.max(axis=1) > 0).mean() < 0.05, (v, dfreq.max(), (dfreq.max(axis=1) > 0).mean())
        dec = net.decompress(None, None, Hm, "pair0", str(tmp_path))
        assert np.array_equal((dec["y1_hat"][0].float().cpu().numpy().astype(np.int64) + int(g["minmax"][0])).transpose(1, 2, 0).reshape(-1),
                              g["symbols"][:n1])
    finally:
        hesic_amd.set_compute_dtype(prev)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16], ids=["f32", "bf16", "f16"])
def test_gpu_joint_wavefront_and_raster_payloads_decode_to_the_same_latents(tmp_path, dtype):
    """The wavefront payload (default: pixels grouped by w + 3h, one batched device step per group) and the raster payload (the
    reference's order, one step per pixel) carry the same symbols under the same tables: both decode to the encoder's latents and
    reconstructions bit for bit, and the payloads have the same length to within the coder's termination bytes."""
    import time
    import hesic_amd
    from hesic_amd import functional as Fn, models
    prev = Fn.compute_dtype()
    hesic_amd.set_compute_dtype(dtype)
    try:
        net = models.HSICJoint()
        synthetic.fill_state_dict_(net.state_dict())
        net = net.cuda().eval()
        net.update(force=True)
        x1, x2, Hm = (t.cuda() for t in synthetic.stereo_batch(5, 1, 128, 192))
        outs, times, sizes = {}, {}, {}
        for order in ("wavefront", "raster"):
            enc = net.compress(x1, x2, Hm, order, str(tmp_path), order=order)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            dec = net.decompress(None, None, Hm, order, str(tmp_path))
            torch.cuda.synchronize()
            times[order] = time.perf_counter() - t0
            sizes[order] = len((tmp_path / (order + ".bin")).read_bytes())
            blob = (tmp_path / (order + ".bin")).read_bytes()
            assert blob[:4] == models.PAYLOAD_MAGIC and blob[4:6] == models.payload_mode_bytes() and blob[6] == (1 if order == "wavefront" else 0)
            for k in ("y1_hat", "y2_hat"):
                assert torch.equal(dec[k].float().cpu(), enc[k].float().cpu()), (order, k)
            outs[order] = dec
        for k in ("x1_hat", "x2_hat", "y1_hat", "y2_hat"):
            assert torch.equal(outs["wavefront"][k].float().cpu(), outs["raster"][k].float().cpu()), k
        assert abs(sizes["wavefront"] - sizes["raster"]) <= 8
        assert (tmp_path / "wavefront.npz").read_bytes() == (tmp_path / "raster.npz").read_bytes()
        print("decode seconds", times)          # reported, not asserted: 33 group steps against 96 pixel steps per view on this 8 x 12 latent map
        # bounded encoder memory: with a table budget of a few groups the wavefront payload is byte-identical to the one-band payload
        ref_bytes = (tmp_path / "wavefront.bin").read_bytes()
        keep, net._TABLE_BYTES = net._TABLE_BYTES, 64 << 10
        try:
            net.compress(x1, x2, Hm, "banded", str(tmp_path), order="wavefront")
        finally:
            net._TABLE_BYTES = keep
        assert (tmp_path / "banded.bin").read_bytes() == ref_bytes
    finally:
        hesic_amd.set_compute_dtype(prev)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["hsic", "joint"])
def test_gpu_payload_names_its_table_mode_and_a_mismatched_decoder_raises(tmp_path, kind):
    """The .bin container starts with the format magic and two MODE bytes (storage format of the maps, error-feedback weights, fp32
    latents, table-kernel version; round 5: warp convention, split-K / grouped hyper-synthesis launches, analysis precision).  A decoder in another mode -- whose tables would differ in the last count and silently desynchronise
    the range decoder -- raises a ValueError that names both modes; so does a headerless (round 2-3) payload."""
    import hesic_amd
    from hesic_amd import functional as Fn, models
    prev = Fn.compute_dtype()
    try:
        hesic_amd.set_compute_dtype(torch.float16)
        net = (models.HSIC if kind == "hsic" else models.HSICJoint)()
        synthetic.fill_state_dict_(net.state_dict())
        net = net.cuda().eval()
        net.update(force=True)
        x1, x2, Hm = (t.cuda() for t in synthetic.stereo_batch(3, 1, 64, 64))
        enc = net.compress(x1, x2, Hm, "p", str(tmp_path))
        blob = (tmp_path / "p.bin").read_bytes()
        assert blob[:4] == models.PAYLOAD_MAGIC and blob[4] & 3 == 2 and blob[4] >> 4 == models.TABLE_KERNEL_VERSION
        dec = net.decompress(None, None, Hm, "p", str(tmp_path))
        for k in ("y1_hat", "y2_hat"):
            assert torch.equal(dec[k].float().cpu(), enc[k].float().cpu()), k
        hesic_amd.set_compute_dtype(torch.bfloat16)
        with pytest.raises(ValueError, match="float16 maps.*bfloat16 maps"):
            net.decompress(None, None, Hm, "p", str(tmp_path))
        hesic_amd.set_compute_dtype(torch.float16)
        # the OTHER warp convention (kornia <= 0.4): x1_hat_warp, hence view 2's tables, would differ -- round 4's header did not name it
        from hesic_amd import geometry
        keep_ac = geometry.use_reference_era_warp(True)
        try:
            with pytest.raises(ValueError, match="align_corners=True.*align_corners=False"):
                net.decompress(None, None, Hm, "p", str(tmp_path))
        finally:
            geometry.use_reference_era_warp(not keep_ac)
        # the summation-order switches of the hyper-synthesis are in the header too
        keep_sk, Fn.SPLIT_K = Fn.SPLIT_K, not Fn.SPLIT_K
        try:
            with pytest.raises(ValueError, match="split-K"):
                net.decompress(None, None, Hm, "p", str(tmp_path))
        finally:
            Fn.SPLIT_K = keep_sk
        dec = net.decompress(None, None, Hm, "p", str(tmp_path))      # and back in the writer's mode it decodes again
        assert torch.equal(dec["y2_hat"].float().cpu(), enc["y2_hat"].float().cpu())
        (tmp_path / "old.npz").write_bytes((tmp_path / "p.npz").read_bytes())
        (tmp_path / "old.bin").write_bytes(blob[6:])                 # what rounds 2-3 wrote: no header
        with pytest.raises(ValueError, match="format-3 header"):
            net.decompress(None, None, Hm, "old", str(tmp_path))
    finally:
        hesic_amd.set_compute_dtype(torch.bfloat16)
        hesic_amd.set_compute_dtype(prev)


@pytest.mark.gpu
def test_gpu_joint_decode_walk_tape_and_graph_fallback_agree(tmp_path, monkeypatch):
    """The HESIC+ wavefront decode walk issues a group's device step in one of two forms: its recorded launches replayed one by one
    (``hesic_joint_decode_groups_tape``), or -- where ``tape_from_calls`` cannot express the step (forced here by making it raise
    ``KeyError``) -- its captured graph (``hesic_joint_decode_groups``).  Both decode one payload to the same latents and reconstructions,
    bit for bit (what they change is who issues the launches, not what is launched), and each form really takes its own entry point."""
    from hesic_amd import models, _lib as L
    net = models.HSICJoint()
    synthetic.fill_state_dict_(net.state_dict())
    net = net.cuda().eval()
    net.update(force=True)
    x1, x2, Hm = (t.cuda() for t in synthetic.stereo_batch(7, 1, 128, 192))
    enc = net.compress(x1, x2, Hm, "w", str(tmp_path), order="wavefront")
    ref = None

    def no_tape(calls):
        raise KeyError("an entry point outside TAPE_IDS")

    walks = {"tape": "hesic_joint_decode_groups_tape", "graph": "hesic_joint_decode_groups"}
    for form in ("tape", "graph"):
        if form == "graph":
            monkeypatch.setattr(L, "tape_from_calls", no_tape)
        net.__dict__.pop("_wf_cache", None)          # the cached steps hold the tapes; the captured graphs the symbol buffer's address
        for rep in range(2):                          # second decode: the cached graphs, another pass over the same state
            seen = []
            with L.call_hook(lambda name, a: seen.append(name)):
                dec = net.decompress(None, None, Hm, "w", str(tmp_path))
            assert [n for n in seen if n in walks.values()] == [walks[form]] * 2, (form, rep)          # one walk per view, by this form's route
            for k in ("y1_hat", "y2_hat"):
                assert torch.equal(dec[k].float().cpu(), enc[k].float().cpu()), (form, rep, k)
            if ref is None:
                ref = dec
            for k in ("x1_hat", "x2_hat"):
                assert torch.equal(dec[k].cpu(), ref[k].cpu()), (form, rep, k)
    net.__dict__.pop("_wf_cache", None)


@pytest.mark.gpu
def test_gpu_joint_decode_walk_reports_a_corrupt_payload(tmp_path):
    """A payload cut short desynchronises the range decoder inside the C walk; the walk must end with a Python exception or a wrong
    latent map, never hang or crash (the decoder reads zeros past the end of its buffer, like the reference's)."""
    from hesic_amd import models
    net = models.HSICJoint()
    synthetic.fill_state_dict_(net.state_dict())
    net = net.cuda().eval()
    net.update(force=True)
    x1, x2, Hm = (t.cuda() for t in synthetic.stereo_batch(7, 1, 128, 192))
    enc = net.compress(x1, x2, Hm, "w", str(tmp_path), order="wavefront")
    blob = (tmp_path / "w.bin").read_bytes()
    (tmp_path / "w.bin").write_bytes(blob[:len(blob) // 2])
    try:
        dec = net.decompress(None, None, Hm, "w", str(tmp_path))
    except (ValueError, RuntimeError):
        return
    assert not torch.equal(dec["y2_hat"].float().cpu(), enc["y2_hat"].float().cpu())

"""Device-resident range coder (csrc/codec.hip) and the batched bit-stream API on top of it (HSIC.compress_batch / decompress_batch).

The kernels are held to the existing, trusted pieces: the coding intervals to the entries of ``Fn.gmm_cdf_tables``, bit for bit; the
device encoder's bytes to the host ``RangeEncoder`` over those tables; the device decoder to both.  The model-level tests ask what
``test_gpu_compress_decompress_round_trip`` asks of the per-pair path: reconstructions ``torch.equal`` to the eval forward."""
import time

import numpy as np
import pytest
import torch

import memguard as MG
import hesic_amd
from hesic_amd import _host, bitstream, synthetic
from hesic_amd import functional as Fn

pytestmark = pytest.mark.gpu
DEV = "cuda"
CL = torch.channels_last
K, M, B, H, W = 5, 192, 3, 16, 20
DTYPES = [torch.float32, torch.bfloat16, torch.float16]
IDS = ["f32", "bf16", "f16"]
# per-image alphabets of a batch: every list holds the value the case is named after, and the images of a batch differ
MINMAX_CASES = {1: [1, 6, 1], 6: [6, 40, 1], 40: [40, 6, 3], 511: [511, 1, 40]}


def _case(dtype, minmax, seed=0):
    """Random mixtures in ``dtype`` storage, latents inside each image's alphabet, per-image channel lists (all / every other / a
    random subset); unlisted channels of y_hat are zero."""
    hesic_amd.set_compute_dtype(dtype)
    g = torch.Generator().manual_seed(1000 + seed)
    sc = (torch.rand(B, K * M, H, W, generator=g) * 2.98 + 0.02).to(dtype).to(DEV).contiguous(memory_format=CL)
    mu = (torch.rand(B, K * M, H, W, generator=g) * 12 - 6).to(dtype).to(DEV).contiguous(memory_format=CL)
    w = torch.softmax(torch.rand(B, K, M, generator=g) * 2 - 1, 1).reshape(B, K * M, 1, 1).to(DEV)
    channels = [list(range(M)), list(range(0, M, 2)), sorted(torch.randperm(M, generator=g)[:150].tolist())]
    # y_hat in the storage dtype where it holds every integer of the alphabet exactly (bf16: up to 256), else fp32
    ydt = dtype if max(minmax) <= 256 else torch.float32
    y = torch.zeros(B, M, H, W)
    for b in range(B):
        mm = minmax[b]
        # mostly near the means (short codes), some anywhere in the alphabet, the two ends always present
        near = torch.round(torch.randn(len(channels[b]), H, W, generator=g) * 2).clamp(-mm, mm)
        far = torch.randint(-mm, mm + 1, near.shape, generator=g).float()
        v = torch.where(torch.rand(near.shape, generator=g) < 0.1, far, near)
        v[0, 0, 0], v[-1, -1, -1] = -mm, mm
        y[b, channels[b]] = v
    y = y.to(ydt).to(DEV).contiguous(memory_format=CL)
    return sc, mu, w, y, channels


def _tables(sc, mu, w, channels, minmax, b):
    return Fn.gmm_cdf_tables(sc, mu, w, channels[b], minmax[b], K, b=b)          # (n_ch, H, W, A + 1) int32 (uint32 bits)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("mm", [1, 6, 40, 511])
def test_ranges_equal_the_table_entries(dtype, mm):
    minmax = MINMAX_CASES[mm]
    sc, mu, w, y, channels = _case(dtype, minmax)
    tr = Fn.gmm_rc_ranges(sc, mu, w, y, minmax, channels, K)
    assert tr.shape == (B, M, H, W, 3) and tr.dtype == torch.int32
    for b in range(B):
        tab = _tables(sc, mu, w, channels, minmax, b).long() & 0xFFFFFFFF
        sym = (y[b, channels[b]].float() + minmax[b]).long()
        assert int(sym.min()) >= 0 and int(sym.max()) <= 2 * minmax[b]
        lo = torch.gather(tab, 3, sym[..., None])[..., 0]
        hi = torch.gather(tab, 3, sym[..., None] + 1)[..., 0]
        want = torch.stack([lo, hi - lo, tab[..., -1]], -1)
        got = tr[b, :len(channels[b])].long()
        bad = int((got != want).any(-1).sum())
        assert bad == 0, (b, minmax[b], bad, want.shape)
        assert int(want[..., 1].min()) >= 1


def _split(data, counts, channels, cps):
    """Device payload -> {(b, s): bytes}; counts beyond an image's streams must be zero."""
    data, counts = data.cpu().numpy().tobytes(), counts.cpu().tolist()
    out, pos = {}, 0
    for b in range(len(counts)):
        ns = (len(channels[b]) + cps - 1) // cps
        assert all(n == 0 for n in counts[b][ns:])
        for s in range(ns):
            out[b, s] = data[pos:pos + counts[b][s]]
            pos += counts[b][s]
    assert pos == len(data)
    return out


def _host_streams(sc, mu, w, y, channels, minmax, cps):
    """{(b, s): (host bytes with the 8-byte flush, symbols, tables)} of every stream, by the host coder over Fn.gmm_cdf_tables."""
    out = {}
    for b in range(B):
        tab = _tables(sc, mu, w, channels, minmax, b).cpu().numpy().view(np.uint32)
        sym = (y[b, channels[b]].float().cpu().numpy().astype(np.int64) + minmax[b]).astype(np.int32)
        for s in range((len(channels[b]) + cps - 1) // cps):
            sl = slice(s * cps, (s + 1) * cps)
            sy, tb = sym[sl].reshape(-1), tab[sl].reshape(-1, tab.shape[-1])
            enc = _host.RangeEncoder()
            enc.encode(sy, tb)
            out[b, s] = (enc.finish(), sy, tb)
    return out


def _guarded(*ts):
    return [MG.guarded(t, name=f"input {i}") for i, t in enumerate(ts)]


ENC_CASES = [(torch.float32, 6, 1), (torch.float32, 6, 8), (torch.bfloat16, 40, 1), (torch.float16, 40, 8), (torch.float16, 6, 1),
             (torch.float32, 511, 8)]


@pytest.mark.parametrize("dtype,mm,cps", ENC_CASES, ids=[f"{IDS[DTYPES.index(d)]}-mm{m}-cps{c}" for d, m, c in ENC_CASES])
def test_device_encoder_equals_the_host_encoder(dtype, mm, cps):
    minmax = MINMAX_CASES[mm]
    assert len(set(minmax)) > 1
    sc, mu, w, y, channels = _case(dtype, minmax, seed=cps)
    data, counts = Fn.gmm_rc_encode(sc, mu, w, y, minmax, channels, K, cps)
    assert counts.shape == (B, (M + cps - 1) // cps) and data.dtype == torch.uint8
    dev = _split(data, counts, channels, cps)
    host = _host_streams(sc, mu, w, y, channels, minmax, cps)
    assert dev.keys() == host.keys() and len(dev) == sum((len(c) + cps - 1) // cps for c in channels)
    for key, (hb, sy, tb) in host.items():
        d = dev[key]
        body = hb[:-8]
        assert d[:len(body)] == body, key
        assert len(body) <= len(d) <= len(body) + 2, (key, len(d), len(body))
        assert np.array_equal(_host.RangeDecoder(d).decode(tb), sy), key
    # the same with every input inside poisoned guards and every allocation of the wrappers poisoned: same bytes, guards intact
    gs = _guarded(sc, mu, w, y)
    with MG.poisoned_allocations([Fn]):
        data_g, counts_g = Fn.gmm_rc_encode(*gs, minmax, channels, K, cps)
    MG.check_all(gs)
    assert torch.equal(data_g, data) and torch.equal(counts_g, counts)


DEC_CASES = [(torch.float32, 6, 1), (torch.bfloat16, 40, 8), (torch.float16, 6, 8), (torch.float16, 40, 1), (torch.float32, 511, 8)]


@pytest.mark.parametrize("dtype,mm,cps", DEC_CASES, ids=[f"{IDS[DTYPES.index(d)]}-mm{m}-cps{c}" for d, m, c in DEC_CASES])
def test_device_decoder(dtype, mm, cps):
    minmax = MINMAX_CASES[mm]
    sc, mu, w, y, channels = _case(dtype, minmax, seed=10 + cps)
    ydt = y.dtype
    data, counts = Fn.gmm_rc_encode(sc, mu, w, y, minmax, channels, K, cps)
    back = Fn.gmm_rc_decode(sc, mu, w, minmax, channels, K, data, counts, ydt, cps)
    assert back.shape == y.shape and back.dtype == ydt and back.is_contiguous(memory_format=CL)
    assert torch.equal(back, y)
    for b in range(B):
        off = sorted(set(range(M)) - set(channels[b]))
        if off:
            assert int((back[b, off] != 0).sum()) == 0
    # host-coded streams of the same symbols (full 8-byte termination)
    host = _host_streams(sc, mu, w, y, channels, minmax, cps)
    S = (M + cps - 1) // cps
    hcounts = [[len(host[b, s][0]) if (b, s) in host else 0 for s in range(S)] for b in range(B)]
    hdata = torch.frombuffer(bytearray(b"".join(host[b, s][0] for b in range(B) for s in range(S) if (b, s) in host)), dtype=torch.uint8).to(DEV)
    assert torch.equal(Fn.gmm_rc_decode(sc, mu, w, minmax, channels, K, hdata, hcounts, ydt, cps), y)
    # guarded inputs -- the byte buffer ends flush against its trailing guard, so a read past the end of the payload meets 0xFF, not
    # luck -- and poisoned allocations: guards intact, no poison in the output, the same latents
    for payload, cnt in ((data, counts), (hdata, hcounts)):
        gs = _guarded(sc, mu, w)
        gdata = MG.guarded(payload, name="payload")
        g = gdata._memguard
        assert g.lead + g.nbytes <= g.buf.numel() - 4096 and int(g.buf[g.lead + g.nbytes]) == MG.NAN_FILL
        gcnt = MG.guarded(torch.as_tensor(cnt, dtype=torch.int32, device=DEV), name="counts")
        with MG.poisoned_allocations([Fn]):
            back_g = Fn.gmm_rc_decode(*gs, minmax, channels, K, gdata, gcnt, ydt, cps)
        MG.check_all(gs + [gdata, gcnt])
        assert bool(torch.isfinite(back_g.float()).all())
        assert torch.equal(back_g, y)


def test_a_damaged_payload_decodes_to_something_and_ends():
    """Garbage bytes and lengths that overrun the payload: the launch ends, writes only y_hat and yields finite values inside the alphabet."""
    minmax = MINMAX_CASES[6]
    sc, mu, w, y, channels = _case(torch.float32, minmax, seed=3)
    data, counts = Fn.gmm_rc_encode(sc, mu, w, y, minmax, channels, K, 8)
    g = torch.Generator().manual_seed(5)
    junk = MG.guarded(torch.randint(0, 256, (data.numel(),), generator=g, dtype=torch.uint8).to(DEV), name="payload")
    wrong = counts.clone()
    wrong[0, 0] = 1 << 30                      # a stream claiming more than the payload holds
    wrong[1, 1] = 0
    gs = _guarded(sc, mu, w)
    with MG.poisoned_allocations([Fn]):
        out = Fn.gmm_rc_decode(*gs, minmax, channels, K, junk, wrong, torch.float32, 8)
    torch.cuda.synchronize()
    MG.check_all(gs + [junk])
    for b in range(B):
        assert float(out[b].abs().max()) <= minmax[b]


# ---------------------------------------------------------------------------------------------------------------- model
def _net(dtype):
    from hesic_amd import models
    hesic_amd.set_compute_dtype(dtype)
    net = models.HSIC()
    synthetic.fill_state_dict_(net.state_dict())
    net = net.cuda().eval()
    net.update(force=True)
    return net


def _same(a, b):
    return torch.equal(a.float().cpu(), b.float().cpu())


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("shape", [(4, 128, 192), (2, 256, 320)], ids=["b4-128x192", "b2-256x320"])
def test_model_round_trip_equals_the_eval_forward(dtype, shape):
    net = _net(dtype)
    x1, x2, Hm = (t.cuda() for t in synthetic.stereo_batch(3, *shape))
    with torch.no_grad():
        fwd = net(x1, x2, Hm)
    enc = net.compress_batch(x1, x2, Hm)
    assert len(enc["blobs"]) == shape[0] == len(enc["bpp_real"]) and all(isinstance(b, bytes) for b in enc["blobs"])
    assert _same(enc["y1_hat"], fwd["y1_hat"]) and _same(enc["y2_hat"], fwd["y2_hat"])
    dec = net.decompress_batch(enc["blobs"], Hm)
    for k in ("y1_hat", "y2_hat", "x1_hat", "x2_hat"):
        assert dec[k].shape == fwd[k].shape
        assert _same(dec[k], fwd[k]), k
    for k in ("z1_hat", "z2_hat"):
        assert _same(dec[k], enc[k]), k


@pytest.mark.parametrize("dtype", [torch.float16, torch.float32], ids=["f16", "f32"])
def test_pairs_are_independent_of_the_batch(dtype):
    net = _net(dtype)
    x1, x2, Hm = (t.cuda() for t in synthetic.stereo_batch(0, 4, 128, 192))
    enc = net.compress_batch(x1, x2, Hm)
    for i in range(4):
        alone = net.compress_batch(x1[i:i + 1], x2[i:i + 1], Hm[i:i + 1])
        assert alone["blobs"][0] == enc["blobs"][i], i
    dec = net.decompress_batch(enc["blobs"], Hm)
    # another grouping and order, with the matching homographies
    sub = net.decompress_batch([enc["blobs"][2], enc["blobs"][0]], Hm[[2, 0]])
    for k in ("y1_hat", "y2_hat", "x1_hat", "x2_hat"):
        assert _same(sub[k], dec[k][[2, 0]]), k
    one = net.decompress_batch(enc["blobs"][3:], Hm[3:])
    for k in ("x1_hat", "x2_hat"):
        assert _same(one[k], dec[k][3:]), k


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_real_size_against_the_estimate(dtype):
    """The bar of test_gpu_compress_decompress_round_trip (y likelihoods floored at 2^-16, z unfloored, 3 % + 0.02 bpp) plus the DERIVED
    worst case of what a stream adds: 2 flush bytes and a 3-byte length varint each."""
    net = _net(dtype)
    Bn, Hh, Ww = 2, 256, 256
    x1, x2, Hm = (t.cuda() for t in synthetic.stereo_batch(3, Bn, Hh, Ww))
    with torch.no_grad():
        fwd = net(x1, x2, Hm)
    L = fwd["likelihoods"]
    enc1 = net.compress_batch(x1, x2, Hm, channels_per_stream=1)
    enc8 = net.compress_batch(x1, x2, Hm, channels_per_stream=8)
    pixels = 2 * Hh * Ww
    for i in range(Bn):
        est = sum(float(-torch.log2(L[k][i].float().clamp_min(2.0 ** -16)).sum()) for k in ("y1", "y2"))
        est += sum(float(-torch.log2(L[k][i].float()).sum()) for k in ("z1", "z2"))
        est /= pixels
        for enc in (enc1, enc8):
            p = bitstream.parse_pair(enc["blobs"][i])
            n_streams = sum(len(v["streams"]) for v in p["views"])
            overhead = n_streams * (2 + 3) * 8 / pixels
            real = enc["bpp_real"][i]
            print(f"pair {i} cps {p['channels_per_stream']}: bpp_real {real:.5f} est {est:.5f} streams {n_streams} overhead bound {overhead:.5f}")
            assert real == len(enc["blobs"][i]) * 8 / pixels
            assert abs(real - est) < 0.03 * est + 0.02 + overhead, (i, real, est, overhead)
        assert len(enc8["blobs"][i]) < len(enc1["blobs"][i])
    d1, d8 = net.decompress_batch(enc1["blobs"], Hm), net.decompress_batch(enc8["blobs"], Hm)
    for k in ("y1_hat", "y2_hat", "x1_hat", "x2_hat"):
        assert _same(d1[k], d8[k]) and _same(d1[k], fwd[k]), k


@pytest.mark.parametrize("dtype", [torch.float16, torch.float32], ids=["f16", "f32"])
def test_batch_and_per_pair_paths_agree(tmp_path, dtype):
    """One pair through HSIC.compress (files) and compress_batch: the same minmax, flags, z strings and latents."""
    net = _net(dtype)
    x1, x2, Hm = (t.cuda() for t in synthetic.stereo_batch(3, 1, 128, 192))
    old = net.compress(x1, x2, Hm, "pair", str(tmp_path))
    new = net.compress_batch(x1, x2, Hm)
    head = (tmp_path / "pair.npz").read_bytes()
    assert np.frombuffer(head[:4], np.uint16).tolist() == [128, 192]
    p = bitstream.parse_pair(new["blobs"][0])
    assert (p["height"], p["width"], p["channels"]) == (128, 192, net.M)
    pos = 4
    for v in p["views"]:
        length, minmax = (int(t) for t in np.frombuffer(head[pos:pos + 4], np.uint16))
        pos += 4
        flags = np.unpackbits(np.frombuffer(head[pos:pos + net.M // 8], np.uint8))[:net.M]
        pos += net.M // 8
        z = head[pos:pos + length]
        pos += length
        assert v["minmax"] == minmax and list(v["flags"]) == flags.tolist() and v["z"] == z
    assert pos == len(head)
    for k in ("y1_hat", "y2_hat", "z1_hat", "z2_hat"):
        assert _same(old[k], new[k]), k
    dec_old = net.decompress(None, None, Hm, "pair", str(tmp_path))
    dec_new = net.decompress_batch(new["blobs"], Hm)
    for k in ("y1_hat", "y2_hat", "x1_hat", "x2_hat"):
        assert _same(dec_old[k], dec_new[k]), k


def test_refusals_happen_on_the_host():
    from hesic_amd import models
    net = _net(torch.float16)
    x1, x2, Hm = (t.cuda() for t in synthetic.stereo_batch(3, 1, 64, 64))
    enc = net.compress_batch(x1, x2, Hm)
    launched = []
    with hesic_amd._lib.call_hook(lambda name, args: launched.append(name)):
        # an alphabet above 1024 symbols: at the wrappers, and in a blob's header
        sc, mu, w, y, channels = _case(torch.float16, MINMAX_CASES[6])
        with pytest.raises(ValueError, match="1024.*HSIC.compress"):
            Fn.gmm_rc_encode(sc, mu, w, y, [6, 512, 1], channels, K)
        with pytest.raises(ValueError, match="1024.*HSIC.compress"):
            Fn.gmm_rc_decode(sc, mu, w, [6, 512, 1], channels, K, torch.zeros(8, dtype=torch.uint8, device=DEV), torch.zeros(B, M, dtype=torch.int32), None, 1)
        p = bitstream.parse_pair(enc["blobs"][0])
        p["views"][1]["minmax"] = 600
        with pytest.raises(ValueError, match="1024.*HSIC.compress"):
            net.decompress_batch([bitstream.pack_pair(p)], Hm)
        # mixed sizes in one call
        x1b, x2b, Hmb = (t.cuda() for t in synthetic.stereo_batch(3, 1, 64, 128))
    other = net.compress_batch(x1b, x2b, Hmb)
    with hesic_amd._lib.call_hook(lambda name, args: launched.append(name)):
        with pytest.raises(ValueError, match="same size"):
            net.decompress_batch([enc["blobs"][0], other["blobs"][0]], torch.cat([Hm, Hmb]))
        # a damaged blob
        bad = bytearray(enc["blobs"][0])
        bad[-9] ^= 1
        with pytest.raises(ValueError, match="CRC"):
            net.decompress_batch([bytes(bad)], Hm)
        # a decoder in another mode: the text of the .bin payload's check
        hesic_amd.set_compute_dtype(torch.bfloat16)
        with pytest.raises(ValueError, match="float16 maps.*bfloat16 maps"):
            net.decompress_batch(enc["blobs"], Hm)
        hesic_amd.set_compute_dtype(torch.float16)
    assert launched == [], launched
    dec = net.decompress_batch(enc["blobs"], Hm)          # and back in the writer's mode it decodes
    assert _same(dec["y2_hat"], enc["y2_hat"])
    assert models.payload_mode_bytes() == enc["blobs"][0][4:6]


def test_b8_512_round_trip_smoke():
    """3072 streams per view pair (B = 8, 512 x 512, float16: the benchmark's configuration): decode equals encode."""
    net = _net(torch.float16)
    x1, x2, Hm = (t.cuda() for t in synthetic.stereo_batch(0, 8, 512, 512))
    t0 = time.time()
    enc = net.compress_batch(x1, x2, Hm)
    torch.cuda.synchronize()
    t1 = time.time()
    dec = net.decompress_batch(enc["blobs"], Hm)
    torch.cuda.synchronize()
    print(f"B=8 512x512 f16 (cold): compress_batch {t1 - t0:.3f} s, decompress_batch {time.time() - t1:.3f} s, mean bpp {np.mean(enc['bpp_real']):.4f}")
    for k in ("y1_hat", "y2_hat", "z1_hat", "z2_hat"):
        assert _same(dec[k], enc[k]), k
    with torch.no_grad():
        fwd = net(x1, x2, Hm)
    for k in ("x1_hat", "x2_hat"):
        assert _same(dec[k], fwd[k]), k


def test_cli_encode_decode_folder(tmp_path, capsys):
    """``python -m hesic_amd.codec`` on a stereo folder of three synthetic pairs of two sizes (one of them not a multiple of 64): the
    PNGs equal the quantised ``decompress_batch`` output of the same blobs, cropped to the image size."""
    import json
    from PIL import Image
    from hesic_amd import codec, models
    root, out, recon = tmp_path / "data", tmp_path / "out", tmp_path / "recon"
    for sub in ("left", "right", "H"):
        (root / "test" / sub).mkdir(parents=True)
    sizes = {"a": (64, 128), "b": (100, 120), "c": (64, 128)}
    for i, (stem, (h, w)) in enumerate(sizes.items()):
        x1, x2, Hm = synthetic.stereo_batch(20 + i, 1, 128, 128)
        for side, x in (("left", x1), ("right", x2)):
            Image.fromarray((x[0, :, :h, :w].clamp(0, 1) * 255).round().to(torch.uint8).permute(1, 2, 0).numpy()).save(root / "test" / side / (stem + ".png"))
        np.save(root / "test" / "H" / (stem + ".npy"), Hm[0].double().numpy())
    # a pair without a sidecar is skipped and counted
    for side in ("left", "right"):
        Image.fromarray(np.zeros((64, 64, 3), np.uint8)).save(root / "test" / side / "d.png")
    assert codec.main(["encode", str(root), str(out), "--batch", "2"]) == 0
    line = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert line["pairs"] == 3 and line["skipped_no_sidecar"] == 1 and line["mean_bpp"] > 0 and line["pairs_per_s"] > 0
    assert sorted(f.name for f in out.glob("*.hsd")) == ["a.hsd", "b.hsd", "c.hsd"]
    assert codec.main(["decode", str(out), str(recon), "--batch", "2"]) == 0
    assert json.loads(capsys.readouterr().out.strip().splitlines()[-1])["pairs"] == 3
    net = codec.load_model(None, torch.float16)
    for stem, (h, w) in sizes.items():
        blob = (out / (stem + ".hsd")).read_bytes()
        p = bitstream.parse_pair(blob)
        assert (p["height"], p["width"]) == ((h + 63) // 64 * 64, (w + 63) // 64 * 64)
        Hm = torch.from_numpy(np.load(root / "test" / "H" / (stem + ".npy"))).float().reshape(1, 3, 3).cuda()
        dec = net.decompress_batch([blob], Hm)
        for side, k in (("left", "x1_hat"), ("right", "x2_hat")):
            png = np.array(Image.open(recon / f"{stem}_{side}.png"))
            assert png.shape == (h, w, 3)
            assert np.array_equal(png, codec.quantise(dec[k])[0, :h, :w]), (stem, side)
    assert models.payload_mode_bytes()[0] & 3 == 2

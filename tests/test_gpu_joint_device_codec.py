"""Batched HESIC+ bit-stream on the device (HSICJoint.compress_batch / decompress_batch; csrc/codec.hip: ordered encoder, batched group
gather, step decoder).

Kernel level: the ordered encoder's bytes against the host ``RangeEncoder`` over ``Fn.gmm_cdf_tables`` rows in the order of
``joint_stream_ref``; the step decoder, driven group by group over given (scale, mean) maps, against the latents; the gather against
plain indexing.  Model level: what the per-pair ``compress`` / ``decompress`` (the trusted path) gives for every pair of the batch."""
import time

import numpy as np
import pytest
import torch

import joint_stream_ref as J
import memguard as MG
import hesic_amd
from hesic_amd import _host, bitstream, synthetic
from hesic_amd import functional as Fn

pytestmark = pytest.mark.gpu
DEV = "cuda"
CL = torch.channels_last
M, B, H, W = 192, 3, 16, 20
DTYPES = [torch.float32, torch.bfloat16, torch.float16]
IDS = ["f32", "bf16", "f16"]
MINMAX_CASES = {1: [1, 6, 1], 6: [6, 40, 1], 40: [40, 6, 3], 511: [511, 1, 40]}


def _case(dtype, minmax, seed=0):
    """``test_gpu_device_codec._case`` for K = 1 without weights: one Gaussian per latent in ``dtype`` storage, latents inside each
    image's alphabet, per-image channel lists (all / every other / a random 150)."""
    hesic_amd.set_compute_dtype(dtype)
    g = torch.Generator().manual_seed(2000 + seed)
    sc = (torch.rand(B, M, H, W, generator=g) * 2.98 + 0.02).to(dtype).to(DEV).contiguous(memory_format=CL)
    mu = (torch.rand(B, M, H, W, generator=g) * 12 - 6).to(dtype).to(DEV).contiguous(memory_format=CL)
    channels = [list(range(M)), list(range(0, M, 2)), sorted(torch.randperm(M, generator=g)[:150].tolist())]
    ydt = dtype if max(minmax) <= 256 else torch.float32
    y = torch.zeros(B, M, H, W)
    for b in range(B):
        mm = minmax[b]
        near = torch.round(torch.randn(len(channels[b]), H, W, generator=g) * 2).clamp(-mm, mm)
        far = torch.randint(-mm, mm + 1, near.shape, generator=g).float()
        v = torch.where(torch.rand(near.shape, generator=g) < 0.1, far, near)
        v[0, 0, 0], v[-1, -1, -1] = -mm, mm
        y[b, channels[b]] = v
    return sc, mu, y.to(ydt).to(DEV).contiguous(memory_format=CL), channels


def _walk(Hh=H, Ww=W):
    """(coding order, padded-map row of every pixel in coding order) as int32 device tensors, and the group sizes."""
    groups = J.wavefront_groups(Hh, Ww)
    order = np.concatenate(groups)
    centre = (order // Ww + 2) * (Ww + 4) + order % Ww + 2
    return (torch.from_numpy(order.astype(np.int32)).to(DEV), torch.from_numpy(centre.astype(np.int32)).to(DEV), [len(g) for g in groups])


def _host_streams(sc, mu, y, channels, minmax, cps):
    """{(b, s): (host bytes with the 8-byte flush, symbols, table rows)} in the order of joint_stream_ref."""
    out = {}
    for b in range(B):
        tab = Fn.gmm_cdf_tables(sc, mu, None, channels[b], minmax[b], 1, b=b).cpu().numpy().view(np.uint32)
        tab = tab.reshape(len(channels[b]), H * W, -1)
        sym = (y[b, channels[b]].float().cpu().numpy().astype(np.int64) + minmax[b]).astype(np.int32).reshape(len(channels[b]), H * W)
        for s, e in enumerate(J.stream_elements(H, W, len(channels[b]), cps)):
            sy, tb = np.ascontiguousarray(sym[e[:, 0], e[:, 1]]), np.ascontiguousarray(tab[e[:, 0], e[:, 1]])
            enc = _host.RangeEncoder()
            enc.encode(sy, tb)
            out[b, s] = (enc.finish(), sy, tb)
    return out


def _split(data, counts, channels, cps):
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


ENC_CASES = [(torch.float32, 6, 1), (torch.float32, 6, 8), (torch.bfloat16, 40, 1), (torch.float16, 40, 8), (torch.float16, 1, M),
             (torch.float32, 511, 8)]


@pytest.mark.parametrize("dtype,mm,cps", ENC_CASES, ids=[f"{IDS[DTYPES.index(d)]}-mm{m}-cps{c}" for d, m, c in ENC_CASES])
def test_ordered_encoder_equals_the_host_encoder(dtype, mm, cps):
    minmax = MINMAX_CASES[mm]
    sc, mu, y, channels = _case(dtype, minmax, seed=cps)
    order, _centre, _sizes = _walk()
    data, counts = Fn.gmm_rc_encode(sc, mu, None, y, minmax, channels, 1, cps, order=order)
    assert counts.shape == (B, (M + cps - 1) // cps) and data.dtype == torch.uint8
    dev = _split(data, counts, channels, cps)
    host = _host_streams(sc, mu, y, channels, minmax, cps)
    assert dev.keys() == host.keys()
    for key, (hb, sy, tb) in host.items():
        d, body = dev[key], hb[:-8]
        assert d[:len(body)] == body, key
        assert len(body) <= len(d) <= len(body) + 2, (key, len(d), len(body))
        assert np.array_equal(_host.RangeDecoder(d).decode(tb), sy), key
    # the HESIC stream of the same inputs is another stream (the order matters) unless a stream holds one pixel's worth
    plain, _ = Fn.gmm_rc_encode(sc, mu, None, y, minmax, channels, 1, cps)
    assert not torch.equal(plain, data)
    gs = [MG.guarded(t, name=f"input {i}") for i, t in enumerate((sc, mu, y))]
    gorder = MG.guarded(order, name="order")
    with MG.poisoned_allocations([Fn]):
        data_g, counts_g = Fn.gmm_rc_encode(gs[0], gs[1], None, gs[2], minmax, channels, 1, cps, order=gorder)
    MG.check_all(gs + [gorder])
    assert torch.equal(data_g, data) and torch.equal(counts_g, counts)
    # a permutation entry outside the map is reported, not followed
    bad = order.clone()
    bad[7] = H * W
    with pytest.raises(RuntimeError, match="zero frequency"):
        Fn.gmm_rc_encode(sc, mu, None, y, minmax, channels, 1, cps, order=bad)


def _decode_by_steps(sc, mu, minmax, channels, data, counts, cps, ydt, guard=False):
    """The step decoder driven group by group over GIVEN (scale, mean) maps -> (B, M, H, W) latents; with ``guard`` every buffer sits
    between poisoned guards, which are checked."""
    order, centre, sizes = _walk()
    wrap = (lambda t, name: MG.guarded(t, name=name)) if guard else (lambda t, name: t)
    S = (M + cps - 1) // cps
    meta = wrap(Fn.rc_meta(minmax, channels, M, DEV), "meta")
    cnt = wrap(torch.as_tensor(counts, dtype=torch.int32, device=DEV).reshape(-1).contiguous(), "counts")
    offsets = wrap(torch.cumsum(cnt, 0, dtype=torch.int64) - cnt, "offsets")
    state = wrap(torch.full((B * S, 4), -1, dtype=torch.int64, device=DEV), "state")          # stale states: the first step begins them
    y_rows = wrap(torch.zeros(B, (H + 4) * (W + 4), M, dtype=ydt, device=DEV), "maps")
    data = wrap(data, "payload")
    centre = wrap(centre, "centre")
    sc_rows, mu_rows = (t.float().permute(0, 2, 3, 1).reshape(B, H * W, M) for t in (sc, mu))
    off, held = 0, [meta, cnt, offsets, state, y_rows, data, centre]
    for P in sizes:
        pix = order[off:off + P].long()
        sm = wrap(torch.cat([sc_rows[:, pix], mu_rows[:, pix]], 2).reshape(B * P, 2 * M).contiguous(), "sm")
        Fn.gmm_rc_decode_step(sm, B, P, M, meta, cps, data, offsets, cnt, state, off == 0, centre, off, y_rows)
        held.append(sm)
        off += P
    if guard:
        MG.check_all(held)
    full = y_rows.view(B, H + 4, W + 4, M)
    border = full.clone()
    border[:, 2:-2, 2:-2] = 0
    assert int((border != 0).sum()) == 0                      # nothing lands in the padding
    return full[:, 2:-2, 2:-2].permute(0, 3, 1, 2)


DEC_CASES = [(torch.float32, 6, 1), (torch.bfloat16, 40, 8), (torch.float16, 6, 8), (torch.float16, 1, 1), (torch.float16, 40, M),
             (torch.float32, 511, 8)]


@pytest.mark.parametrize("dtype,mm,cps", DEC_CASES, ids=[f"{IDS[DTYPES.index(d)]}-mm{m}-cps{c}" for d, m, c in DEC_CASES])
def test_step_decoder(dtype, mm, cps):
    minmax = MINMAX_CASES[mm]
    sc, mu, y, channels = _case(dtype, minmax, seed=10 + cps)
    order, _c, _s = _walk()
    data, counts = Fn.gmm_rc_encode(sc, mu, None, y, minmax, channels, 1, cps, order=order)
    back = _decode_by_steps(sc, mu, minmax, channels, data, counts, cps, y.dtype)
    assert back.dtype == y.dtype and torch.equal(back, y)
    for b in range(B):
        off = sorted(set(range(M)) - set(channels[b]))
        if off:
            assert int((back[b, off] != 0).sum()) == 0
    # host-coded streams of the same symbols (8-byte termination)
    host = _host_streams(sc, mu, y, channels, minmax, cps)
    S = (M + cps - 1) // cps
    hcounts = [[len(host[b, s][0]) if (b, s) in host else 0 for s in range(S)] for b in range(B)]
    hdata = torch.frombuffer(bytearray(b"".join(host[b, s][0] for b in range(B) for s in range(S) if (b, s) in host)), dtype=torch.uint8).to(DEV)
    assert torch.equal(_decode_by_steps(sc, mu, minmax, channels, hdata, hcounts, cps, y.dtype), y)
    # every buffer between poisoned guards: the payload ends flush against its trailing guard
    for payload, cnt in ((data, counts), (hdata, hcounts)):
        assert torch.equal(_decode_by_steps(sc, mu, minmax, channels, payload, cnt, cps, y.dtype, guard=True), y)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("view", [1, 2])
def test_batched_gather_equals_indexing(dtype, view):
    hesic_amd.set_compute_dtype(dtype)
    Bn, c_par, c_ctx = 4, 2 * M, 2 * M
    c_feat = c_par + c_ctx + (M if view == 2 else 0)
    order, centre, sizes = _walk()
    Wp, rows = W + 4, (H + 4) * (W + 4)
    g = torch.Generator().manual_seed(7)
    y_rows = MG.guarded(torch.randint(-9, 10, (Bn, rows, M), generator=g).to(dtype).to(DEV), name="maps")
    par = MG.guarded(torch.randn(Bn, H * W, c_par, generator=g).to(dtype).to(DEV), name="par")
    ext = MG.guarded(torch.randn(Bn, H * W, M, generator=g).to(dtype).to(DEV), name="ext") if view == 2 else None
    pmax = max(sizes)
    win = torch.tensor([(t // 5 - 2) * Wp + (t % 5 - 2) for t in range(25)], device=DEV)
    off = 0
    for P in sizes:
        if P in (1, 2, pmax) or off % 7 == 0:
            crops = MG.guarded(torch.full((Bn * pmax, 5, 5, M), 77.0, dtype=dtype, device=DEV), name="crops")
            feat = MG.guarded(torch.full((Bn * pmax, c_feat), 77.0, dtype=dtype, device=DEV), name="feat")
            Fn.joint_gather_batch(y_rows, Wp, centre, order, off, P, crops, par, ext, c_par + c_ctx, feat)
            MG.check_all([y_rows, par, ext, crops, feat])
            src = centre[off:off + P].long()[:, None] + win[None, :]                                  # (P, 25)
            assert torch.equal(crops[:Bn * P].reshape(Bn, P, 25, M), y_rows[:, src])
            pix = order[off:off + P].long()
            f = feat[:Bn * P].reshape(Bn, P, c_feat)
            assert torch.equal(f[..., :c_par], par[:, pix])
            assert bool((f[..., c_par:c_par + c_ctx] == 77.0).all())                                  # the masked conv's slice is not touched
            if view == 2:
                assert torch.equal(f[..., c_par + c_ctx:], ext[:, pix])
            assert bool((crops[Bn * P:] == 77.0).all()) and bool((feat[Bn * P:] == 77.0).all())      # nor the rows of other groups
        off += P


def test_gather_reads_rows_outside_the_map_as_zeros():
    """Forged index tables: a centre whose 5 x 5 window leaves the padded map on either side, raster rows outside [0, HW) -- the
    documented "reads as zeros", under guards; and the wrapper refuses buffers of another shape or dtype."""
    hesic_amd.set_compute_dtype(torch.float16)
    Bn, c_par = 2, 2 * M
    c_feat = c_par + 2 * M + M
    order, centre, _sizes = _walk()
    Wp, rows = W + 4, (H + 4) * (W + 4)
    g = torch.Generator().manual_seed(11)
    y_rows = MG.guarded((torch.randint(-9, 10, (Bn, rows, M), generator=g).float() + 0.5).half().to(DEV), name="maps")
    par = MG.guarded((torch.rand(Bn, H * W, c_par, generator=g) + 1).half().to(DEV), name="par")
    ext = MG.guarded((torch.rand(Bn, H * W, M, generator=g) + 1).half().to(DEV), name="ext")
    bad_c, bad_r = centre.clone(), order.clone()
    bad_c[0], bad_c[1], bad_c[2] = 0, rows - 1, -7            # window above the map, below it, a negative row
    bad_r[0], bad_r[1] = H * W, -1
    bad_c, bad_r = MG.guarded(bad_c, name="centre"), MG.guarded(bad_r, name="rows")
    P = 4
    crops = MG.guarded(torch.full((Bn * P, 5, 5, M), 77.0, dtype=torch.float16, device=DEV), name="crops")
    feat = MG.guarded(torch.full((Bn * P, c_feat), 77.0, dtype=torch.float16, device=DEV), name="feat")
    Fn.joint_gather_batch(y_rows, Wp, bad_c, bad_r, 0, P, crops, par, ext, c_par + 2 * M, feat)
    MG.check_all([y_rows, par, ext, bad_c, bad_r, crops, feat])
    win = torch.tensor([(t // 5 - 2) * Wp + (t % 5 - 2) for t in range(25)], device=DEV)
    src = bad_c[:P].long()[:, None] + win[None, :]
    inside = (src >= 0) & (src < rows)
    want = torch.where(inside[None, :, :, None], y_rows[:, src.clamp(0, rows - 1)], torch.zeros((), dtype=torch.float16, device=DEV))
    assert not bool(inside[:3].all()) and bool(inside[3].all()) and int(inside[0].sum()) > 0
    assert torch.equal(crops.reshape(Bn, P, 25, M), want)
    f = feat.reshape(Bn, P, c_feat)
    assert bool((f[:, :2, :c_par] == 0).all()) and bool((f[:, :2, c_par + 2 * M:] == 0).all())
    pix = bad_r[2:P].long()
    assert torch.equal(f[:, 2:, :c_par], par[:, pix]) and torch.equal(f[:, 2:, c_par + 2 * M:], ext[:, pix])
    for kw in (dict(crops=crops.reshape(Bn * P * 5, 5, M)), dict(crops=crops.float()), dict(ext=ext[:, :-1]), dict(feat=feat.float()),
               dict(par=par[:1]), dict(centre=bad_c.long())):
        a = dict(crops=crops, par=par, ext=ext, feat=feat, centre=bad_c)
        a.update(kw)
        with pytest.raises(ValueError, match="joint_gather_batch"):
            Fn.joint_gather_batch(y_rows, Wp, a["centre"], bad_r, 0, P, a["crops"], a["par"], a["ext"], c_par + 2 * M, a["feat"])


# ---------------------------------------------------------------------------------------------------------------- model
def _net(dtype, cls="HSICJoint"):
    from hesic_amd import models
    hesic_amd.set_compute_dtype(dtype)
    net = getattr(models, cls)()
    synthetic.fill_state_dict_(net.state_dict())
    net = net.cuda().eval()
    net.update(force=True)
    return net


def _same(a, b):
    return torch.equal(a.float().cpu(), b.float().cpu())


def _minmax_ok(blobs):
    for bl in blobs:
        p = bitstream.parse_pair(bl)
        assert bitstream.kind_of(p) == "joint"
        assert all(v["minmax"] <= 511 for v in p["views"]), [v["minmax"] for v in p["views"]]


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("shape", [(3, 128, 192), (2, 256, 320), (1, 128, 192)], ids=["b3-128x192", "b2-256x320", "b1-128x192"])
def test_model_round_trip_equals_the_per_pair_path(tmp_path, dtype, shape):
    net = _net(dtype)
    x1, x2, Hm = (t.cuda() for t in synthetic.stereo_batch(3, *shape))
    enc = net.compress_batch(x1, x2, Hm)
    assert len(enc["blobs"]) == shape[0] == len(enc["bpp_real"]) and all(isinstance(b, bytes) for b in enc["blobs"])
    _minmax_ok(enc["blobs"])
    dec = net.decompress_batch(enc["blobs"], Hm)
    for k in ("y1_hat", "y2_hat", "z1_hat", "z2_hat"):
        assert dec[k].shape == enc[k].shape and _same(dec[k], enc[k]), k
    for i in range(shape[0]):
        old = net.compress(x1[i:i + 1], x2[i:i + 1], Hm[i:i + 1], f"pair{i}", str(tmp_path))
        ref = net.decompress(None, None, Hm[i:i + 1], f"pair{i}", str(tmp_path))
        for k in ("y1_hat", "y2_hat"):
            assert _same(old[k], enc[k][i:i + 1]), (i, k)
        for k in ("x1_hat", "x2_hat", "y1_hat", "y2_hat"):
            assert _same(dec[k][i:i + 1], ref[k]), (i, k)
    if shape[0] == 1:
        with torch.no_grad(), Fn.no_split_k():
            fwd = net(x1, x2, Hm)
        for k in ("y1_hat", "x1_hat", "x2_hat"):
            assert _same(dec[k], fwd[k]), k


@pytest.mark.parametrize("dtype", [torch.float16, torch.float32], ids=["f16", "f32"])
def test_batch_and_per_pair_paths_agree(tmp_path, dtype):
    from hesic_amd import models
    net = _net(dtype)
    x1, x2, Hm = (t.cuda() for t in synthetic.stereo_batch(3, 1, 128, 192))
    old = net.compress(x1, x2, Hm, "pair", str(tmp_path), order="wavefront")
    new = net.compress_batch(x1, x2, Hm)
    head = (tmp_path / "pair.npz").read_bytes()
    assert np.frombuffer(head[:4], np.uint16).tolist() == [128, 192]
    p = bitstream.parse_pair(new["blobs"][0])
    assert (bitstream.kind_of(p), p["height"], p["width"], p["channels"]) == ("joint", 128, 192, net.M)
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
    # cps = M: view 1 is one stream, the symbol sequence the per-pair coder starts with; this coder has no carry propagation, so the
    # bytes it emitted before view 2 entered are final, and the short flush is 0 - 2 bytes
    one = bitstream.parse_pair(net.compress_batch(x1, x2, Hm, channels_per_stream=net.M)["blobs"][0])
    assert len(one["views"][0]["streams"]) == 1
    s1 = one["views"][0]["streams"][0]
    payload = (tmp_path / "pair.bin").read_bytes()
    _extra, off = models.check_payload(payload, 1)
    assert len(s1) > 100 and payload[off:off + len(s1) - 2] == s1[:-2]


@pytest.mark.parametrize("dtype", [torch.float16, torch.float32], ids=["f16", "f32"])
def test_pairs_are_independent_of_the_batch(dtype):
    """The decoder derives a pixel's (scale, mean) from B * P crops, the encoder from the whole maps of the batch: the stream only
    decodes, and a pair only codes to the same bytes in any batch, if the two agree bit for bit for every B and P."""
    net = _net(dtype)
    x1, x2, Hm = (t.cuda() for t in synthetic.stereo_batch(0, 4, 128, 192))
    enc = net.compress_batch(x1, x2, Hm)
    _minmax_ok(enc["blobs"])
    for i in range(4):
        alone = net.compress_batch(x1[i:i + 1], x2[i:i + 1], Hm[i:i + 1])
        assert alone["blobs"][0] == enc["blobs"][i], i
    dec = net.decompress_batch(enc["blobs"], Hm)
    for k in ("y1_hat", "y2_hat"):
        assert _same(dec[k], enc[k]), k
    sub = net.decompress_batch([enc["blobs"][2], enc["blobs"][0]], Hm[[2, 0]])
    for k in ("y1_hat", "y2_hat", "x1_hat", "x2_hat"):
        assert _same(sub[k], dec[k][[2, 0]]), k
    one = net.decompress_batch(enc["blobs"][3:], Hm[3:])
    for k in ("y1_hat", "y2_hat", "x1_hat", "x2_hat"):
        assert _same(one[k], dec[k][3:]), k


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_real_size_against_the_estimate(dtype):
    """The bar the project uses for HESIC+ (0.15 est + 0.05: the forward prices round(y - mu) + mu, the stream codes round(y)) plus the
    derived worst case of what a stream adds: 2 flush bytes and a 3-byte length varint each."""
    net = _net(dtype)
    Bn, Hh, Ww = 2, 128, 192
    x1, x2, Hm = (t.cuda() for t in synthetic.stereo_batch(3, Bn, Hh, Ww))
    with torch.no_grad(), Fn.no_split_k():
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
            assert abs(real - est) < 0.15 * est + 0.05 + overhead, (i, real, est, overhead)
        assert len(enc8["blobs"][i]) < len(enc1["blobs"][i])
    d1, d8 = net.decompress_batch(enc1["blobs"], Hm), net.decompress_batch(enc8["blobs"], Hm)
    for k in ("y1_hat", "y2_hat", "x1_hat", "x2_hat"):
        assert _same(d1[k], d8[k]), k
    assert _same(d1["y1_hat"], enc1["y1_hat"]) and _same(d1["y2_hat"], enc1["y2_hat"])


def test_a_cached_walk_is_refilled():
    """A second decode of the same blobs (cached graph), and one with another B and other pairs in between: identical results."""
    net = _net(torch.float16)
    x1, x2, Hm = (t.cuda() for t in synthetic.stereo_batch(7, 3, 128, 192))
    enc = net.compress_batch(x1, x2, Hm)
    first = net.decompress_batch(enc["blobs"], Hm)
    first = {k: v.clone() for k, v in first.items()}
    again = net.decompress_batch(enc["blobs"], Hm)
    y1, y2, Hn = (t.cuda() for t in synthetic.stereo_batch(0, 2, 128, 192))
    other = net.compress_batch(y1, y2, Hn)
    between = net.decompress_batch(other["blobs"], Hn)
    assert _same(between["y2_hat"], other["y2_hat"])
    swapped = net.decompress_batch(enc["blobs"][::-1], Hm.flip(0))            # the same B: the same graph and buffers, other contents
    third = net.decompress_batch(enc["blobs"], Hm)
    for k in ("y1_hat", "y2_hat", "x1_hat", "x2_hat", "z1_hat", "z2_hat"):
        assert _same(first[k], again[k]) and _same(first[k], third[k]), k
        assert _same(swapped[k], first[k].flip(0)), k
    assert _same(first["y1_hat"], enc["y1_hat"]) and _same(first["y2_hat"], enc["y2_hat"])
    assert len(net._bw_cache) == 4 and all(st["graph"] is not None for st in net._bw_cache.values())


def test_refusals_happen_on_the_host():
    net, hesic = _net(torch.float16), _net(torch.float16, "HSIC")
    x1, x2, Hm = (t.cuda() for t in synthetic.stereo_batch(3, 1, 64, 64))
    enc = net.compress_batch(x1, x2, Hm)
    enc_h = hesic.compress_batch(x1, x2, Hm)
    launched = []
    with hesic_amd._lib.call_hook(lambda name, args: launched.append(name)):
        p = bitstream.parse_pair(enc["blobs"][0])
        p["views"][1]["minmax"] = 600
        with pytest.raises(ValueError, match="1024.*compress"):
            net.decompress_batch([bitstream.pack_pair(p)], Hm)
        with pytest.raises(ValueError, match="HSJ.*HSD"):
            net.decompress_batch(enc_h["blobs"], Hm)
        with pytest.raises(ValueError, match="HSD.*HSJ"):
            hesic.decompress_batch(enc["blobs"], Hm)
        bad = bytearray(enc["blobs"][0])
        bad[-9] ^= 1
        with pytest.raises(ValueError, match="CRC"):
            net.decompress_batch([bytes(bad)], Hm)
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            net.decompress_batch(enc["blobs"], Hm.cpu())
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            net.compress_batch(x1.cpu(), x2.cpu(), Hm.cpu())
        with pytest.raises(ValueError, match="channels_per_stream"):
            net.compress_batch(x1, x2, Hm, channels_per_stream=0)
        hesic_amd.set_compute_dtype(torch.bfloat16)
        with pytest.raises(ValueError, match="float16 maps.*bfloat16 maps"):
            net.decompress_batch(enc["blobs"], Hm)
        hesic_amd.set_compute_dtype(torch.float16)
    assert launched == [], launched
    dec = net.decompress_batch(enc["blobs"], Hm)
    assert _same(dec["y2_hat"], enc["y2_hat"])


def test_a_damaged_payload_decodes_to_something_and_ends():
    """View 1's stream bytes cut in half, the container re-packed with a valid CRC; the payload buffer and the padded maps of the walk
    between poisoned guards.  Loop counts follow from the header and every byte read is index-checked (rc_decode_symbol, the
    clipping of [offset, offset + length) in rc_decode_step_kernel), so the call returns -- with latents inside the alphabet that are
    not the encoder's.  Runs once: it documents the bound, it does not search for a fault.  CPU counterpart:
    test_joint_codec_cpu.test_truncated_stream_decodes_to_the_end."""
    net = _net(torch.float16)
    x1, x2, Hm = (t.cuda() for t in synthetic.stereo_batch(3, 1, 128, 192))
    enc = net.compress_batch(x1, x2, Hm, channels_per_stream=8)
    p = bitstream.parse_pair(enc["blobs"][0])
    p["views"][0]["streams"] = [s[:len(s) // 2] for s in p["views"][0]["streams"]]
    blob = bitstream.pack_pair(p)
    assert bitstream.parse_pair(blob)["views"][0]["minmax"] == p["views"][0]["minmax"]
    guards = []
    for which in (1, 2):
        st = net._batch_walk_state(which, 8, 12, 1, 8, torch.device("cuda", torch.cuda.current_device()))
        assert st["graph"] is None
        st["data"] = MG.guarded(st["data"], name=f"payload {which}")
        st["y_pad"] = MG.guarded(st["y_pad"], name=f"maps {which}")
        st["y_rows"] = st["y_pad"].permute(0, 2, 3, 1).reshape(st["y_rows"].shape)
        assert st["y_rows"].data_ptr() == st["y_pad"].data_ptr()
        guards += [st["data"], st["y_pad"]]
    dec = net.decompress_batch([blob], Hm)
    torch.cuda.synchronize()
    MG.check_all(guards)
    mm = p["views"][0]["minmax"]
    assert bool(torch.isfinite(dec["y1_hat"].float()).all()) and float(dec["y1_hat"].abs().max()) <= mm
    assert not _same(dec["y1_hat"], enc["y1_hat"])
    assert bool(torch.isfinite(dec["x2_hat"].float()).all())


def test_b8_512_round_trip_smoke():
    """B = 8, 512 x 512, float16 (the benchmark's configuration): 125 groups of up to 11 pixels per view, 1536 streams per view."""
    net = _net(torch.float16)
    x1, x2, Hm = (t.cuda() for t in synthetic.stereo_batch(0, 8, 512, 512))
    t0 = time.time()
    enc = net.compress_batch(x1, x2, Hm)
    torch.cuda.synchronize()
    t1 = time.time()
    dec = net.decompress_batch(enc["blobs"], Hm)
    torch.cuda.synchronize()
    t2 = time.time()
    again = net.decompress_batch(enc["blobs"], Hm)
    torch.cuda.synchronize()
    print(f"B=8 512x512 f16: compress_batch (cold) {t1 - t0:.3f} s, decompress_batch cold {t2 - t1:.3f} s, warm {time.time() - t2:.3f} s, "
          f"mean bpp {np.mean(enc['bpp_real']):.4f}")
    _minmax_ok(enc["blobs"])
    for k in ("y1_hat", "y2_hat", "z1_hat", "z2_hat"):
        assert _same(dec[k], enc[k]), k
    for k in ("x1_hat", "x2_hat"):
        assert _same(dec[k], again[k]), k


def test_cli_encode_decode_folder_joint(tmp_path, capsys):
    """``python -m hesic_amd.codec encode|decode --model joint`` reproduces ``decompress_batch``; without ``--model joint`` the decoder
    refuses the blobs by their kind."""
    import json
    from PIL import Image
    from hesic_amd import codec
    root, out, recon = tmp_path / "data", tmp_path / "out", tmp_path / "recon"
    for sub in ("left", "right", "H"):
        (root / "test" / sub).mkdir(parents=True)
    sizes = {"a": (64, 128), "b": (100, 120), "c": (64, 128)}
    for i, (stem, (h, w)) in enumerate(sizes.items()):
        x1, x2, Hm = synthetic.stereo_batch(20 + i, 1, 128, 128)
        for side, x in (("left", x1), ("right", x2)):
            Image.fromarray((x[0, :, :h, :w].clamp(0, 1) * 255).round().to(torch.uint8).permute(1, 2, 0).numpy()).save(root / "test" / side / (stem + ".png"))
        np.save(root / "test" / "H" / (stem + ".npy"), Hm[0].double().numpy())
    assert codec.main(["encode", str(root), str(out), "--batch", "2", "--model", "joint"]) == 0
    line = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert line["pairs"] == 3 and line["mean_bpp"] > 0
    assert all((out / f"{s}.hsd").read_bytes()[:4] == b"HSJ\x01" for s in sizes)
    with pytest.raises(ValueError, match="HSD.*HSJ"):
        codec.main(["decode", str(out), str(recon)])
    capsys.readouterr()
    assert codec.main(["decode", str(out), str(recon), "--batch", "2", "--model", "joint"]) == 0
    assert json.loads(capsys.readouterr().out.strip().splitlines()[-1])["pairs"] == 3
    net = codec.load_model(None, torch.float16, model="joint")
    for stem, (h, w) in sizes.items():
        blob = (out / (stem + ".hsd")).read_bytes()
        Hm = torch.from_numpy(np.load(root / "test" / "H" / (stem + ".npy"))).float().reshape(1, 3, 3).cuda()
        dec = net.decompress_batch([blob], Hm)
        for side, k in (("left", "x1_hat"), ("right", "x2_hat")):
            png = np.array(Image.open(recon / f"{stem}_{side}.png"))
            assert png.shape == (h, w, 3)
            assert np.array_equal(png, codec.quantise(dec[k])[0, :h, :w]), (stem, side)

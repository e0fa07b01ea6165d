"""``compress_batch`` / ``decompress_batch(z_coder="device")`` of HSIC and HSICJoint against the ``"host"`` setting (the code path these
models had before the device rANS coder): the same blobs byte for byte, the same latents and reconstructions ``torch.equal``, and
either decoder setting reads either encoder's blobs.  A few bottleneck channels get narrowed quantiles first, so the z symbols hold
escapes as well as in-support symbols and the comparison cannot pass on a trivial path."""
import json

import numpy as np
import pytest
import torch

import hesic_amd
from hesic_amd import bitstream, synthetic

pytestmark = pytest.mark.gpu
DTYPES = [torch.float16, torch.bfloat16, torch.float32]
IDS = ["f16", "bf16", "f32"]
_NETS = {}


def _narrow(net):
    """Quantiles of the first bottleneck channels pulled in to a support of median + {-1, 0, 1} with a fractional median, tables rebuilt:
    16 channels around 0.3, and 16 around 10.3 -- the synthetic weights' z is small at 64 x 64, so those code escapes whatever z is."""
    with torch.no_grad():
        for eb in (net.entropy_bottleneck1, net.entropy_bottleneck2):
            eb.quantiles[:16, 0, 0], eb.quantiles[:16, 0, 1], eb.quantiles[:16, 0, 2] = 0.1, 0.3, 0.5
            eb.quantiles[16:32, 0, 0], eb.quantiles[16:32, 0, 1], eb.quantiles[16:32, 0, 2] = 10.1, 10.3, 10.5
    net.update(force=True)


def _net(dtype, cls):
    from hesic_amd import models
    hesic_amd.set_compute_dtype(dtype)
    key = (dtype, cls)
    if key not in _NETS:                       # one model per (dtype, class) for the module: building one costs more than a case
        net = getattr(models, cls)()
        synthetic.fill_state_dict_(net.state_dict())
        net = net.cuda().eval()
        net.update(force=True)
        _narrow(net)
        _NETS[key] = net
    return _NETS[key]


def _z_symbol_census(net, blobs, zs):
    """(escapes, in-support symbols) among the z symbols of the blobs, decoded by the host coder."""
    esc = inside = 0
    for vi, eb in enumerate((net.entropy_bottleneck1, net.entropy_bottleneck2)):
        strings = [bitstream.parse_pair(bl)["views"][vi]["z"] for bl in blobs]
        z_hat = eb.decompress(strings[:1], zs)
        for s_ in strings[1:]:
            z_hat = torch.cat([z_hat, eb.decompress([s_], zs)])
        v = torch.round(z_hat - eb._medians().detach().view(1, -1, 1, 1)).int() - eb._offset.view(1, -1, 1, 1)
        out = (v < 0) | (v >= eb._cdf_length.view(1, -1, 1, 1) - 2)
        esc, inside = esc + int(out.sum()), inside + int((~out).sum())
    return esc, inside


@pytest.mark.parametrize("shape", [(64, 64), (128, 192)], ids=["64x64", "128x192"])
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("cls", ["HSIC", "HSICJoint"])
def test_device_z_coder_equals_the_host_setting(cls, dtype, shape):
    net = _net(dtype, cls)
    x1, x2, Hm = (t.cuda() for t in synthetic.stereo_batch(3, 3, *shape))
    host = net.compress_batch(x1, x2, Hm, z_coder="host")
    dev = net.compress_batch(x1, x2, Hm, z_coder="device")
    assert dev["blobs"] == host["blobs"] and all(isinstance(b, bytes) for b in dev["blobs"])
    for k in ("z1_hat", "z2_hat", "y1_hat", "y2_hat"):
        assert dev[k].dtype == host[k].dtype and torch.equal(dev[k], host[k]), k
    esc, inside = _z_symbol_census(net, host["blobs"], (shape[0] // 64, shape[1] // 64))
    assert esc > 0 and inside > 0, (esc, inside)
    want = net.decompress_batch(host["blobs"], Hm, z_coder="host")
    for blobs in (host["blobs"], dev["blobs"]):
        got = net.decompress_batch(blobs, Hm, z_coder="device")
        assert set(got) == set(want)
        for k in want:
            assert got[k].dtype == want[k].dtype and torch.equal(got[k], want[k]), k
    for k in ("z1_hat", "z2_hat", "y1_hat", "y2_hat"):
        assert torch.equal(want[k], host[k]), k


def test_z_coder_argument_is_checked():
    net = _net(torch.float16, "HSIC")
    x1, x2, Hm = (t.cuda() for t in synthetic.stereo_batch(3, 1, 64, 64))
    with pytest.raises(ValueError, match="z_coder"):
        net.compress_batch(x1, x2, Hm, z_coder="gpu")
    blobs = net.compress_batch(x1, x2, Hm, z_coder="device")["blobs"]
    with pytest.raises(ValueError, match="z_coder"):
        net.decompress_batch(blobs, Hm, z_coder=None)
    # a z string that is not whole 32-bit words is refused on the host, before any launch
    p = bitstream.parse_pair(blobs[0])
    p["views"][0]["z"] = p["views"][0]["z"][:-2]
    with pytest.raises(ValueError, match="z string of pair 0, view 1"):
        net.decompress_batch([bitstream.pack_pair(p)], Hm, z_coder="device")


def test_cli_z_coder_device_reproduces_the_host_files(tmp_path, capsys):
    """``codec encode --z-coder device`` + ``decode --z-coder device`` on a two-pair folder: the .hsd files and the reconstructed PNGs of
    the host setting."""
    from PIL import Image
    from hesic_amd import codec
    root = tmp_path / "data"
    for sub in ("left", "right", "H"):
        (root / "test" / sub).mkdir(parents=True)
    for i, stem in enumerate(("a", "b")):
        x1, x2, Hm = synthetic.stereo_batch(20 + i, 1, 128, 128)
        for side, x in (("left", x1), ("right", x2)):
            Image.fromarray((x[0, :, :100, :120].clamp(0, 1) * 255).round().to(torch.uint8).permute(1, 2, 0).numpy()).save(
                root / "test" / side / (stem + ".png"))
        np.save(root / "test" / "H" / (stem + ".npy"), Hm[0].double().numpy())
    files = {}
    for z in ("host", "device"):
        out, recon = tmp_path / f"out_{z}", tmp_path / f"recon_{z}"
        assert codec.main(["encode", str(root), str(out), "--batch", "2", "--z-coder", z]) == 0
        assert json.loads(capsys.readouterr().out.strip().splitlines()[-1])["pairs"] == 2
        assert codec.main(["decode", str(out), str(recon), "--batch", "2", "--z-coder", z]) == 0
        assert json.loads(capsys.readouterr().out.strip().splitlines()[-1])["pairs"] == 2
        files[z] = {f.name: f.read_bytes() for d in (out, recon) for f in sorted(d.iterdir())}
    assert set(files["host"]) == set(files["device"]) and len(files["host"]) == 2 * 2 + 2 * 2
    for name, data in files["host"].items():
        if name.endswith(".png"):
            assert np.array_equal(np.array(Image.open(tmp_path / "recon_host" / name)), np.array(Image.open(tmp_path / "recon_device" / name))), name
        else:
            assert files["device"][name] == data, name

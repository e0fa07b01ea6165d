"""HomographyNet's inputs from device image pairs, the parts that need no GPU: the C ABI of include/hesic_homography_prep.h, the numpy
restatement the GPU test holds the kernel to (tests/homography_prep_ref.py) against the loader's host path, the window rule of
``homography.prepare_inputs`` against the loader's draws, and the checkpoint format of ``python -m hesic_amd.homography_train``."""
import ctypes as C
import random
import subprocess

import numpy as np
import pytest
import torch

import homography_prep_ref as R
from hesic_amd import _lib as L
from hesic_amd import homography
from hesic_amd.compressai.datasets import MEAN, STD


# ------------------------------------------------------------------------------------------------------------------------ ABI
@pytest.mark.parametrize("fmt", ["bf16", "f16"])
def test_abi_header_bindings_exports(fmt):
    declared = L.declared_symbols("hesic_homography_prep.h")
    assert declared == ["hesic_homonet_prepare"]
    assert set(declared) == set(L._HOMOGRAPHY_PREP_SIGS)
    assert not set(declared) & set(L.declared_symbols())                # a header of its own: include/hesic_hip.h does not list it
    text = open(L.header_path("hesic_homography_prep.h")).read()
    assert f"#define HESIC_PREP_U8 {L.PREP_U8} " in text and f"#define HESIC_PREP_F32 {L.PREP_F32} " in text
    assert "#define HESIC_ABI_VERSION 3" in open(L.header_path("hesic_hip.h")).read() and L.ABI_VERSION == 3
    exported = subprocess.check_output(["nm", "-D", "--defined-only", L.LIB_PATH_F16 if fmt == "f16" else L.LIB_PATH], text=True)
    for s in declared:
        assert f" T {s}\n" in exported, s


def _call_raw(lib, **kw):
    """hesic_homonet_prepare with host dummies for pointers: every case below is refused before anything is launched or dereferenced."""
    buf = (C.c_float * 16)()
    p = C.cast(buf, C.c_void_p)
    a = dict(x1=p, xs1=(C.c_int64 * 4)(1, 1, 1, 1), x2=p, xs2=(C.c_int64 * 4)(1, 1, 1, 1), xy=p, B=1, H=4, W=4, S=8, P=4, mean=0.5, std=0.25,
             dtype=L.PREP_U8, grey1=p, grey2=p, patch1=p, patch2=p, corners=p)
    a.update(kw)
    return lib.hesic_homonet_prepare(a["x1"], a["xs1"], a["x2"], a["xs2"], a["xy"], a["B"], a["H"], a["W"], a["S"], a["P"], a["mean"], a["std"],
                                     a["dtype"], a["grey1"], a["grey2"], a["patch1"], a["patch2"], a["corners"], None)


@pytest.mark.parametrize("bad, word", [
    (dict(x1=None), "null"), (dict(corners=None), "null"), (dict(xs2=None), "null"),
    (dict(dtype=2), "dtype"), (dict(B=0), "shape"), (dict(B=65536), "shape"), (dict(H=0), "shape"), (dict(W=-3), "shape"),
    (dict(S=0), "P <= S"), (dict(P=0), "P <= S"), (dict(P=9), "P <= S"), (dict(S=16385, P=4), "P <= S"),
    (dict(std=0.0), "std"), (dict(std=float("nan")), "std"), (dict(mean=float("nan")), "std"),
    (dict(xs1=(C.c_int64 * 4)(1, 1, -1, 1)), "stride"), (dict(xs2=(C.c_int64 * 4)(-16, 1, 1, 1)), "stride"),
], ids=lambda v: "-".join(f"{k}" for k in v) if isinstance(v, dict) else None)
def test_bad_arguments_return_einval_with_a_message(bad, word):
    lib = L.lib()
    assert _call_raw(lib, **bad) == -1
    msg = lib.hesic_last_error().decode()
    assert msg.startswith("homonet_prepare:") and word in msg, msg


def test_misaligned_float_input_is_refused():
    lib = L.lib()
    buf = (C.c_float * 16)()
    assert _call_raw(lib, dtype=L.PREP_F32, x1=C.c_void_p(C.addressof(buf) + 1)) == -1
    assert "misaligned" in lib.hesic_last_error().decode()


# ------------------------------------------------------------------------------------------- the restatement against the loader
@pytest.mark.parametrize("case", R.CASES, ids=R.case_id)
def test_restatement_equals_the_loader(case):
    """Grey frames and windows: atol 1e-6 (one flipped grey level is 1 / (255 * 0.226) = 1.7e-2 in a channel, 5.8e-3 in the grey); corners
    exact.  The windows are the loader's own seeded draws."""
    (h, w), S, P, rho = case
    x1, x2 = R.images(case)
    p1, p2, corners = R.loader_items(x1, x2, S, P, rho, seed=11)
    xy = [(int(c[0, 0]), int(c[0, 1])) for c in corners]
    g1, g2 = R.loader_greys(x1, x2, S)
    got = R.prepare(x1, x2, xy, S, P, float(MEAN), float(STD))
    for name, a, b in zip(("grey1", "grey2", "patch1", "patch2"), got, (g1, g2, p1, p2)):
        assert a.dtype == np.float32 and a.shape == b.shape, name
        err = float(np.abs(a - b).max())
        print(f"homography_prep_ref {R.case_id(case)} {name} max |restatement - loader| {err:.3e}")
        assert err <= 1e-6, name
    assert np.array_equal(got[4], corners)


def test_float_levels_are_exact_for_all_256_bytes():
    u = np.arange(256, dtype=np.uint8)
    assert np.array_equal(R.levels((u.astype(np.float32) / np.float32(255.0)).astype(np.float32)), u.astype(np.float32))
    assert np.array_equal(R.levels(torch.from_numpy(u).float().div(255.0).numpy()), u.astype(np.float32))       # ToTensor's form
    assert np.array_equal(R.levels(np.array([-0.2, 1.7], dtype=np.float32)), np.array([0.0, 255.0], dtype=np.float32))


def test_exact_two_to_one_rounds_ties_to_even():
    """64 -> 32 averages 2 x 2 blocks: a block (a, a, a, a + 2) has the mean a + 0.5 exactly, and the level is the EVEN neighbour."""
    x = np.zeros((1, 3, 64, 64), dtype=np.uint8)
    for c, a in enumerate((10, 11, 254)):
        x[0, c] = a
        x[0, c, 1::2, 1::2] = a + (2 if a < 254 else -2)
    lv = R.resized_levels(x, 32)
    assert (lv[0, 0] == 10).all() and (lv[0, 1] == 12).all() and (lv[0, 2] == 254).all()        # 10.5 -> 10, 11.5 -> 12, 253.5 -> 254


# ------------------------------------------------------------------------------------------------------------------- windows
@pytest.mark.parametrize("S, P, rho", [(256, 128, 45), (64, 32, 8), (32, 16, 4)])
def test_random_windows_are_the_loaders(S, P, rho):
    case = ((20, 24), S, P, rho)
    x1, x2 = R.images(case, batch=5)
    for k in (0, 7):
        corners = R.loader_items(x1, x2, S, P, rho, seed=k)[2]
        random.seed(k)
        xy = homography.window_origins(5, None, S, P, rho)
        assert [list(c[0]) for c in corners] == [list(map(float, v)) for v in xy]
        assert all(rho <= v <= S - rho - P for pair in xy for v in pair)
        assert xy == homography.window_origins(5, None, S, P, rho, rng=random.Random(k))


def test_window_fallback_centre_and_given():
    assert homography.window_origins(3, None, 64, 32, 20) == [(0, 0)] * 3              # 64 - 20 - 32 < 20: the loader's x = y = 0
    state = random.getstate()
    homography.window_origins(3, None, 64, 32, 20)
    assert random.getstate() == state                                                  # ... without a draw, as in the loader
    assert homography.window_origins(2, "centre", 256, 128) == [(64, 64)] * 2
    assert homography.window_origins(1, "centre", 65, 32) == [(16, 16)]
    assert homography.window_origins(2, torch.tensor([[0, 128], [128, 0]]), 256, 128) == [(0, 128), (128, 0)]
    assert homography.window_origins(2, [(3, 4), [5, 6]], 64, 32) == [(3, 4), (5, 6)]
    assert homography.window_origins(1, np.array([[32, 32]]), 64, 32) == [(32, 32)]


def test_window_and_argument_errors_come_before_any_launch():
    launches = []
    x = torch.zeros(2, 3, 8, 8, dtype=torch.uint8)
    with L.call_hook(lambda name, args: launches.append(name)):
        for bad in ([(0, 129), (0, 0)], [(-1, 0), (0, 0)], torch.tensor([[129, 0], [0, 0]])):
            with pytest.raises(ValueError, match="outside"):
                homography.prepare_inputs(x, x, bad)
        for bad in ([(0, 0)], torch.zeros(2, 3, dtype=torch.int64), [(0, 0, 0), (0, 0, 0)]):
            with pytest.raises(ValueError, match="shape"):
                homography.prepare_inputs(x, x, bad)
        with pytest.raises(TypeError, match="integers"):
            homography.prepare_inputs(x, x, torch.zeros(2, 2))
        with pytest.raises(ValueError, match="centre"):
            homography.prepare_inputs(x, x, "center")
        with pytest.raises(ValueError, match="patch_size"):
            homography.prepare_inputs(x, x, "centre", pic_size=64, patch_size=128)
        with pytest.raises(ValueError, match="one shape"):
            homography.prepare_inputs(x, x[:, :, :4], "centre")
        with pytest.raises(ValueError, match="one shape"):
            homography.prepare_inputs(x[:, :2], x[:, :2], "centre")
        with pytest.raises(TypeError, match="uint8 or both float32"):
            homography.prepare_inputs(x, x.float(), "centre")
        with pytest.raises(TypeError, match="uint8 or both float32"):
            homography.prepare_inputs(x.double(), x.double(), "centre")
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            homography.prepare_inputs(x, x, "centre")
    assert launches == []


# ---------------------------------------------------------------------------------------------------------------- checkpoints
def test_checkpoint_keys_and_round_trip(tmp_path):
    torch.manual_seed(3)
    net = homography.Net(patch_size=32)
    plain = {k: v.clone() for k, v in net.state_dict().items()}
    sd = homography.checkpoint_state_dict(net)
    assert set(sd) == {"model." + k for k in homography.Net().state_dict()}
    torch.save({"state_dict": sd, "loss": 0.25, "epoch": 0}, tmp_path / "prefixed.pth.tar")
    torch.save({"state_dict": plain}, tmp_path / "plain.pth.tar")
    torch.save(plain, tmp_path / "bare.pth.tar")
    for name in ("prefixed", "plain", "bare"):
        other = homography.Net(patch_size=32)
        got = homography.load_checkpoint(other, tmp_path / f"{name}.pth.tar")
        for k, v in other.state_dict().items():
            assert torch.equal(v, plain[k]), (name, k)
        if name == "prefixed":
            assert got["loss"] == 0.25
    missing = dict(sd)
    missing.pop("model.fc.5.bias")
    torch.save({"state_dict": missing}, tmp_path / "missing.pth.tar")
    with pytest.raises(RuntimeError, match="fc.5.bias"):
        homography.load_checkpoint(homography.Net(patch_size=32), tmp_path / "missing.pth.tar")           # strict

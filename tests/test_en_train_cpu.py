"""Stage-2 training, the parts that need no GPU: the numpy restatement the GPU tests hold the kernels to (tests/en_train_ref.py) against fp64
torch autograd and ``functional._mirror_t``, the C ABI of include/hesic_en_train.h with its refusals, the host logic of
``python -m hesic_amd.train_stage2`` and ``Independent_EN.criterion``'s plain path."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import torch

import en_train_ref as R
from hesic_amd import synthetic

LAMBDA = 0.0067


def _lib():
    from hesic_amd import _lib as L
    if not (os.path.exists(L.LIB_PATH) and os.path.exists(L.LIB_PATH_F16)):
        import __graft_entry__ as ge
        ge.build()
    return L


def _images(tag, shape):
    a = synthetic._uniform(f"en.cpu.{tag}.a", shape, -0.2, 1.2).float()
    b = synthetic._uniform(f"en.cpu.{tag}.b", shape, 0, 1).float()
    return a, b


# --------------------------------------------------------------------------------------------------- the restatement's 16-bit rounding
def _edge_values():
    g = np.random.Generator(np.random.PCG64(5))
    bits = g.integers(0, 2 ** 32, size=200000, dtype=np.uint64).astype(np.uint32)
    x = bits.view(np.float32)
    x = x[np.isfinite(x)]
    small = (g.standard_normal(50000) * 10.0 ** g.uniform(-9, 5, 50000)).astype(np.float32)
    ties = np.array([1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, 1.0 + 2.0 ** -11, 1.0 + 3 * 2.0 ** -11, 65504.0, 65519.9, 65520.0, 2.0 ** -24, 2.0 ** -25,
                     2.0 ** -25 * 1.0000001, 3 * 2.0 ** -25, 2.0 ** -14, 2.0 ** -14 * (1 - 2.0 ** -12), 0.0, -0.0, 3.3895314e38, 3.4e38], dtype=np.float32)
    return np.concatenate((x, small, ties, -ties))


@pytest.mark.parametrize("fmt,dtype", [("bf16", torch.bfloat16), ("f16", torch.float16)])
def test_integer_rounding_is_round_to_nearest_even(fmt, dtype):
    x = _edge_values()
    want = torch.from_numpy(x).to(dtype).view(torch.int16).numpy().view(np.uint16)
    got = R.ROUND[fmt](x)
    assert np.array_equal(got, want), np.flatnonzero(got != want)[:5]
    nan = R.ROUND[fmt](np.array([np.nan, -np.nan, np.inf, -np.inf], dtype=np.float32))
    back = torch.from_numpy(nan.view(np.int16)).view(dtype).float()
    assert torch.isnan(back[:2]).all() and back[2] == float("inf") and back[3] == -float("inf")


# ---------------------------------------------------------------------------------------------------- the restatement against autograd
@pytest.mark.parametrize("shape", [(1, 3, 1, 1), (2, 3, 3, 5), (1, 3, 17, 29)], ids=str)
def test_restatement_equals_fp64_autograd(shape):
    """loss and d loss / d a of lambda * 255^2 * (MSE(a1, b1) + MSE(a2, b2)) in fp64 autograd: the sums to fp64 rounding, the gradient map to the
    roundings the restatement models (fp32 subtract and multiply: 2^-23 relative, then half a unit of the 16-bit format)."""
    (a1, b1), (a2, b2) = _images("r1", shape), _images("r2", shape)
    k = LAMBDA * 255 ** 2
    A1, A2 = a1.double().requires_grad_(True), a2.double().requires_grad_(True)
    mse = torch.nn.functional.mse_loss(A1, b1.double()) + torch.nn.functional.mse_loss(A2, b2.double())
    (k * mse).backward()
    vals = R.loss_values(a1.numpy(), b1.numpy(), a2.numpy(), b2.numpy(), k)
    # fp64 autograd subtracts in fp64 (exact here: both operands are fp32); the restatement's fp32 difference is within 2^-24 of it per element
    assert vals[2] == pytest.approx(float(mse.detach()), rel=1e-6) and vals[3] == pytest.approx(float(k * mse.detach()), rel=1e-6)
    assert vals[3] == k * vals[2] and vals[2] == vals[0] / a1.numel() + vals[1] / a1.numel()
    B, _, H, W = shape
    for fmt, dtype, ulp in (("bf16", torch.bfloat16, 2.0 ** -8), ("f16", torch.float16, 2.0 ** -11)):
        for a, b, A in ((a1, b1, A1), (a2, b2, A2)):
            bits = R.grad_map_bits(a.numpy(), b.numpy(), k, fmt)
            assert bits.shape == (B, H, W, 32) and not bits[..., 3:].any()
            got = torch.from_numpy(bits[..., :3].copy().view(np.int16)).view(dtype).double().permute(0, 3, 1, 2)
            want = A.grad
            tol = want.abs() * (ulp + 2.0 ** -21) + 2.0 ** -25           # half a unit in the last place, the fp32 steps, binary16's subnormal step
            assert bool(((got - want).abs() <= tol).all()), float(((got - want).abs() / tol).max())
    # the seed multiplies the scale in fp32
    s, s2 = R.scale(B, H, W, k), R.scale(B, H, W, k, seed=0.5)
    assert s2 == np.float32(s * np.float32(0.5)) and s == np.float32(2.0 * k / (B * 3 * H * W))


def test_exact_sse_is_exact_and_nan_stays_in_its_view():
    a, b = _images("x", (2, 3, 5, 7))
    d = (a.numpy() - b.numpy()).astype(np.float64)
    from fractions import Fraction
    exact = sum(Fraction(float(v)) ** 2 for v in d.reshape(-1))
    assert Fraction(R.exact_sse(a.numpy(), b.numpy())) == Fraction(float(exact))          # the correctly rounded sum
    a2 = a.clone()
    a2[1, 2, 3, 4] = float("nan")
    v = R.loss_values(a2.numpy(), b.numpy(), a.numpy(), b.numpy(), 1.0)
    assert np.isnan(v[0]) and np.isfinite(v[1]) and np.isnan(v[2]) and np.isnan(v[3])
    bits = R.grad_map_bits(a2.numpy(), b.numpy(), 1.0, "bf16")
    back = torch.from_numpy(bits.view(np.int16)).view(torch.bfloat16).float()
    assert int(torch.isnan(back).sum()) == 1 and bool(torch.isnan(back[1, 3, 4, 2]))
    assert R.sum_bar(3) == 11 * 2.0 ** -53


# ----------------------------------------------------------------------------------------------------------------------------- the mirror
@pytest.mark.parametrize("cout,cin,pad", [(32, 32, None), (32, 32, 32), (32, 6, 32), (3, 32, 32)], ids=str)
def test_mirror_equals_mirror_t(cout, cin, pad):
    from hesic_amd import functional as Fn
    w = synthetic._uniform(f"en.cpu.w{cout}.{cin}", (cout, cin, 3, 3), -1, 1).float()
    want = Fn._mirror_t(w, pad)
    got = torch.from_numpy(R.mirror(w.numpy(), pad))
    assert got.shape == want.shape == (cin, max(cout, pad or 0), 3, 3) and torch.equal(got, want)


# -------------------------------------------------------------------------------------------------------------------------------- ABI
@pytest.mark.parametrize("fmt", ["bf16", "f16"])
def test_abi_header_bindings_exports(fmt):
    L = _lib()
    declared = L.declared_symbols("hesic_en_train.h")
    assert declared == ["hesic_c32_mirror_weights", "hesic_en_loss", "hesic_en_loss_grad", "hesic_en_loss_ws_bytes"]
    assert set(declared) == set(L._EN_TRAIN_SIGS)
    assert not set(declared) & set(L.declared_symbols())                # a header of its own: include/hesic_hip.h does not list it
    assert "hesic_en_train.h" not in open(L.header_path("hesic_hip.h")).read()
    assert C.sizeof(L.MirrorEntry) == 32
    exported = subprocess.check_output(["nm", "-D", "--defined-only", L.LIB_PATH_F16 if fmt == "f16" else L.LIB_PATH], text=True)
    for s in declared:
        assert f" T {s}\n" in exported, s
    lib = L.lib(torch.float16 if fmt == "f16" else torch.bfloat16)      # binds every signature, the new ones included
    assert lib.hesic_abi_version() == 3


def _host_ptr(offset=0):
    buf = (C.c_double * 64)()
    return C.c_void_p(C.cast(buf, C.c_void_p).value + offset), buf


def _call(lib, name, **kw):
    """An entry point with host dummies for pointers: every case below is refused before anything is launched or dereferenced."""
    p, keep = _host_ptr()
    if name == "hesic_en_loss":
        a = dict(a1=p, b1=p, a2=p, b2=p, B=2, H=4, W=4, k=1.0, out=p, ws=p, ws_bytes=1 << 20)
        a.update(kw)
        return lib.hesic_en_loss(a["a1"], a["b1"], a["a2"], a["b2"], a["B"], a["H"], a["W"], a["k"], a["out"], a["ws"], a["ws_bytes"], None)
    if name == "hesic_en_loss_grad":
        a = dict(a1=p, b1=p, a2=p, b2=p, B=2, H=4, W=4, k=1.0, seed=None, g1=p, g2=p)
        a.update(kw)
        return lib.hesic_en_loss_grad(a["a1"], a["b1"], a["a2"], a["b2"], a["B"], a["H"], a["W"], a["k"], a["seed"], a["g1"], a["g2"], None)
    a = dict(src=p, src_numel=64, dst=p, dst_numel=64, table=p, n_layers=1, capacity=1)
    a.update(kw)
    return lib.hesic_c32_mirror_weights(a["src"], a["src_numel"], a["dst"], a["dst_numel"], a["table"], a["n_layers"], a["capacity"], None)


_ODD8, _K1 = _host_ptr(4)
_ODD4, _K2 = _host_ptr(2)


@pytest.mark.parametrize("name,bad,word", [
    ("hesic_en_loss", dict(a1=None), "null"), ("hesic_en_loss", dict(b2=None), "null"), ("hesic_en_loss", dict(out=None), "null"),
    ("hesic_en_loss", dict(ws=None), "null"),
    ("hesic_en_loss", dict(B=0), "non-positive"), ("hesic_en_loss", dict(H=0), "non-positive"), ("hesic_en_loss", dict(W=-1), "non-positive"),
    ("hesic_en_loss", dict(H=1 << 16, W=1 << 15), "2^31"), ("hesic_en_loss", dict(H=46341, W=46341), "2^31"),
    ("hesic_en_loss", dict(ws_bytes=0), "workspace too small"), ("hesic_en_loss", dict(ws_bytes=2 * 2 * 8 - 1), "workspace too small"),
    ("hesic_en_loss", dict(ws=_ODD8), "8-byte aligned"), ("hesic_en_loss", dict(out=_ODD8), "8-byte aligned"),
    ("hesic_en_loss", dict(a2=_ODD4), "4-byte aligned"),
    ("hesic_en_loss_grad", dict(b1=None), "null"), ("hesic_en_loss_grad", dict(g2=None), "null"),
    ("hesic_en_loss_grad", dict(B=-3), "non-positive"), ("hesic_en_loss_grad", dict(H=1 << 16, W=1 << 15), "2^31"),
    ("hesic_en_loss_grad", dict(g1=_ODD8), "16-byte aligned"), ("hesic_en_loss_grad", dict(seed=_ODD4), "4-byte aligned"),
    ("hesic_c32_mirror_weights", dict(src=None), "null"), ("hesic_c32_mirror_weights", dict(dst=None), "null"),
    ("hesic_c32_mirror_weights", dict(table=None), "null"),
    ("hesic_c32_mirror_weights", dict(n_layers=0), "outside 1.."), ("hesic_c32_mirror_weights", dict(n_layers=3, capacity=2), "capacity"),
    ("hesic_c32_mirror_weights", dict(dst_numel=0), "non-positive"), ("hesic_c32_mirror_weights", dict(table=_ODD8), "misaligned"),
], ids=lambda v: "-".join(v) if isinstance(v, dict) else str(v).replace(" ", "_"))
def test_bad_arguments_return_einval_with_a_message(name, bad, word):
    lib = _lib().lib()
    assert _call(lib, name, **bad) == -1
    msg = lib.hesic_last_error().decode()
    assert msg.startswith(name[len("hesic_"):] + ":") and word in msg, msg


def test_ws_bytes_depends_on_its_arguments_alone():
    lib = _lib().lib()
    ws = lib.hesic_en_loss_ws_bytes
    assert ws(1, 1, 1) == 2 * 8 and ws(2, 3, 5) == 2 * 2 * 8
    assert ws(1, 32, 42) == 2 * 8 and ws(1, 37, 37) == 2 * 2 * 8          # 3 * 32 * 42 = 4032 <= 4096 < 3 * 37 * 37 = 4107
    assert ws(1, 512, 512) == 2 * 64 * 8 and ws(1, 4096, 4096) == 2 * 64 * 8      # the cap
    # an image's block count depends on H * W alone: B images need B times the partials of one, whatever was asked before
    assert ws(8, 512, 512) == 8 * ws(1, 512, 512) and ws(3, 64, 64) == 3 * ws(1, 64, 64) and ws(1, 64, 64) == ws(1, 128, 32)
    assert [ws(2, 100, 100) for _ in range(3)] == [2 * ws(1, 100, 100)] * 3
    for args, word in (((0, 4, 4), "non-positive"), ((1, 0, 4), "non-positive"), ((1, 65536, 32768), "2^31"), (((1 << 20) + 1, 4, 4), "2^20")):
        assert ws(*args) == -1
        msg = lib.hesic_last_error().decode()
        assert msg.startswith("en_loss_ws_bytes:") and word in msg, msg


def test_wrappers_refuse_cpu_tensors_and_bad_shapes():
    from hesic_amd import functional as Fn
    x = torch.zeros(2, 3, 4, 4)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        Fn.en_loss(x, x, x, x, 1.0)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        Fn.en_loss_grad(x, x, x, x, 1.0)


# --------------------------------------------------------------------------------------------------------- the command's host logic
def _write_pair(root, split, stem, h, w, H=None, seed=0):
    from PIL import Image
    g = np.random.Generator(np.random.PCG64([11, seed]))
    for side in ("left", "right"):
        d = root / split / side
        d.mkdir(parents=True, exist_ok=True)
        Image.fromarray(g.integers(0, 256, size=(h, w, 3), dtype=np.uint8)).save(d / f"{stem}.png")
    if H is not None:
        (root / split / "H").mkdir(exist_ok=True)
        np.save(root / split / "H" / f"{stem}.npy", H)


def test_parser_defaults_and_shared_code():
    from hesic_amd import train_folder, train_stage2
    a = train_stage2.parser().parse_args(["root", "--checkpoint", "synthetic"])
    assert (a.root, a.epochs, a.learning_rate, a.lmbda, a.batch_size, a.test_batch_size, tuple(a.patch_size), a.num_workers, a.save, a.seed,
            a.homography, a.homography_checkpoint, a.clip_max_norm, a.skip_nonfinite, a.graphed, a.dtype, a.cache, a.cache_gb, a.valid_split,
            a.out, a.model, a.checkpoint, a.infer_dtype, a.resume) == \
        ("root", 100, 1e-4, 1e-2, 16, 64, (256, 256), 3, False, None, "sidecar", None, None, False, False, "bf16", "device", None, "test", ".",
         "hesic", "synthetic", "f16", "none")
    for bad in (["r", "--dtype", "f16"], ["r", "--infer-dtype", "f64"], ["r", "--model", "x"], ["r", "--aux-learning-rate", "1"],
                ["r", "--distortion", "mse"], []):
        with pytest.raises(SystemExit):
            train_stage2.parser().parse_args(bad)
    # imported, not copied
    assert train_stage2._inputs is train_folder._inputs and train_stage2._Homography is train_folder._Homography
    assert train_stage2._kept is train_folder._kept


def test_main_refuses_bad_flags_and_returns_2_without_a_device(tmp_path, capsys):
    from hesic_amd import train_stage2
    for split in ("train", "test"):
        _write_pair(tmp_path, split, "a", 80, 96, np.eye(3))
    ok = ["--checkpoint", "synthetic", "--patch-size", "64", "64"]
    for bad in (["--checkpoint", "synthetic", "--patch-size", "64", "80"],           # not a multiple of 64
                ["--checkpoint", "synthetic", "--patch-size", "128", "64"],          # larger than an image
                ["--patch-size", "64", "64"],                                        # no --checkpoint
                [*ok, "--homography-checkpoint", "x.pth.tar"],                       # without --homography net
                [*ok, "--batch-size", "0"], [*ok, "--cache-gb", "0"]):
        with pytest.raises(SystemExit) as e:
            train_stage2.main([str(tmp_path), *bad], log=lambda s: None)
        assert e.value.code == 2, bad
    err = capsys.readouterr().err
    assert "multiples of 64" in err and "larger than" in err and "--checkpoint is required" in err and "needs --homography net" in err
    if not torch.cuda.is_available():
        assert train_stage2.main([str(tmp_path), *ok], log=lambda s: None) == 2
        assert "needs a ROCm device" in capsys.readouterr().err


# ------------------------------------------------------------------------------------------------------- the criterion's plain path
def test_criterion_on_the_cpu_equals_the_modules_plain_path(monkeypatch):
    """On the CPU ``Independent_EN.criterion`` is ``forward`` plus torch's elementwise ops: the same loss, mse, images and gradients.  The warp
    and the general conv operator have no CPU path, so both sides run with the same torch stand-ins for them (the warp: a shift by one
    column, so that the two views' inputs differ): what is compared is ``criterion``'s own branch against ``forward`` + the loss."""
    from hesic_amd import functional as Fn
    from hesic_amd import models
    from test_oracle_golden import _en_params

    def shift(src, M, dsize, inverse_map=False, **kw):
        return torch.roll(src, -1 if inverse_map else 1, dims=-1)

    def conv2d(x, weight, bias, *, kernel_size, stride, padding, act=0, **kw):
        y = torch.nn.functional.conv2d(x, weight, bias, stride=stride, padding=padding)
        return torch.nn.functional.leaky_relu(y, 0.01) if act == 2 else y

    monkeypatch.setattr(models, "warp_perspective", shift)
    monkeypatch.setattr(Fn, "conv2d", conv2d)
    en = models.Independent_EN()
    en.load_state_dict(_en_params(), strict=True)
    en.train()
    x1, x2, Hm = synthetic.stereo_batch(3, 2, 16, 24)
    r1 = (x1 + synthetic._uniform("en.cpu.c1", x1.shape, -0.05, 0.05)).float()
    r2 = (x2 + synthetic._uniform("en.cpu.c2", x2.shape, -0.05, 0.05)).float()
    assert torch.equal(en.EH1(r1, r2), en.EH1.head(en.EH1.trunk(r1, r2), r1))            # forward is trunk + the output branch

    crit = en.criterion(r1, r2, Hm, x1, x2, LAMBDA)
    assert set(crit) == {"loss", "mse_loss", "x1_hat", "x2_hat"}
    assert crit["loss"].requires_grad and not crit["mse_loss"].requires_grad and not crit["x1_hat"].requires_grad
    crit["loss"].backward()
    got = {k: p.grad.clone() for k, p in en.named_parameters()}
    en.zero_grad(set_to_none=True)

    out = en(r1, r2, Hm)
    mse = ((out["x1_hat"].float() - x1) ** 2).mean() + ((out["x2_hat"].float() - x2) ** 2).mean()
    loss = LAMBDA * 255 ** 2 * mse
    loss.backward()
    assert torch.equal(crit["loss"].detach(), loss.detach()) and torch.equal(crit["mse_loss"], mse.detach())
    assert torch.equal(crit["x1_hat"], out["x1_hat"].detach()) and torch.equal(crit["x2_hat"], out["x2_hat"].detach())
    for k, p in en.named_parameters():
        assert torch.equal(got[k], p.grad), k

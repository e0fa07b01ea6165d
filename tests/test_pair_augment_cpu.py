"""Stereo-aware augmentation in the pair gather, the parts that need no GPU: the numpy restatement the GPU test holds the kernel to
(tests/pair_augment_ref.py) against numpy flips, ``numpy.linalg.inv`` and a bilinear warp; ``pair_cache.epoch_plan(augment=...)``; the C ABI of
include/hesic_pair_augment.h; the wrapper's refusal of unknown flag bits and the trainers' ``--augment`` option."""
import ctypes as C
import subprocess

import numpy as np
import pytest

import pair_augment_ref as A
import pair_batch_ref as R
from hesic_amd import _lib as L
from hesic_amd import functional as Fn
from hesic_amd import pair_cache, train_folder, train_stage2

FLAGS = list(range(8))


def _matrices(n, seed=21):
    """Full-image homographies like the existing test table (near a translation of tens of pixels, small perspective terms), with fp64
    entries that are not fp32-representable, each with a crop origin (hx, hy)."""
    g = np.random.Generator(np.random.PCG64(seed))
    out = []
    for _ in range(n):
        H = np.eye(3) + g.normal(0, 0.02, size=(3, 3))
        H[0, 2], H[1, 2] = g.uniform(-60, 60), g.uniform(-20, 20)
        H[2, 0], H[2, 1] = g.normal(0, 2e-5), g.normal(0, 2e-5)
        out.append(((H / H[2, 2]).reshape(9), int(g.integers(0, 1201)), int(g.integers(0, 1201))))
    return out


# ------------------------------------------------------------------------------------------------------------------- pixels
@pytest.mark.parametrize("shape, crop, origin", [((37, 53), (16, 20), (21, 33)), ((37, 53), (16, 19), (0, 0)), ((40, 64), (5, 1), (35, 63)),
                                                 ((40, 64), (40, 64), (0, 0))])
@pytest.mark.parametrize("flags", FLAGS)
def test_restatement_pixels_are_numpy_flips_and_a_view_exchange(shape, crop, origin, flags):
    g = np.random.Generator(np.random.PCG64([3, *shape]))
    left, right = (g.integers(0, 256, size=(*shape, 3), dtype=np.uint8) for _ in range(2))
    (ph, pw), (y0, x0) = crop, origin
    got = A.pixels(left, right, x0, y0, ph, pw, flags)
    want = [R.pixels(v, x0, y0, ph, pw) for v in ((right, left) if flags & A.SWAP else (left, right))]
    for gv, wv in zip(got, want):
        if flags & A.VFLIP:
            wv = wv[:, ::-1, :]
        if flags & A.HFLIP:
            wv = wv[:, :, ::-1]
        assert gv.dtype == np.float32 and gv.shape == (3, ph, pw) and np.array_equal(gv, wv)


# ------------------------------------------------------------------------------------------------------------------- matrix
def test_restatement_matrix_without_flags_is_the_plain_one_bit_for_bit():
    for H, hx, hy in _matrices(200):
        a, b = A.matrix(H, hx, hy, 64, 48, 0), R.matrix(H, hx, hy)
        assert a.dtype == np.float32 and np.array_equal(a.view(np.int32), b.view(np.int32))
    for f in FLAGS:
        assert np.array_equal(A.matrix(None, 5, 7, 64, 48, f), np.eye(3, dtype=np.float32))           # h_index = -1: the identity whatever the flags


def _by_matrix_products(H, hx, hy, ph, pw, flags):
    """F_v F_h R F_h F_v, inverted by numpy for a swap, normalised: the same map by library products instead of the header's scalar steps."""
    M = A.rebased(H, hx, hy)
    Fh = np.array([[-1, 0, pw - 1], [0, 1, 0], [0, 0, 1]], dtype=np.float64) if flags & A.HFLIP else np.eye(3)
    Fv = np.array([[1, 0, 0], [0, -1, ph - 1], [0, 0, 1]], dtype=np.float64) if flags & A.VFLIP else np.eye(3)
    M = Fv @ Fh @ M @ Fh @ Fv
    if flags & A.SWAP:
        M = np.linalg.inv(M)
    return M / M[2, 2]


@pytest.mark.parametrize("flags", FLAGS)
def test_restatement_matrix_agrees_with_the_matrix_products(flags):
    """1e-12 relative to the matrix's largest entry: both sides are fp64 evaluations of the same rational function of well-conditioned
    inputs, a few hundred fp64 ulps (1.1e-16 each) apart at the most."""
    worst = 0.0
    for ph, pw in ((64, 64), (16, 19), (5, 1)):
        for H, hx, hy in _matrices(100):
            got, want = A.matrix64(H, hx, hy, ph, pw, flags), _by_matrix_products(H, hx, hy, ph, pw, flags)
            err = float(np.abs(got - want).max() / np.abs(want).max())
            worst = max(worst, err)
            assert err <= 1e-12, (flags, ph, pw, err)
    print(f"pair_augment_ref matrix, flags {flags}: worst relative difference to the matrix products {worst:.2e} (bar 1e-12)")


@pytest.mark.parametrize("flips", [0, 1, 2, 3])
def test_swapped_matrix_times_the_unswapped_one_is_the_identity(flips):
    worst = 0.0
    for H, hx, hy in _matrices(100):
        P = A.matrix64(H, hx, hy, 64, 48, flips | A.SWAP) @ A.matrix64(H, hx, hy, 64, 48, flips)
        err = float(np.abs(P / P[2, 2] - np.eye(3)).max() / np.abs(A.matrix64(H, hx, hy, 64, 48, flips)).max())
        worst = max(worst, err)
        assert err <= 1e-12, (flips, err)
    print(f"pair_augment_ref H_swap H, flips {flips}: worst |H_swap H / [2,2] - I| relative to H's largest entry {worst:.2e} (bar 1e-12)")


# --------------------------------------------------------------------------------------------------------------------- warp
def _warp(x, H):
    """Plain bilinear warp in fp64, zeros outside: out[r, q] = x sampled at H (q, r, 1), each of the four neighbours counting as 0 where it
    lies outside the image (so the warp is continuous in H)."""
    h, w = x.shape
    q, r = np.meshgrid(np.arange(w, dtype=np.float64), np.arange(h, dtype=np.float64))
    d = H[2, 0] * q + H[2, 1] * r + H[2, 2]
    u, v = (H[0, 0] * q + H[0, 1] * r + H[0, 2]) / d, (H[1, 0] * q + H[1, 1] * r + H[1, 2]) / d
    u0, v0 = np.floor(u), np.floor(v)
    out = np.zeros_like(x)
    for dv in (0, 1):
        for du in (0, 1):
            ui, vi = (u0 + du).astype(np.int64), (v0 + dv).astype(np.int64)
            wgt = (1 - np.abs(u - (u0 + du))) * (1 - np.abs(v - (v0 + dv)))
            ok = (ui >= 0) & (ui < w) & (vi >= 0) & (vi < h)
            out += np.where(ok, wgt * x[np.clip(vi, 0, h - 1), np.clip(ui, 0, w - 1)], 0.0)
    return out


def _flip(img, flags):
    """Rows and columns of one image reversed as the flags say."""
    if flags & A.VFLIP:
        img = img[::-1]
    if flags & A.HFLIP:
        img = img[:, ::-1]
    return np.ascontiguousarray(img)


@pytest.mark.parametrize("flags", FLAGS)
def test_warp_commutes_with_the_augmentation(flags):
    """warp(aug(x1), H_aug) == aug(warp(x1, H)) -- with a swap, aug(warp(x2, H^-1)) -- on [0, 1] images to 1e-10."""
    ph, pw = 24, 33
    g = np.random.Generator(np.random.PCG64([9, flags]))
    worst = 0.0
    for _ in range(6):
        x1, x2 = g.uniform(0, 1, size=(ph, pw)), g.uniform(0, 1, size=(ph, pw))
        H = np.eye(3) + g.normal(0, 0.02, size=(3, 3))
        H[0, 2], H[1, 2] = g.uniform(-6, 6), g.uniform(-4, 4)
        H[2, 0], H[2, 1] = g.normal(0, 2e-5, size=2)
        H = (H / H[2, 2]).reshape(9)
        hx, hy = int(g.integers(0, 40)), int(g.integers(0, 40))
        plain, aug = A.matrix64(H, hx, hy, ph, pw, 0), A.matrix64(H, hx, hy, ph, pw, flags)
        got = _warp(_flip(x2 if flags & A.SWAP else x1, flags), aug)
        want = _flip(_warp(x2, np.linalg.inv(plain)) if flags & A.SWAP else _warp(x1, plain), flags)
        assert float(np.abs(want).max()) > 0.1                                  # the warp is not all zeros
        worst = max(worst, float(np.abs(got - want).max()))
    print(f"pair_augment warp property, flags {flags}: worst |warp(aug(x1), H_aug) - aug(warp(x1, H))| {worst:.2e} (bar 1e-10)")
    assert worst <= 1e-10


# --------------------------------------------------------------------------------------------------------------- epoch_plan
SIZES = [(96, 128)] * 3 + [(80, 112)] * 2
ALL = ("hflip", "vflip", "swap")


def _plan(**kw):
    a = dict(n_pairs=5, sizes=SIZES, batch_size=2, ph=64, pw=64, seed=1, epoch=0, shuffle=True, drop_tail=False)
    a.update(kw)
    return pair_cache.epoch_plan(**a)


def test_plan_without_augmentation_is_the_plan_as_it_was():
    old, new = _plan(), _plan(augment=())
    assert list(old) == list(new) and old.rng.random() == new.rng.random()
    assert new.flags == [[0, 0], [0, 0], [0]] and old.flags == new.flags
    assert new.augmented() == {"hflip": 0, "vflip": 0, "swap": 0}


def test_augmentation_leaves_order_crops_and_the_epochs_stream_alone():
    for epoch in (0, 1, 7):
        old, new = _plan(epoch=epoch), _plan(epoch=epoch, augment=ALL)
        assert list(old) == list(new) and [len(f) for f in new.flags] == [len(idx) for idx, _ in new]
        assert old.rng.getstate() == new.rng.getstate()


def test_flags_repeat_for_a_seed_and_epoch_and_differ_between_epochs():
    big = dict(n_pairs=64, sizes=[(96, 128)] * 64, batch_size=8)
    a, b = _plan(augment=ALL, **big), _plan(augment=ALL, **big)
    assert a.flags == b.flags and _plan(augment=list(reversed(ALL)), **big).flags == a.flags      # a collection: its order does not matter
    assert _plan(augment=ALL, epoch=1, **big).flags != a.flags and _plan(augment=ALL, seed=2, **big).flags != a.flags
    assert {f for fl in a.flags for f in fl} <= set(range(8))


def test_flags_are_the_documented_stream():
    import random
    rng = random.Random("1/3/augment")
    plan = _plan(epoch=3, augment=("swap", "hflip"))
    want = [[sum(bit for bit in (1, 4) if rng.getrandbits(1)) for _ in idx] for idx, _ in plan]
    assert plan.flags == want


@pytest.mark.parametrize("augment", [("hflip",), ("vflip",), ("swap",), ("hflip", "swap"), ALL])
def test_each_enabled_flag_is_set_on_about_half_of_4096_items(augment):
    """45-55 % of 4096 fair draws: 2048 +- 205 is 6.4 standard deviations (sigma = 32), and the stream is fixed by the seed anyway."""
    plan = _plan(n_pairs=4096, sizes=[(96, 128)] * 4096, batch_size=16, augment=augment)
    counts = plan.augmented()
    print(f"epoch_plan augment {augment}: {counts} of 4096")
    for name, n in counts.items():
        if name in augment:
            assert 0.45 * 4096 <= n <= 0.55 * 4096, (name, n)
        else:
            assert n == 0, (name, n)


def test_validation_and_unknown_names_are_refused():
    with pytest.raises(ValueError, match="validation"):
        _plan(epoch=None, shuffle=False, augment=("hflip",))
    assert _plan(epoch=None, shuffle=False, augment=()).flags == [[0, 0], [0, 0], [0]]
    with pytest.raises(ValueError, match="rot90"):
        _plan(augment=("hflip", "rot90"))


# ------------------------------------------------------------------------------------------------------------------------ ABI
@pytest.mark.parametrize("fmt", ["bf16", "f16"])
def test_abi_header_bindings_exports(fmt):
    declared = L.declared_symbols("hesic_pair_augment.h")
    assert declared == ["hesic_pair_batch_gather_aug"] and set(declared) == set(L._PAIR_AUGMENT_SIGS)
    assert L._PAIR_AUGMENT_SIGS["hesic_pair_batch_gather_aug"] == L._PAIR_BATCH_SIGS["hesic_pair_batch_gather"]        # the same arguments
    assert not set(declared) & set(L.declared_symbols()) and L.ABI_VERSION == 3
    text = open(L.header_path("hesic_pair_augment.h")).read()
    for name, bit in (("HFLIP", L.PAIR_HFLIP), ("VFLIP", L.PAIR_VFLIP), ("SWAP", L.PAIR_SWAP)):
        assert f"#define HESIC_PAIR_{name} {bit}" in text and pair_cache.AUGMENT_BITS[name.lower()] == bit
    assert (Fn.PAIR_HFLIP, Fn.PAIR_VFLIP, Fn.PAIR_SWAP, Fn.PAIR_FLAG_MASK) == (1, 2, 4, 7)
    for formula in ("S0j = a * R2j - R0j", "Ti2 = a * Si0 + Si2", "S1j = c * R2j - R1j", "Ti2 = c * Si1 + Si2", "U00 = m11 * m22 - m12 * m21",
                    "U21 = m01 * m20 - m00 * m21", "(float)(R[i][j] / R[2][2])", "CANNOT refuse"):
        assert formula in text, formula
    exported = subprocess.check_output(["nm", "-D", "--defined-only", L.LIB_PATH_F16 if fmt == "f16" else L.LIB_PATH], text=True)
    assert " T hesic_pair_batch_gather_aug\n" in exported and " T hesic_pair_batch_gather\n" in exported


@pytest.mark.parametrize("bad, word", [(dict(items=None), "null"), (dict(x2=None), "null"), (dict(B=0), "shape"), (dict(pw=0), "shape"),
                                       (dict(B=8, ph=16384, pw=16384), "overflows"), (dict(misalign="x1"), "misaligned")],
                         ids=lambda v: "-".join(f"{k}{x}" for k, x in v.items()) if isinstance(v, dict) else None)
def test_bad_arguments_return_einval_with_a_message(bad, word):
    """Host dummies for pointers: every case is refused before anything is launched or dereferenced."""
    lib = L.lib()
    buf = (C.c_double * 16)()
    p = C.cast(buf, C.c_void_p)
    a = dict(items=p, h_table=p, B=1, ph=4, pw=4, x1=p, x2=p, h_out=p)
    if "misalign" in bad:
        a[bad["misalign"]] = C.c_void_p(C.addressof(buf) + 2)
    else:
        a.update(bad)
    assert lib.hesic_pair_batch_gather_aug(a["items"], a["h_table"], a["B"], a["ph"], a["pw"], a["x1"], a["x2"], a["h_out"], None) == -1
    msg = lib.hesic_last_error().decode()
    assert msg.startswith("pair_batch_gather_aug:") and word in msg, msg


# ------------------------------------------------------------------------------------------------- the wrapper's host checks
def _items(**kw):
    it = Fn.pair_items(2)
    for f, v in dict(left=4096, right=8192, pitch_px=40, rows=30, x0=3, y0=2, hx=3, hy=2, h_index=-1).items():
        it[f] = v
    for f, v in kw.items():
        it[f][1] = v
    return it


@pytest.mark.parametrize("reserved", [8, 9, 16, -1, 1 << 30])
def test_wrapper_refuses_unknown_flag_bits_before_any_launch(reserved):
    """Before any launch and before the device check: on a host without a GPU the ValueError still comes first."""
    launches = []
    with L.call_hook(lambda name, args: launches.append(name)):
        with pytest.raises(ValueError, match="reserved") as e:
            Fn.pair_batch_gather_aug(_items(reserved=reserved), None, 16, 32)
        assert "item 1" in str(e.value) and "pair_batch_gather_aug" in str(e.value)
    assert launches == []


@pytest.mark.parametrize("reserved", FLAGS)
def test_the_three_bits_pass_the_new_check_and_the_old_entry_still_wants_zero(reserved):
    Fn.check_pair_items(_items(reserved=reserved), 0, 16, 32, Fn.PAIR_FLAG_MASK, "pair_batch_gather_aug")
    if reserved:
        with pytest.raises(ValueError, match="reserved field must be 0"):
            Fn.pair_batch_gather(_items(reserved=reserved), None, 16, 32)
    with pytest.raises(ValueError, match="columns"):
        Fn.pair_batch_gather_aug(_items(reserved=reserved, x0=9), None, 16, 32)                   # the other checks are the plain entry's


# ------------------------------------------------------------------------------------------------------------------- parser
@pytest.mark.parametrize("mod", [train_folder, train_stage2], ids=["train_folder", "train_stage2"])
def test_parsers_take_augment_and_default_to_none(mod, capsys):
    p = mod.parser()
    assert tuple(p.parse_args(["root"]).augment) == ()
    assert list(p.parse_args(["root", "--augment", "hflip", "swap", "-e", "3"]).augment) == ["hflip", "swap"]
    with pytest.raises(SystemExit):
        p.parse_args(["root", "--augment", "rot90"])
    assert "--augment" in capsys.readouterr().err

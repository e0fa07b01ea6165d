"""The options of one launch belong to that launch.  Many entry points of the library are an ordinary launcher plus options -- a fused
GDN, a workspace, an fp32 copy, hi/lo operands, a prepacked weight image, "accumulate", "stop behind the first kernel".  For the three
files that have such families (csrc/conv_igemm.hip, sconv.hip, wgrad.hip) this test runs the plain entry point, then every sibling that
carries an option -- once validly and once with arguments its checks refuse, which returns an argument error before anything is
launched -- and then the plain entry point again: its output is bit-identical to the first.  The one option that is MEANT to travel,
hesic_conv2d_hilo_set_acc_scale, is consumed by the next hi/lo launch of the thread even when that launch is refused.

The convolution families are refused through a wrong Ho; hesic_conv2d_wgrad_* and hesic_gdn_backward* check no output size, they get a
channel count / pixel count / channel width their own checks refuse."""
import ctypes as C

import pytest
import torch

import hesic_amd
from hesic_amd import synthetic

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF = torch.bfloat16
CL = torch.channels_last


def rnd(name, shape, lo=-1.0, hi=1.0):
    return synthetic._uniform("iso." + name, shape, lo, hi)


@pytest.fixture
def L():
    from hesic_amd import _lib
    hesic_amd.set_compute_dtype(BF)          # the bfloat16 library is the active one
    yield _lib
    hesic_amd.set_compute_dtype(torch.float32)


def refused(L, match, name, *args):
    with pytest.raises(RuntimeError, match=match):
        L.call(name, *args)


def with_field(d, **fields):
    d2 = type(d).from_buffer_copy(d)
    for k, v in fields.items():
        setattr(d2, k, v)
    return d2


def nhwc(B, Cc, H, W, dtype):
    return torch.zeros((B, Cc, H, W), dtype=dtype, device=DEV).contiguous(memory_format=CL)


def scratch(n):
    return torch.empty(max(int(n), 16), dtype=torch.uint8, device=DEV)


def gdn_params(L, tag, Cc):
    beta = rnd(tag + "b", (Cc,), 0.5, 1.5).to(DEV)
    gamma = (rnd(tag + "g", (Cc, Cc), 0.0, 0.02) + 0.1 * torch.eye(Cc)).to(DEV)
    return beta, gamma


def packed_gdn(L, tag):
    beta, gamma = gdn_params(L, tag, 128)
    gp = torch.empty(2 * 128 * 128, dtype=BF, device=DEV)
    bp = torch.empty(128, dtype=torch.float32, device=DEV)
    glo = torch.empty(128 * 128, dtype=BF, device=DEV)
    L.call("hesic_gdn_pack_params", L.ptr(beta), L.ptr(gamma), 1e-6, L.ptr(gp), L.ptr(bp), 128, L.stream())
    L.call("hesic_gdn_pack_params_lo", L.ptr(gamma), L.ptr(glo), 128, L.stream())
    return gp, glo, bp


def test_igemm_options_stay_with_their_call(L):
    """B = 1, 8 x 8, 32 -> 128 3 x 3 in bfloat16: the smallest shape every implicit-GEMM entry point accepts."""
    st, lib = L.stream(), L.lib()
    Cin, Cout, k = 32, 128, 3
    BAD = "output size does not match"

    def pack(w):
        co, ci = w.shape[:2]
        wp = torch.empty(k * k * co * ci, dtype=BF, device=DEV)
        L.call("hesic_pack_conv_weight", L.ptr(w), None, L.ptr(wp), co, ci, k, k, 0, 0, L.H16, st)
        return wp

    def desc(cout=Cout, x_ps=Cin, y_ps=Cout):
        return L.ConvDesc(1, 8, 8, Cin, 8, 8, cout, k, k, 1, 1, 0, L.H16, 0, 0, x_ps, 0, y_ps, 0, 0)

    xf = rnd("x", (1, Cin, 8, 8), -2, 2).to(DEV)
    x = xf.to(BF).contiguous(memory_format=CL)
    xh = torch.cat((x, (xf - x.float()).to(BF)), 1).contiguous(memory_format=CL)          # [hi | lo] per pixel
    wp = pack(rnd("w", (Cout, Cin, k, k), -0.1, 0.1).to(DEV))
    wp2 = pack(rnd("w2", (2 * Cout, Cin, k, k), -0.1, 0.1).to(DEV))
    wph = pack(rnd("wh", (Cout, 2 * Cin, k, k), -0.1, 0.1).to(DEV))
    bias = rnd("b", (2 * Cout,)).to(DEV)
    gp, glo, bp = packed_gdn(L, "ig")
    y1, y2, ypre = nhwc(1, Cout, 8, 8, BF), nhwc(1, 2 * Cout, 8, 8, BF), nhwc(1, Cout, 8, 8, BF)
    y32 = nhwc(1, Cout, 8, 8, torch.float32)
    d = desc()
    ws, ws32, wsh = (scratch(f(C.byref(dd))) for f, dd in ((lib.hesic_conv2d_ws_bytes, d), (lib.hesic_conv2d_f32out_ws_bytes, d),
                                                          (lib.hesic_conv2d_hilo_ws_bytes, desc(x_ps=2 * Cin))))

    def plain():
        y = nhwc(1, Cout, 8, 8, BF)
        L.call("hesic_conv2d_forward", C.byref(d), L.ptr(x), L.ptr(wp), L.ptr(bias), L.ptr(y), st)
        return y

    def hilo():
        y32.zero_()
        L.call("hesic_conv2d_forward_hilo", *hilo_args(desc(x_ps=2 * Cin)))
        return y32.clone()

    def hilo_args(dd):
        return (C.byref(dd), L.ptr(xh), L.ptr(wph), L.ptr(bias), None, None, None, 0, None, 0, L.ptr(y32), Cout, 0, L.ptr(wsh), wsh.numel(), st)

    # name, descriptor, arguments behind the descriptor
    siblings = [
        ("hesic_conv2d_forward_ws", d, (L.ptr(x), L.ptr(wp), L.ptr(bias), L.ptr(y1), L.ptr(ws), ws.numel(), st)),
        ("hesic_conv2d_forward_f32out", d, (L.ptr(x), L.ptr(wp), L.ptr(bias), L.ptr(y1), L.ptr(y32), Cout, 0, L.ptr(ws32), ws32.numel(), st)),
        ("hesic_conv2d_forward_grouped", desc(cout=2 * Cout, y_ps=2 * Cout),
         (2, 0, L.ACT_RELU, Cout, L.ptr(x), L.ptr(wp2), L.ptr(bias), L.ptr(y2), None, 0, 0, st)),
        ("hesic_conv2d_gdn_forward", d, (L.ptr(x), L.ptr(wp), L.ptr(bias), L.ptr(gp), L.ptr(bp), 0, L.ptr(y1), st)),
        ("hesic_conv2d_gdn_forward_train", d, (L.ptr(x), L.ptr(wp), L.ptr(bias), L.ptr(gp), L.ptr(bp), 1, L.ptr(y1), L.ptr(ypre), st)),
        ("hesic_conv2d_forward_hilo", desc(x_ps=2 * Cin), hilo_args(d)[1:]),
        ("hesic_conv2d_forward_hilo_w1", desc(x_ps=2 * Cin), hilo_args(d)[1:]),
        ("hesic_conv2d_forward_hilo", desc(x_ps=2 * Cin, y_ps=2 * Cout),
         (L.ptr(xh), L.ptr(wph), L.ptr(bias), L.ptr(gp), L.ptr(glo), L.ptr(bp), 0, L.ptr(y2), 0, None, 0, 0, None, 0, st)),
        ("hesic_conv2d_gdn_forward_hilo_out", desc(y_ps=2 * Cout), (L.ptr(x), L.ptr(wp), L.ptr(bias), L.ptr(gp), L.ptr(glo), L.ptr(bp), 0, L.ptr(y2), st)),
    ]
    first = plain()
    torch.cuda.synchronize()
    assert float(first.float().abs().max()) > 0.1
    for name, dd, args in siblings:
        L.call(name, C.byref(dd), *args)
        refused(L, BAD, name, C.byref(with_field(dd, Ho=9)), *args)
        assert torch.equal(plain(), first), f"hesic_conv2d_forward after {name}"

    # the accumulator scale: taken by the next hi/lo launch, refused or not
    base = hilo()
    L.call("hesic_conv2d_hilo_set_acc_scale", 0.25)
    scaled = hilo()
    assert not torch.equal(scaled, base)
    assert torch.equal(hilo(), base)
    L.call("hesic_conv2d_hilo_set_acc_scale", 0.25)
    refused(L, BAD, "hesic_conv2d_forward_hilo", *hilo_args(with_field(desc(x_ps=2 * Cin), Ho=9)))
    assert torch.equal(hilo(), base), "a hi/lo launch after a refused hi/lo launch runs at scale 1"
    assert torch.equal(plain(), first)


def test_sconv_options_stay_with_their_call(L):
    """The cat stage (B = 1, 16 x 128, 6 -> 3 5 x 5) with and without its (I)GDN, and the two image-side stages with and without their
    prepacked weight image (128 -> 3 transposed at 32 x 32, 3 -> 128 + GDN at 64 x 64)."""
    from hesic_amd import functional as Fn
    st = L.stream()

    def bad(d):
        return with_field(d, Ho=d.Ho + 1)

    # ---- hesic_sconv2d_forward_cat / _cat_gdn
    xa, xb = rnd("xa", (1, 3, 16, 128)).to(DEV), rnd("xb", (1, 3, 16, 128)).to(DEV)
    w, bias = rnd("wc", (3, 6, 5, 5), -0.2, 0.2).to(DEV), rnd("bc", (3,)).to(DEV)
    beta, gamma = gdn_params(L, "cat", 3)
    xbs = (C.c_int64 * 4)(*xb.stride())
    y = torch.zeros((1, 3, 16, 128), device=DEV)
    d = Fn._sdesc(xa, y, 6, 3, 5, 1, 2, False)

    def cat(out):
        L.call("hesic_sconv2d_forward_cat", C.byref(d), L.ptr(xa), L.ptr(xb), xbs, L.F32, 3, L.ptr(w), L.ptr(bias), L.ptr(out), st)
        return out

    def cat_gdn(dd, on_input, out):
        return ("hesic_sconv2d_forward_cat_gdn", C.byref(dd), L.ptr(xa), L.ptr(xb), xbs, L.F32, 3, L.ptr(w), L.ptr(bias), L.ptr(beta), L.ptr(gamma),
                1e-6, 0, on_input, L.ptr(out), st)

    first = cat(torch.zeros_like(y)).clone()
    for on_input in (0, 1):
        yg = torch.zeros_like(y)
        L.call(*cat_gdn(d, on_input, yg))
        refused(L, "conv output size mismatch", *cat_gdn(bad(d), on_input, yg))
        assert not torch.equal(yg, first)
        assert torch.equal(cat(torch.zeros_like(y)), first), "hesic_sconv2d_forward_cat after _cat_gdn applies no GDN"

    # ---- hesic_sconv2d_forward / _forward_prepacked
    x = rnd("x4", (1, 128, 32, 32)).to(DEV, BF).contiguous(memory_format=CL)
    w4, b4 = rnd("w4", (128, 3, 5, 5), -0.1, 0.1).to(DEV), rnd("b4", (3,)).to(DEV)
    y4 = torch.zeros((1, 3, 64, 64), device=DEV)
    d4 = Fn._sdesc(x, y4, 128, 3, 5, 2, 2, True)
    img = torch.empty(24576, dtype=torch.uint8, device=DEV)
    L.call("hesic_sconv_pack_weight_image", 1, L.ptr(w4), None, L.ptr(img), st)

    def conv4(out):
        L.call("hesic_sconv2d_forward", C.byref(d4), L.ptr(x), L.ptr(w4), L.ptr(b4), L.ptr(out), st)
        return out

    first = conv4(torch.zeros_like(y4)).clone()
    yp = torch.zeros_like(y4)
    L.call("hesic_sconv2d_forward_prepacked", C.byref(d4), L.ptr(x), L.ptr(w4), L.ptr(img), L.ptr(b4), L.ptr(yp), st)
    refused(L, "transposed output size mismatch", "hesic_sconv2d_forward_prepacked", C.byref(bad(d4)), L.ptr(x), L.ptr(w4), L.ptr(img), L.ptr(b4), L.ptr(yp), st)
    assert torch.equal(conv4(torch.zeros_like(y4)), first), "hesic_sconv2d_forward after _forward_prepacked"

    # ---- hesic_sconv2d_gdn_forward / _gdn_forward_prepacked
    x1 = rnd("x1", (1, 3, 64, 64)).to(DEV)
    w1, b1 = rnd("w1", (128, 3, 5, 5), -0.2, 0.2).to(DEV), rnd("b1", (128,)).to(DEV)
    gp, _, bp = packed_gdn(L, "s1")
    y1 = nhwc(1, 128, 32, 32, BF)
    d1 = Fn._sdesc(x1, y1, 3, 128, 5, 2, 2, False)
    img1 = torch.empty(65536, dtype=torch.uint8, device=DEV)
    L.call("hesic_sconv_pack_weight_image", 0, L.ptr(w1), L.ptr(gp), L.ptr(img1), st)

    def conv1(out):
        L.call("hesic_sconv2d_gdn_forward", C.byref(d1), L.ptr(x1), L.ptr(w1), L.ptr(b1), L.ptr(gp), L.ptr(bp), 0, L.ptr(out), st)
        return out

    first = conv1(torch.zeros_like(y1)).clone()
    yp = torch.zeros_like(y1)
    args = (L.ptr(x1), L.ptr(w1), L.ptr(img1), L.ptr(b1), L.ptr(gp), L.ptr(bp), 0, L.ptr(yp), None, st)
    L.call("hesic_sconv2d_gdn_forward_prepacked", C.byref(d1), *args)
    refused(L, "conv output size mismatch", "hesic_sconv2d_gdn_forward_prepacked", C.byref(bad(d1)), *args)
    assert torch.equal(conv1(torch.zeros_like(y1)), first), "hesic_sconv2d_gdn_forward after _gdn_forward_prepacked"


def test_gdn_backward_options_stay_with_their_call(L):
    """P = 256 pixels, C = 128, bfloat16 (the fused form, the only one with block partials)."""
    st = L.stream()
    P = 256
    x = rnd("gx", (1, 128, 16, 16), -2, 2).to(DEV, BF).contiguous(memory_format=CL)
    gy = rnd("gg", (1, 128, 16, 16)).to(DEV, BF).contiguous(memory_format=CL)
    beta, gamma = gdn_params(L, "gb", 128)
    ws = scratch(L.lib().hesic_gdn_backward_ws_bytes(P, 128))

    def plain():
        dx, db, dg = torch.zeros_like(x), torch.full((128,), -0.5, device=DEV), torch.full((128, 128), 0.25, device=DEV)      # overwritten, not added to
        L.call("hesic_gdn_backward", L.ptr(x), L.ptr(gy), L.ptr(beta), L.ptr(gamma), L.ptr(dx), L.ptr(db), L.ptr(dg), L.ptr(ws), P, 128, 0, 1e-6, L.H16, st)
        return dx, db, dg

    def same(a, b):
        return all(torch.equal(p, q) for p, q in zip(a, b))

    first = plain()
    dx, db, dg = torch.zeros_like(x), torch.full((128,), -0.5, device=DEV), torch.full((128, 128), 0.25, device=DEV)
    acc = lambda p: ("hesic_gdn_backward_acc", L.ptr(x), L.ptr(gy), L.ptr(beta), L.ptr(gamma), L.ptr(dx), L.ptr(db), L.ptr(dg), 1, L.ptr(ws), p, 128, 0, 1e-6, L.H16, st)
    L.call(*acc(P))
    assert torch.allclose(dg, first[2] + 0.25, rtol=1e-5, atol=1e-6) and torch.allclose(db, first[1] - 0.5, rtol=1e-5, atol=1e-6)      # it did accumulate
    refused(L, "bad arguments", *acc(0))
    assert same(plain(), first), "hesic_gdn_backward after hesic_gdn_backward_acc(accumulate = 1) overwrites"
    part = lambda c: ("hesic_gdn_backward_partial", L.ptr(x), L.ptr(gy), L.ptr(beta), L.ptr(gamma), L.ptr(dx), L.ptr(ws), P, c, 0, 1e-6, L.H16, st)
    L.call(*part(128))
    refused(L, "only the fused 128-channel 16-bit form", *part(3))
    assert same(plain(), first), "hesic_gdn_backward after hesic_gdn_backward_partial finishes the parameter gradients"


def test_wgrad_options_stay_with_their_call(L):
    """The weight gradient of the 8 x 8 layer of the igemm test."""
    st = L.stream()
    Cin, Cout, k = 32, 128, 3
    x = rnd("wx", (1, Cin, 8, 8), -2, 2).to(DEV, BF).contiguous(memory_format=CL)
    gy = rnd("wg", (1, Cout, 8, 8)).to(DEV, BF).contiguous(memory_format=CL)
    d = L.ConvDesc(1, 8, 8, Cin, 8, 8, Cout, k, k, 1, 1, 0, L.H16, 0, 0, Cin, 0, Cout, 0, 0)
    nws = int(L.lib().hesic_conv2d_wgrad_ws_bytes(C.byref(d)))
    ws, ws2 = scratch(nws), scratch(nws)

    def direct():
        dw, db = torch.full((Cout, Cin, k, k), 7.0, device=DEV), torch.full((Cout,), 7.0, device=DEV)
        L.call("hesic_conv2d_wgrad_direct", C.byref(d), L.ptr(x), L.ptr(gy), L.ptr(dw), L.ptr(db), 0, L.ptr(ws), nws, st)
        return dw, db

    dw0, db0 = direct()
    assert not bool((dw0 == 7.0).any()) and not bool((db0 == 7.0).any())
    L.call("hesic_conv2d_wgrad_partial", C.byref(d), L.ptr(x), L.ptr(gy), L.ptr(ws2), nws, st)
    refused(L, "channels must be multiples of 8", "hesic_conv2d_wgrad_partial", C.byref(with_field(d, Cin=36)), L.ptr(x), L.ptr(gy), L.ptr(ws2), nws, st)
    dw1, db1 = direct()
    assert torch.equal(dw1, dw0) and torch.equal(db1, db0), "hesic_conv2d_wgrad_direct after hesic_conv2d_wgrad_partial still finishes into dw"

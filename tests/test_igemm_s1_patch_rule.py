"""hesic_conv2d_variant is host logic: which launches take the stride-1 5 x 5 kernel that keeps its input patch resident in LDS
(igemm_s1p_kernel, csrc/conv_igemm.hip; reported as {256, 128, 64, 1}).  HESIC_IGEMM_S1_PATCH = 0: never; 1 (default): auto -- the
256-pixel grid fills the chip (>= 256 blocks in >= 32 pixel tiles, rounds of the 256 CUs >= 70 % full) and the 16 x 16 tiles cover the map
without hanging over by more than 1/8; 2: whenever the shape is eligible (5 x 5, pad 2, stride 1, not transposed, 128 input channels, no tap mask)."""
import ctypes as C
import os

import pytest

ENV = "HESIC_IGEMM_S1_PATCH"
NEW = [256, 128, 64, 1]


def _lib():
    from hesic_amd import _lib as L
    if not os.path.exists(L.LIB_PATH):
        import __graft_entry__ as ge
        ge.build()
    return L


@pytest.fixture
def mode():
    prev = os.environ.get(ENV)

    def set_mode(m):
        if m is None:
            os.environ.pop(ENV, None)
        else:
            os.environ[ENV] = str(m)
    yield set_mode
    set_mode(prev)


def variant(B, H, W, Cin=128, Cout=960, k=5, stride=1, transposed=0, tap_mask=0, x_ps=None):
    L = _lib()
    l = L.lib()
    if transposed:
        Ho, Wo = H * stride, W * stride
    else:
        Ho, Wo = (H + 2 * (k // 2) - k) // stride + 1, (W + 2 * (k // 2) - k) // stride + 1
    d = L.ConvDesc(B, H, W, Cin, Ho, Wo, Cout, k, k, stride, k // 2, transposed, L.H16, 0, 0, x_ps or Cin, 0, Cout, 0, tap_mask)
    v = (C.c_int32 * 4)()
    assert l.hesic_conv2d_variant(C.byref(d), v) == 0, l.hesic_last_error()
    return list(v)


def test_auto_mode_takes_the_workload_launches(mode):
    for m in (None, 1):                                             # unset == auto
        mode(m)
        assert variant(8, 32, 32, Cout=2048, x_ps=256) == NEW       # gmm_sigma | gmm_means of gmm_hyper_y1 / _y2, grouped: 512 blocks
        assert variant(8, 32, 32, Cout=960) == NEW                  # gmm_weights of gmm_hyper_y2: 256 blocks


def test_auto_mode_leaves_the_shapes_that_do_not_gain(mode):
    mode(1)
    assert variant(4, 56, 68, Cout=2048, x_ps=256)[0] != 256        # config C5 (896 x 1088): 20 tiles of 256 for 3808 pixels
    assert variant(4, 56, 68, Cout=960)[0] != 256
    assert variant(4, 32, 32, Cout=960)[0] != 256                   # B = 4: 128 blocks, half the CUs idle
    assert variant(4, 32, 32, Cout=2048, x_ps=256)[0] != 256        # B = 4 grouped: 256 blocks of 16 pixel tiles; the HESIC+ B = 4 step did not gain
    assert variant(1, 32, 32, Cout=2048, x_ps=256)[0] != 256        # B = 1: 64 blocks
    assert variant(1, 32, 32, Cout=960)[0] != 256
    assert variant(8, 32, 32, Cout=1280)[0] != 256                  # 320 blocks: the second round of the 256 CUs would be 25 % full


def test_mode_0_never_and_mode_2_whenever_eligible(mode):
    mode(0)
    assert variant(8, 32, 32, Cout=2048, x_ps=256)[0] != 256
    assert variant(8, 32, 32, Cout=960)[0] != 256
    mode(2)
    assert variant(1, 5, 7, Cout=128) == NEW
    assert variant(1, 32, 32, Cout=960) == NEW


@pytest.mark.parametrize("m", [0, 1, 2])
def test_other_shapes_never_take_it(m, mode):
    mode(m)
    assert variant(8, 64, 64, Cout=128, stride=2)[0] != 256                  # stride 2
    assert variant(8, 32, 32, Cout=128, stride=2, transposed=1)[0] != 256    # transposed
    assert variant(8, 32, 32, Cout=128, stride=1, transposed=1)[0] != 256
    assert variant(8, 32, 32, Cin=192, Cout=960)[0] != 256                   # Cin != 128
    assert variant(8, 32, 32, Cin=64, Cout=960)[0] != 256
    assert variant(8, 32, 32, Cout=960, k=3)[0] != 256                       # 3 x 3
    assert variant(8, 32, 32, Cout=960, tap_mask=(1 << 12) - 1)[0] != 256    # MaskedConv2d: a raster-order prefix of the taps
    assert variant(8, 32, 32, Cout=192)[0] != 256                            # cout tiles of 64

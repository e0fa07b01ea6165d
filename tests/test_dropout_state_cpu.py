"""The dropout state in device memory, without a GPU: the NumPy restatement (tests/dropout_state_ref.py) against the by-value stream of
``functional.dropout_args``, the host words ``Net.dropout_on_device`` uploads, and the ``--graphed`` parser rules."""
import numpy as np
import pytest
import torch

import dropout_state_ref as S
import homography_net_ref as R
from hesic_amd import functional as Fn
from hesic_amd import homography_train

CASES = [(0, 0), (7, 3), (0x0123456789ABCDEF, 41), (0xFFFFFFFFFFFFFFFF, 0xFFFFFFFE), (1 << 32, 0xFFFFFFFF)]


@pytest.mark.parametrize("seed,step", CASES)
def test_take_is_use_then_increment(seed, step):
    state = S.state_words(seed, step)
    taken, after = S.take(state)
    assert taken.dtype == after.dtype == np.uint32
    assert S.seed_step(taken) == (seed, step)
    assert S.seed_step(after) == (seed, (step + 1) & 0xFFFFFFFF) and after[3] == taken[3] == 0
    assert np.array_equal(state, S.state_words(seed, step))            # the argument is left alone
    # three takes: the steps the host counter of Net._forward_train would pass by value
    steps = []
    for _ in range(3):
        t, state = S.take(state)
        steps.append(int(t[2]))
    assert steps == [(step + k) & 0xFFFFFFFF for k in range(3)]


def test_take_wraps_at_two_to_the_32():
    taken, after = S.take(S.state_words(5, 0xFFFFFFFF))
    assert int(taken[2]) == 0xFFFFFFFF and int(after[2]) == 0 and (int(after[0]), int(after[1])) == (5, 0)


@pytest.mark.parametrize("seed,step", CASES)
def test_state_fed_mask_is_the_by_value_stream(seed, step):
    taken, _ = S.take(S.state_words(seed, step))
    for site, (B, Fdim) in enumerate(((3, 64), (2, 36))):
        thr, scale, seed_v, step_v, site_v = Fn.dropout_args(0.5, seed, step, site)
        assert (seed_v, step_v, site_v) == (*S.seed_step(taken), site)
        want = R.dropout_words(B, Fdim, seed_v, step_v, site_v)
        assert np.array_equal(S.dropout_words(B, Fdim, taken, site), want)
        assert np.array_equal(S.keep_mask(B, Fdim, 0.5, taken, site), want >= np.uint32(thr))
        assert torch.equal(torch.from_numpy(S.keep_mask(B, Fdim, 0.5, taken, site)), R.keep_mask(B, Fdim, 0.5, seed, step, site))
        assert (thr, scale) == R.thr_scale(0.5)
    x = torch.linspace(-2, 2, 2 * 9 * 4).reshape(2, 4, 3, 3)
    assert torch.equal(S.flatten_dropout(x, 0.5, taken, 0), R.flatten_dropout(x, 0.5, seed, step, 0))
    assert torch.equal(S.flatten_dropout_backward(x.reshape(2, -1), x.shape, 0.5, taken, 1), R.flatten_dropout_backward(x.reshape(2, -1), x.shape, 0.5, seed, step, 1))


@pytest.mark.parametrize("seed,step", CASES)
def test_the_uploaded_words_are_the_reference_state(seed, step):
    words = Fn._dropout_words(seed, step)
    assert words.dtype == np.int32 and np.array_equal(words.view(np.uint32), S.state_words(seed, step))


def test_state_args_refuse_what_is_not_a_taken_state():
    for bad in (None, torch.zeros(4, dtype=torch.int32), torch.zeros(3, dtype=torch.int32)):
        with pytest.raises(ValueError, match="taken must be a contiguous 16-byte device tensor"):
            Fn.dropout_state_args(0.5, bad, 0)


def test_parser_graphed(tmp_path, capsys):
    assert homography_train.parser().parse_args(["root"]).graphed is False
    for cache in ("device", "stream"):
        a = homography_train.parser().parse_args(["root", "--graphed", "--cache", cache, "--supervision", "synthetic"])
        assert a.graphed is True and a.cache == cache
    for argv in (["--graphed"], ["--graphed", "--cache", "host"]):
        with pytest.raises(SystemExit) as e:
            homography_train.main([str(tmp_path)] + argv)
        assert e.value.code == 2
    assert "--graphed needs --cache device or --cache stream" in capsys.readouterr().err

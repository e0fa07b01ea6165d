"""NumPy statement of the dropout state in device memory (include/hesic_homography_net.h; a plain module, not a conftest).  No GPU.

The state is four uint32 words ``{seed lo, seed hi, step, reserved}``.  ``take`` is ``hesic_dropout_state_take``: the four words as they
stand, and the state with ``step + 1`` modulo 2^32.  ``keep_mask`` / ``flatten_dropout`` / ``flatten_dropout_backward`` are what the ``_state``
entries compute from a taken state: the Philox stream of tests/homography_net_ref.py keyed by its first two words, with its third word as
the counter's step."""
import numpy as np

import homography_net_ref as R


def state_words(seed, step, reserved=0):
    """(4,) uint32: the state for a 64-bit ``seed`` and a 32-bit ``step``."""
    seed, step = int(seed) & 0xFFFFFFFFFFFFFFFF, int(step) & 0xFFFFFFFF
    return np.array([seed & 0xFFFFFFFF, seed >> 32, step, int(reserved) & 0xFFFFFFFF], dtype=np.uint32)


def take(state):
    """``(taken, state afterwards)``: a copy of the four words, and the state with its step incremented modulo 2^32."""
    state = np.asarray(state, dtype=np.uint32)
    assert state.shape == (4,)
    after = state.copy()
    after[2] = np.uint32((int(state[2]) + 1) & 0xFFFFFFFF)
    return state.copy(), after


def seed_step(taken):
    """``(seed, step)`` as Python ints."""
    return int(taken[0]) | (int(taken[1]) << 32), int(taken[2])


def dropout_words(B, Fdim, taken, site):
    """(B, F) uint32: Philox4x32-10(counter = (q lo, q hi, taken[2], site), key = (taken[0], taken[1]))."""
    q = np.arange(B * Fdim // 4, dtype=np.uint64)
    ctr = np.stack([q & np.uint64(0xFFFFFFFF), q >> np.uint64(32), np.full_like(q, int(taken[2])), np.full_like(q, site)], -1)
    return R.philox4x32_10(ctr, (int(taken[0]), int(taken[1]))).reshape(B, Fdim)


def keep_mask(B, Fdim, p, taken, site):
    """(B, F) bool array: True where the element is kept."""
    return dropout_words(B, Fdim, taken, site) >= np.uint32(R.thr_scale(p)[0])


def flatten_dropout(x, p, taken, site):
    return R.flatten_dropout(x, p, *seed_step(taken), site)


def flatten_dropout_backward(gy, shape, p, taken, site):
    return R.flatten_dropout_backward(gy, shape, p, *seed_step(taken), site)

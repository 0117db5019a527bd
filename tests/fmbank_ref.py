"""Shared by tests/test_fmbank_cpu.py and tests/test_fmbank_gpu.py: the expected values of include/rtlws_fmbank.h --
tests/ddc_ref.py per channel fed to the oracle's per-block chain (tests/fm_ref.py) -- and the test inputs."""
import numpy as np

import ddc_ref
import fm_ref

P = ddc_ref.P
SPECIAL_WORDS = (0, 1, -1, -32768, 32767)
# (cic_r, channels): both sides of a column-tile border (8 | 9) and of a K step (16 | 17), every instantiation
# (8, 10, 12, generic); one column tile, two of which the second holds one channel, and four full ones.  Three column
# tiles, a second one that is full or partly filled and every other C = 1 .. 32 run from tests/ddc_family_channels.py
BANKS = [(1, 1), (7, 9), (8, 8), (8, 32), (10, 1), (12, 9), (16, 8), (17, 2), (128, 32)]

# the banks of the multi-tile suite (fm_ref.tile_cases): every case at a compile-time factor with two column tiles of
# which the second holds one channel; the cases whose stage-1 map skips also at the other instantiations
TILE_BANK = (8, 9)
SKIP_BANKS = [(10, 2), (12, 8), (7, 9)]

_cache = {}


def words_for(C, seed):
    """The recipe of tests/test_ddc_gpu.py: seeded random words, the special ones at positions 1 .. as far as they
    fit, and the last channel on the first one's word."""
    w = [int(k) for k in np.random.default_rng(seed).integers(-P // 2, P // 2, C)]
    for i, s in enumerate(SPECIAL_WORDS):
        if 1 + i < C - 1:
            w[1 + i] = s
    if C >= 2:
        w[C - 1] = w[0]
    return w


def states_for(C, seed):
    """fm_ref.random_state(seed + c) for channel c -> f32 [C, 21]."""
    return np.stack([fm_ref.random_state(seed + c) for c in range(C)])


def expected(oracle, iq, R, words, L, states, first=0, key=None):
    """(audio f32 [C, nblocks * quarter], states out f32 [C, 21]): ddc_ref per channel, then the oracle's chain.
    With a key the result is computed once and shared (it is returned read-only)."""
    if key is not None and key in _cache:
        return _cache[key]
    streams = ddc_ref.ddc_ref(iq, R, words, first)
    audio, out = [], []
    for c in range(len(words)):
        a, s = fm_ref.oracle_chain(oracle, streams[c], L, states[c])
        audio.append(a)
        out.append(s)
    res = (np.stack(audio), np.stack(out))
    for a in res:
        a.setflags(write=False)
    if key is not None:
        _cache[key] = res
    return res


def case_inputs(case, R, C):
    """(capture, tuning words, carried states) of an fm_ref.tile_cases case at a bank of C channels and factor R: the
    last channel is the first one's station, word and state."""
    seed = 1000 * case.block_len + 10 * R + C
    words = words_for(C, seed)
    states = states_for(C, seed + 1)
    states[C - 1] = states[0]
    return ddc_ref.random_iq(case.nblocks * case.block_len * R, seed + 2), words, states


def tile_bank_runs(t):
    """(case, R, C) of every launch of the multi-tile suite"""
    cases = fm_ref.tile_cases(t)
    return [(c,) + TILE_BANK for c in cases] + [(c, R, C) for R, C in SKIP_BANKS for c in cases if c.residue in (1, 3)]


def matrix_shape(t):
    """(block_len, nblocks) for a tile of t audio samples: two full tiles and a remainder, the block borders inside
    the tiles, an odd half.  1030 x 5 at t = 512, 518 x 5 at t = 256."""
    L, nb = 2 * t + 6, 5
    half, quarter = L // 2, L // 4
    assert half % 2 == 1 and 2 * t < nb * quarter < 3 * t and all((b * quarter) % t for b in range(1, nb))
    return L, nb


# ---- the inputs that reach every branch of atan2_approx (the word-0 channel is the plain block sum) --------------

BRANCH_R, BRANCH_C, BRANCH_L, BRANCH_NB = 8, 8, 262, 2


def branch_words():
    w = words_for(BRANCH_C, seed=77)
    w[0] = 0
    w[BRANCH_C - 1] = 0
    return w


def branch_captures():
    """name -> uint8 capture of BRANCH_NB blocks of BRANCH_L decimated samples at cic_r = BRANCH_R.  "axes": random
    bytes with three stretches of 40 decimated samples inside the first block and across the block border -- re bytes
    all 128 with im above 128, re all 128 with im below 128, every byte 128 -- so that the word-0 channel has x == 0
    with y > 0, y < 0 and y == 0.  "all128": every byte 128, every channel's stream is zero."""
    n = BRANCH_L * BRANCH_NB * BRANCH_R
    rng = np.random.default_rng(78)
    axes = rng.integers(0, 256, size=(n, 2), dtype=np.uint8)
    span = 40 * BRANCH_R
    for start_dec, lo, hi in ((50, 129, 256), (130, 0, 128), (BRANCH_L - 20, 128, 129)):
        s = start_dec * BRANCH_R
        axes[s:s + span, 0] = 128
        axes[s:s + span, 1] = rng.integers(lo, hi, span)
    return {"axes": axes, "all128": np.full((n, 2), 128, dtype=np.uint8)}

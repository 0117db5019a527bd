"""Shared by tests/test_fmfir_cpu.py and tests/test_fmfir_gpu.py: the expected values of include/rtlws_fmfir.h --
tests/ddcfir_ref.py per channel fed to the oracle's per-block chain (tests/fm_ref.py), in the shape of
tests/fmbank_ref.py's expected -- the test inputs, and the end-to-end measurement of what the filter buys a
discriminator.  Nothing here uses the code under test."""
import numpy as np

import ddcfir_ref
import fm_ref
import fmbank_ref

P = ddcfir_ref.P

# (decim, ntaps, channels, designed taps) of the bank matrix
BANKS = [(1, 1, 1, False), (4, 32, 8, False), (8, 64, 9, False), (12, 96, 32, True), (10, 80, 2, False), (7, 17, 9, False),
         (12, 16, 8, False), (12, 17, 8, False), (16, 5, 3, False), (3, 256, 1, False), (128, 256, 32, False)]
TILE_BANK = (8, 40, 9)
SKIP_BANKS = [(10, 30, 2), (7, 17, 9)]

_cache = {}


def samples_needed(R, L, block_len, nblocks):
    return ddcfir_ref.samples_needed(R, L, nblocks * block_len)


def taps_for(R, L, seed, designed=False):
    """ddcfir_ref.design, or random taps with both ends of the range among them (as far as L holds them)."""
    if designed:
        return ddcfir_ref.design(R, L)
    h = ddcfir_ref.random_taps(L, seed)
    h[0] = ddcfir_ref.MAX_TAP
    if L >= 2:
        h[L - 1] = -ddcfir_ref.MAX_TAP
    return h


def expected(oracle, iq, R, taps, words, L, states, out_shift=14, first=0, nblocks=None, key=None):
    """(audio f32 [C, nblocks * quarter], states out f32 [C, 21]): ddcfir_ref per channel, then the oracle's chain.
    With a key the result is computed once and shared (it is returned read-only)."""
    if key is not None and key in _cache:
        return _cache[key]
    dec_len = None if nblocks is None else nblocks * L
    streams = ddcfir_ref.ddcfir_ref(iq, R, taps, words, out_shift, first, dec_len)
    assert streams.shape[1] % L == 0
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


def inputs(R, L, C, block_len, nblocks, seed):
    """(capture of exactly the samples needed, words, states): fmbank_ref's recipes, the last channel the first one's
    station."""
    words = fmbank_ref.words_for(C, seed)
    states = fmbank_ref.states_for(C, seed + 1)
    if C >= 2:
        states[C - 1] = states[0]
    return ddcfir_ref.random_iq(samples_needed(R, L, block_len, nblocks), seed + 2), words, states


def tile_bank_runs(t):
    """(case, R, L, C) of every launch of the multi-tile suite"""
    cases = fm_ref.tile_cases(t)
    return [(c,) + TILE_BANK for c in cases] + [(c,) + b for b in SKIP_BANKS for c in cases if c.residue in (1, 3)]


def extend(iq, extra, fill_seed=79):
    """A capture of fmbank_ref's (nblocks * block_len * R samples) by `extra` more samples (ntaps - decim of them)."""
    if extra <= 0:
        return iq
    more = np.random.default_rng(fill_seed).integers(0, 256, size=(extra, 2), dtype=np.uint8)
    return np.concatenate([iq, more])


# ---- stage A at the window forms of the filtered down-converter ---------------------------------------------------
# fmfir_bank.hip's phases<ALIGNED> shares the operand builder and the window loader with ddcfir_bank.hip, but the loop
# around them is its own: the next K step's window loaded ahead of the MFMAs (one step past the last), the block-phasor
# lookups in front of the K loop, lanes masked by idx < np && g >= 0, row tiles dealt in pairs per wavefront.  This
# matrix runs it at every (decim, ntaps) at which tests/test_ddcfir_gpu.py holds ddcfir_bank_kernel to the restatement
# (ddcfir_ref.R_AXIS x l_axis) and at STAGE_A_EXTRA; the other axes are cycled over the pairs of an instantiation.
# tests/test_fmfir_cpu.py holds it to its conditions.

STAGE_A_EXTRA = ((8, 24),)          # two K steps under the aligned instantiation: the axes' aligned pairs have 1, 4, 6, 8, 16
STAGE_A_C = (1, 2, 8, 9, 17, 24, 32)
STAGE_A_SHIFTS = (0, 9, 14)
STAGE_A_FIRSTS = (0, 123456789, (1 << 40) + 12345)
STAGE_A_BYTES = ("random", "full scale")
STAGE_A_TAPS = ("random", "+max", "-max")
NP_CLASSES = {"1 .. 15": range(1, 16), "16": (16,), "17 .. 31": range(17, 32), "0": (0,)}


class StageACase(tuple):
    """(decim, ntaps, channels, out_shift, first_dec_index, bytes, taps, block_len, nblocks)"""
    R, L, C = (property(lambda s, i=i: s[i]) for i in range(3))
    shift, first, bytes, taps, block_len, nblocks = (property(lambda s, i=i: s[i]) for i in range(3, 9))
    id = property(lambda s: "R%d-L%d-C%d-s%d-%dx%d" % (s[0], s[1], s[2], s[3], s[7], s[8]))
    aligned = property(lambda s: ddcfir_ref.aligned(s[0], s[1]))
    product = property(lambda s: s[1] * s[2] * s[7] * s[8])          # what the restatement's time goes with


def stage_a_pairs():
    return [(R, L) for R in ddcfir_ref.R_AXIS for L in ddcfir_ref.l_axis(R)] + list(STAGE_A_EXTRA)


def stage_a_shapes(tile):
    """(block_len, nblocks): fm_ref.tile_cases' a3 (block_len 23, the shape the LDS capacities are derived for) cut to
    one tile and a part of a second, its b1 and b3 (the stage-1 map skips, borders in front of tiles, four tiles), and
    three blocks of 20, 22, 23 and 25 inside one tile."""
    cases = {(c.regime, c.residue): c for c in fm_ref.tile_cases(tile)}
    a3 = cases["a", 3]
    cut = tile // (a3.block_len // 4) + 1
    assert cut < a3.nblocks and tile < cut * (a3.block_len // 4) < 2 * tile
    return [(a3.block_len, cut), tuple(cases["b", 1][2:]), tuple(cases["b", 3][2:]), (20, 3), (22, 3), (23, 3), (25, 3)]


def stage_a_matrix(tile):
    """Every (decim, ntaps) of stage_a_pairs(); per instantiation the other axes cycle over its pairs: the channel
    counts with stride 1, the block shapes with stride 1 from the fourth on and one more step per round of the channel
    counts (two axes of seven: a channel count meets another shape in every round, and in the first round 17, 24 and
    32 channels meet the shapes of several tiles), the others with strides 2, 4, 3 and 5, none of which shares a factor
    with its axis' length."""
    shapes = stage_a_shapes(tile)
    count = {True: 0, False: 0}
    cases = []
    for R, L in stage_a_pairs():
        inst = ddcfir_ref.aligned(R, L)
        i = count[inst]
        count[inst] += 1
        cases.append(StageACase((R, L, STAGE_A_C[i % 7], STAGE_A_SHIFTS[(i // 2) % 3], STAGE_A_FIRSTS[(i // 4) % 3],
                                 STAGE_A_BYTES[(i // 3) % 2], STAGE_A_TAPS[(i // 5) % 3]) + shapes[(i + 3 + i // 7) % len(shapes)]))
    return cases


def np_residues(case, tile):
    """np mod 32 of every ordinary tile of a case's launch (fm_ref.tile_bounds): how the last pair of row tiles of
    stage A is masked"""
    nt = -(-case.nblocks * (case.block_len // 4) // tile)
    return [int(fm_ref.tile_bounds(t, case.block_len, case.nblocks, tile)["np"]) % 32 for t in range(nt)]


def stage_a_inputs(case, seed):
    """(capture of exactly the samples needed, taps, words, states) of a case"""
    R, L = case.R, case.L
    iq, words, states = inputs(R, L, case.C, case.block_len, case.nblocks, seed)
    if case.bytes == "full scale":
        iq = ddcfir_ref.full_scale_iq(iq.shape[0], seed + 2)
    if case.taps == "random":
        taps = taps_for(R, L, seed + 3)
    else:
        taps = np.full(L, ddcfir_ref.MAX_TAP if case.taps == "+max" else -ddcfir_ref.MAX_TAP, dtype=np.int16)
    return iq, taps, words, states


def composition_cases(tile):
    """One case per instantiation for the comparison with rtlws_ddcfir_run followed by rtlws_fm_audio_blocks on the
    device: the first with more than one tile and more than one column tile."""
    matrix = stage_a_matrix(tile)
    return [next(i for i, c in enumerate(matrix) if c.aligned == inst and c.C > 8 and c.nblocks * (c.block_len // 4) > tile)
            for inst in (True, False)]


# ---- why the filter matters, end to end (on the restatement, not the device) ------------------------------------

FM_R = ddcfir_ref.SELECTIVITY_R
FM_CENTRE = ddcfir_ref.SELECTIVITY_CENTRE
FM_OFFSET = ddcfir_ref.SELECTIVITY_OFFSET                  # the interferer: 1.5 output bandwidths off the centre
FM_BLOCK, FM_NBLOCKS = 400, 4                              # 1600 decimated samples, 400 audio samples
FM_WANTED_AMP, FM_INTERFERER_AMP = 30.0, 90.0              # 30 + 90 <= 127: the sum stays inside u8 without clipping
FM_TONE_CYCLES = 10                                        # audio tone: cycles over the capture's decimated samples
FM_DEVIATION = 0.25                                        # peak phase step per decimated sample, radians


def fm_capture(ntaps, interferer):
    """u8 capture: an FM-modulated audio tone on the channel's centre, and (interferer) a stronger unmodulated carrier
    FM_OFFSET words above it."""
    n = samples_needed(FM_R, ntaps, FM_BLOCK, FM_NBLOCKS)
    t = np.arange(n, dtype=np.float64)
    ndec = FM_BLOCK * FM_NBLOCKS
    # instantaneous frequency: centre + deviation * cos(tone); the phase is its running sum
    tone = 2.0 * np.pi * FM_TONE_CYCLES * t / (ndec * FM_R)
    phase = 2.0 * np.pi * FM_CENTRE * t / P + (FM_DEVIATION / FM_R) * np.cumsum(np.cos(tone))
    x = FM_WANTED_AMP * np.exp(1j * phase)
    if interferer:
        x = x + FM_INTERFERER_AMP * np.exp(2j * np.pi * ((FM_CENTRE + FM_OFFSET) * np.arange(n, dtype=np.int64) % P) / P)
    return (np.rint(np.stack([x.real, x.imag], axis=1)) + 128).astype(np.uint8)


def audio_error_db(oracle, taps):
    """Power of (audio with the interferer - audio without) over the power of the wanted audio tone, in dB, behind the
    channel filter `taps` at decimation FM_R.  The first quarter of the audio (the filters' and the chain's start) is
    left out of both."""
    taps = np.asarray(taps)
    state = np.zeros((1, fm_ref.STATE), dtype=np.float32)
    audio = []
    for interferer in (False, True):
        iq = fm_capture(taps.size, interferer)
        a, _ = expected(oracle, iq, FM_R, taps, [FM_CENTRE], FM_BLOCK, state, nblocks=FM_NBLOCKS)
        audio.append(a[0].astype(np.float64))
    skip = audio[0].size // 4
    clean, dirty = audio[0][skip:], audio[1][skip:]
    wanted = clean - clean.mean()
    return 10.0 * np.log10(((dirty - clean) ** 2).mean() / (wanted ** 2).mean())

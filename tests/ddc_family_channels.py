"""The channel counts of the tuned-channel family as data (rtl-ws_amd/csrc/ddc_bank.hip, ddcfir_bank.hip, fm_bank.hip,
fmfir_bank.hip): every C = 1 .. 32 at every code path of the four kernels, so that
every number of column tiles nct = ceil(C / 8) = 1 .. 4 meets every filling 1 .. 8 of the last one.
tests/test_ddc_family_channels_cpu.py holds the lists to their conditions; the four tests/test_*_gpu.py launch them.

One set of 32 tuning words and 32 carried states serves every launch: a bank of C channels gets the first C of each.
A channel's output depends on its own word and state only, so the expected value of a launch is the first C rows of
the 32-channel expected value of its path, computed once.  The words are pairwise different, so a channel stored in
another channel's row shows.

The shapes are the smallest at which the paths differ: the banks that store streams run tile + 17 decimated samples
(two workgroups, the second with one full row tile and one lane of the next) from first_dec_index = 123456789; the FM
banks run fmbank_ref.matrix_shape(tile), two full tiles and a remainder, 4 nct workgroups: with nct = 3 blockIdx.x =
0 .. 11 passes through the kernels' division by nct and meets every (tile, column tile)."""
import numpy as np

import ddc_ref
import ddcfir_ref
import fmbank_ref
import fmfir_ref

MAX_CH = 32
COL_CH = 8                                              # channels of a column tile
FIRST = 123456789
SPECIAL_WORDS = (0, 1, -1, 777, -20001, 32767, -32768)  # those of the four suites together


def _words():
    """32 pairwise different words: seeded random ones, special word i at position 1 + 4 i (two in every column tile
    but the last, which has one)."""
    w, seen = [], set(SPECIAL_WORDS)
    for k in np.random.default_rng(2024).integers(-ddc_ref.P // 2, ddc_ref.P // 2, 4 * MAX_CH):
        if int(k) not in seen and len(w) < MAX_CH:
            seen.add(int(k))
            w.append(int(k))
    for i, s in enumerate(SPECIAL_WORDS):
        w[1 + 4 * i] = s
    return tuple(w)


WORDS = _words()
EVERY_C = tuple(range(1, MAX_CH + 1))
BORDERS = (16, 17, 24, 25)                              # both sides of the borders of the third column tile

# library -> [(path, the C launched there)]; a path is cic_r for the unfiltered banks, (decim, ntaps) for the filtered
RUNS = {
    # the four instantiations Vals<0, 8, 10, 12>; the generic one at one K step (R = 7) and at three (R = 33)
    "ddc": [(8, EVERY_C), (10, EVERY_C), (12, EVERY_C), (7, EVERY_C), (33, EVERY_C)],
    # the three load forms of a window -- aligned (8-byte), both even (4-byte), one odd (2-byte) -- and the extremes of
    # ntaps at the new column-tile counts: ntaps = 256 at C = 17 .. 24 asks for 48 KiB of dynamic LDS, under both
    # instantiations.  One tap at an odd decim: there a channel is its block phasor T[k R g] alone, and at an even R
    # two words with the same k R mod P (0 and -32768 at R = 8) are the same channel
    "ddcfir": [((8, 64), EVERY_C), ((10, 30), EVERY_C), ((7, 17), EVERY_C), ((7, 1), BORDERS), ((8, 256), BORDERS),
               ((10, 256), BORDERS)],
    "fmbank": [(8, EVERY_C), (10, EVERY_C), (12, EVERY_C), (7, EVERY_C)],
    "fmfir": [((8, 40), EVERY_C), ((10, 30), EVERY_C), ((7, 17), EVERY_C)],
}
LIBRARIES = tuple(RUNS)
# the paths of a library that take every C (the ntaps extremes of ddcfir take the borders only)
FULL_PATHS = {lib: [path for path, cs in runs if len(cs) > len(BORDERS)] for lib, runs in RUNS.items()}


def paths(lib):
    return [path for path, _ in RUNS[lib]]


def channels(lib, path):
    return dict(RUNS[lib])[path]


def col_tiles(C):
    """(nct, channels in the last column tile) of a bank of C channels"""
    nct = -(-C // COL_CH)
    return nct, C - COL_CH * (nct - 1)


def path_id(path):
    return "R%d" % path if isinstance(path, int) else "R%d-L%d" % path


def _seed(lib, path):
    return 7000 + 1000 * LIBRARIES.index(lib) + (path if isinstance(path, int) else 10 * path[0] + path[1])


def states():
    """the 32 carried states of the FM banks, f32 [32, 21], pairwise different"""
    return fmbank_ref.states_for(MAX_CH, seed=4242)


def taps_of(path):
    R, L = path
    return fmfir_ref.taps_for(R, L, seed=R + L)


def stream_len(tile):
    return tile + 17


_cache = {}


def stream_inputs(lib, path, tile):
    """The capture of a ddc or ddcfir path (exactly the samples the run needs)."""
    n = stream_len(tile)
    if lib == "ddc":
        return ddc_ref.random_iq(n * path, _seed(lib, path))
    return ddcfir_ref.random_iq(ddcfir_ref.samples_needed(path[0], path[1], n), _seed(lib, path))


def stream_expected(lib, path, tile):
    """int32 [32, tile + 17, 2] of a ddc or ddcfir path on the restatement, computed once, read-only"""
    key = (lib, path, tile)
    if key not in _cache:
        iq = stream_inputs(lib, path, tile)
        if lib == "ddc":
            want = ddc_ref.ddc_ref(iq, path, WORDS, FIRST)
        else:
            want = ddcfir_ref.ddcfir_ref(iq, path[0], taps_of(path), WORDS, 14, FIRST)
        want.setflags(write=False)
        _cache[key] = want
    return _cache[key]


def fm_inputs(lib, path, tile):
    """(capture, block_len, nblocks) of an fmbank or fmfir path"""
    bl, nb = fmbank_ref.matrix_shape(tile)
    if lib == "fmbank":
        return ddc_ref.random_iq(nb * bl * path, _seed(lib, path)), bl, nb
    return ddcfir_ref.random_iq(fmfir_ref.samples_needed(path[0], path[1], bl, nb), _seed(lib, path)), bl, nb


def fm_expected(oracle, lib, path, tile):
    """(audio f32 [32, nblocks * quarter], states f32 [32, 21]) of an fmbank or fmfir path through the oracle's
    per-block chain, computed once, read-only"""
    iq, bl, nb = fm_inputs(lib, path, tile)
    key = ("channels", lib, path, tile)
    if lib == "fmbank":
        return fmbank_ref.expected(oracle, iq, path, WORDS, bl, states(), key=key)
    return fmfir_ref.expected(oracle, iq, path[0], taps_of(path), WORDS, bl, states(), key=key)


# ---- what the suites ran before this list existed: each file's own lists are the source --------------------------

def earlier_channel_counts():
    """library -> the sorted channel counts of its GPU suite's matrices beside this one"""
    import test_ddc_gpu
    import test_ddcfir_gpu
    return {"ddc": sorted({C for _, C in test_ddc_gpu.BANKS}),
            "ddcfir": sorted(set(test_ddcfir_gpu.C_AXIS)),
            "fmbank": sorted({C for _, C in fmbank_ref.BANKS + [fmbank_ref.TILE_BANK] + fmbank_ref.SKIP_BANKS}),
            "fmfir": sorted({b[2] for b in fmfir_ref.BANKS + [fmfir_ref.TILE_BANK] + fmfir_ref.SKIP_BANKS})}


def coverage_text():
    """For the documents: per library the column-tile geometries (nct, channels in the last tile) run before and now."""
    lines = []
    every = {col_tiles(C) for C in EVERY_C}
    for lib, cs in earlier_channel_counts().items():
        before = {col_tiles(C) for C in cs}
        now = {col_tiles(C) for path in FULL_PATHS[lib] for C in channels(lib, path)}
        lines.append("  %-6s before: C = %s: nct in %s, %2d of the %d (nct, last tile); now C = 1 .. 32 at %d paths: %d of %d"
                     % (lib, ", ".join(map(str, cs)), sorted({n for n, _ in before}), len(before), len(every),
                        len(FULL_PATHS[lib]), len(now), len(every)))
    return "\n".join(lines)

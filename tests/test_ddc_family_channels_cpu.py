"""CPU suite of the channel-count matrix of the tuned-channel family (tests/ddc_family_channels.py; DESIGN.md 4.12, 4.12a,
4.13, 4.13c, 10): the lists that the four GPU suites launch hold every C = 1 .. 32 and with them every (number of column
tiles, channels in the last one) of {1 .. 4} x {1 .. 8} at every code path; the 32 words are pairwise different and hold
the suites' special ones; on the restatements the 32 expected rows of every case are pairwise different (audio and
states for the FM banks), so a channel stored in another one's row, or a row stored twice, cannot pass; deleting any one
C from any path breaks a condition; the grids and the dynamic LDS that the GPU tests assert are what the libraries
report.  No GPU is used.

The channel counts that the suites ran before (each file's own BANKS, C_AXIS, TILE_BANK and SKIP_BANKS), and now:
%s
Before, no launch of any of the four kernels had three column tiles, none had a second column tile holding more than
one channel, and no test looked at an output row behind the last channel's."""
import copy

import numpy as np
import pytest

import ddc_family_channels as ch

__doc__ %= ch.coverage_text()

EVERY_GEOMETRY = {(nct, last) for nct in range(1, 5) for last in range(1, 9)}


def conditions(runs):
    """What the lists have to meet, on their own (no restatement): raises AssertionError."""
    assert set(runs) == {"ddc", "ddcfir", "fmbank", "fmfir"}
    want_paths = {"ddc": {8, 10, 12, 7, 33}, "fmbank": {8, 10, 12, 7},
                  "ddcfir": {(8, 64), (10, 30), (7, 17)}, "fmfir": {(8, 40), (10, 30), (7, 17)}}
    for lib, paths in want_paths.items():
        full = {path: cs for path, cs in runs[lib] if path in paths}
        assert set(full) == paths, lib
        for path, cs in full.items():
            assert sorted(cs) == list(range(1, 33)) and len(set(cs)) == len(cs), (lib, path)
            assert {ch.col_tiles(C) for C in cs} == EVERY_GEOMETRY, (lib, path)
    # the three load forms of a window, by their conditions
    for lib in ("ddcfir", "fmfir"):
        forms = {(R % 4 == 0 and L % 4 == 0, (R | L) % 2 == 0) for R, L in want_paths[lib]}
        assert forms == {(True, True), (False, True), (False, False)}, lib
    # the extremes of ntaps at the borders of the third column tile, both instantiations at the largest LDS
    extremes = {path: cs for path, cs in runs["ddcfir"] if path not in want_paths["ddcfir"]}
    assert {L for _, L in extremes} == {1, 256}
    assert {(R % 4 == 0) for R, L in extremes if L == 256} == {True, False}
    for path, cs in extremes.items():
        assert tuple(cs) == (16, 17, 24, 25), path
    assert sum(len(p) for p in want_paths.values()) + len(extremes) == sum(len(r) for r in runs.values())


def test_the_lists_meet_their_conditions():
    conditions(ch.RUNS)
    assert ch.FULL_PATHS == {"ddc": [8, 10, 12, 7, 33], "ddcfir": [(8, 64), (10, 30), (7, 17)], "fmbank": [8, 10, 12, 7],
                             "fmfir": [(8, 40), (10, 30), (7, 17)]}
    launches = sum(len(cs) for runs in ch.RUNS.values() for _, cs in runs)
    assert launches == 15 * 32 + 3 * 4
    assert [ch.col_tiles(C) for C in (1, 8, 9, 16, 17, 24, 25, 32)] == [(1, 1), (1, 8), (2, 1), (2, 8), (3, 1), (3, 8), (4, 1), (4, 8)]


def test_deleting_any_one_channel_count_fails():
    n = 0
    for lib, runs in ch.RUNS.items():
        for i, (path, cs) in enumerate(runs):
            for C in cs:
                cut = copy.deepcopy({k: list(v) for k, v in ch.RUNS.items()})
                cut[lib][i] = (path, tuple(c for c in cs if c != C))
                with pytest.raises(AssertionError):
                    conditions(cut)
                n += 1
    assert n == 15 * 32 + 3 * 4
    for lib in ch.RUNS:                                   # and so does a path that is missing altogether
        cut = {k: list(v) for k, v in ch.RUNS.items()}
        cut[lib] = cut[lib][1:]
        with pytest.raises(AssertionError):
            conditions(cut)


def test_the_words_are_pairwise_different_and_hold_the_special_ones():
    import test_ddc_gpu
    import test_ddcfir_gpu
    import fmbank_ref
    assert len(ch.WORDS) == 32 == len(set(ch.WORDS))
    assert all(-32768 <= k <= 32767 for k in ch.WORDS)
    assert {0, 1, -1, 777, -20001, 32767, -32768} == set(ch.SPECIAL_WORDS) <= set(ch.WORDS)
    assert set(test_ddc_gpu.SPECIAL_WORDS) | set(test_ddcfir_gpu.SPECIAL_WORDS) | set(fmbank_ref.SPECIAL_WORDS) == set(ch.SPECIAL_WORDS)
    for ct in range(4):                                   # special and random words in every column tile
        tile_words = set(ch.WORDS[8 * ct:8 * ct + 8])
        assert tile_words & set(ch.SPECIAL_WORDS) and tile_words - set(ch.SPECIAL_WORDS), ct
    st = ch.states()
    assert st.shape == (32, 21) and len({s.tobytes() for s in st}) == 32


def test_what_the_suites_ran_before():
    """The docstring's figures as assertions: nct was 1, 2 or 4 everywhere, a second column tile held one channel or
    eight (as the second of four), and of the 32 (nct, last tile) geometries the suites reached 5 or 6."""
    before = ch.earlier_channel_counts()
    assert before == {"ddc": [1, 2, 8, 9, 32], "ddcfir": [1, 2, 7, 8, 9, 32], "fmbank": [1, 2, 8, 9, 32],
                      "fmfir": [1, 2, 3, 8, 9, 32]}
    for lib, cs in before.items():
        geo = {ch.col_tiles(C) for C in cs}
        assert {n for n, _ in geo} == {1, 2, 4}, lib
        assert {last for n, last in geo if n == 2} == {1}, lib
        assert not any(10 <= C <= 31 for C in cs), lib
        assert len(geo) == len(cs)
    print(ch.coverage_text())


def _distinct(rows):
    return len({np.ascontiguousarray(r).tobytes() for r in rows}) == len(rows)


def _tiles(built):
    return {"ddc": built.ddc_grid(8, 1, 1)[4], "ddcfir": built.ddcfir_grid(8, 8, 1, 1)[4],
            "fmbank": built.fmbank_grid(8, 1, 20, 1)[4], "fmfir": built.fmfir_grid(8, 8, 1, 20, 1)[4]}


@pytest.mark.parametrize("lib", ["ddc", "ddcfir"])
def test_the_expected_streams_are_pairwise_different(built, lib):
    tile = _tiles(built)[lib]
    n = ch.stream_len(tile)
    assert n == tile + 17 and tile % 16 == 0               # one full row tile and one lane of the next
    for path in ch.paths(lib):
        want = ch.stream_expected(lib, path, tile)
        assert want.shape == (32, n, 2) and want.dtype == np.int32 and not want.flags.writeable
        assert _distinct(want), (lib, path)
        assert ch.stream_expected(lib, path, tile) is want                       # computed once
        if lib == "ddcfir":
            assert ch.stream_inputs(lib, path, tile).shape[0] == built.ddcfir_samples_needed(path[0], path[1], n)


@pytest.mark.parametrize("lib", ["fmbank", "fmfir"])
def test_the_expected_audio_and_states_are_pairwise_different(built, oracle, lib):
    tile = _tiles(built)[lib]
    for path in ch.paths(lib):
        iq, bl, nb = ch.fm_inputs(lib, path, tile)
        audio, st = ch.fm_expected(oracle, lib, path, tile)
        assert audio.shape == (32, nb * (bl // 4)) and st.shape == (32, 21)
        assert _distinct(audio) and _distinct(st), (lib, path)
        assert not audio.flags.writeable and ch.fm_expected(oracle, lib, path, tile)[0] is audio
        assert 2 * tile < nb * (bl // 4) < 3 * tile                              # two full tiles and a remainder
        if lib == "fmfir":
            assert iq.shape[0] == built.fmfir_samples_needed(path[0], path[1], bl, nb)


def test_the_grids_the_gpu_tests_assert(built):
    """ceil(dec_len / tile) workgroups for the banks that store streams, (ntiles + 1) ceil(C / 8) for the FM banks,
    ceil(C / 8) ceil(L / 16) KiB of dynamic LDS for the filtered bank: 48 KiB at ntaps = 256 and three column tiles."""
    tiles = _tiles(built)
    for lib, runs in ch.RUNS.items():
        tile = tiles[lib]
        for path, cs in runs:
            for C in cs:
                nct = ch.col_tiles(C)[0]
                if lib == "ddc":
                    assert built.ddc_grid(path, C, ch.stream_len(tile))[:2] == (0, 2)
                elif lib == "ddcfir":
                    rc, blocks, _, lds, _ = built.ddcfir_grid(path[0], path[1], C, ch.stream_len(tile))
                    assert (rc, blocks, lds) == (0, 2, nct * -(-path[1] // 16) * 1024), (path, C)
                else:
                    bl, nb = ch.fm_inputs(lib, path, tile)[1:]
                    grid = built.fmbank_grid(path, C, bl, nb) if lib == "fmbank" else built.fmfir_grid(path[0], path[1], C, bl, nb)
                    assert grid[:2] == (0, 4 * nct), (lib, path, C)
    assert [built.ddcfir_grid(8, 256, C, 1)[3] for C in ch.BORDERS] == [32768, 49152, 49152, 65536]

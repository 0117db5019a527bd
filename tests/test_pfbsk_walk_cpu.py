"""CPU suite of the walk matrix of the spectrometer with excision (tests/pfbsk_walk_cases.py, csrc/pfbsk.hip, DESIGN.md
4.18): the L that tests/test_pfbsk_gpu.py::test_every_walk_geometry_to_the_bit launches reach, with the L = 3 of the
matrix before it, every class of walk that any L = 1 .. 65535 reaches at every K < F of tests/pfb_ksum_cases.py; the
largest sub-integration of a tile, two full steps in a row and a last step one sub-integration short of a tile are
launched wherever they exist; the item split of pfbsk.hip restated and checked exhaustively; the size of the matrix
under a bound; and the f64 definition alone, on the captures and taps of the GPU test, flags some and keeps some
sub-integrations at every (log2 M, hop).  No GPU is used.

The classes, the number of (log2 M, K < F) of the matrix where each occurs, and at how many of them the suite held it
to the bit before (L = 3 and pfbsk_walk_cases.OLD_OUTSIDE) and holds it now:
%s"""
import numpy as np
import pytest

import pfb_ksum_cases as ksum
import pfbsk_ref
import pfbsk_walk_cases as walks
from test_pfb_ksum_gpu import T, capture, frames64, the_taps

__doc__ %= walks.coverage_text()


def below_a_tile(k):
    return [K for K in ksum.cases(k) if K < ksum.tile_frames(k)]


def launched(k, K):
    """The L of the walk matrix and the one of the matrix before it."""
    return sorted(set(walks.ls(k, K)) | {walks.OLD_NSUB})


def test_the_cases_reach_every_class():
    """At every (log2 M, K < F) of the matrix the launched L hold every class that L = 1 .. 65535 reach.  L is
    enumerated to 3 G + 2 only: the class of L is a function of min(steps, 3) and of whether last = G.  For L > 3 G,
    L - G has one step less, still >= 3, and the same last step, hence the same class, so every L > 3 G has the class
    of one L in 2 G + 1 .. 3 G.  The identity is checked where the enumeration ends and at the largest L."""
    for k in ksum.LOG2_MS:
        assert [K for K in walks.ks(k) if K < ksum.tile_frames(k)] == below_a_tile(k)
        for K in below_a_tile(k):
            G = ksum.geometry(k, K)[1]
            every = {walks.classify(k, K, L) for L in walks.enumerated(k, K)}
            assert len(every) == (6 if G > 1 else 3), (k, K)
            for L in list(range(3 * G + 1, 5 * G + 3)) + [walks.MAX_NSUB - i for i in range(min(G, 300))]:
                assert walks.classify(k, K, L) == walks.classify(k, K, L - G) and walks.walk(k, K, L - G)[2] >= 3, (k, K, L)
            got = {walks.classify(k, K, L) for L in launched(k, K)}
            assert got == every, (k, K, every - got)
            assert walks.ls(k, K) == ([G - 1, G, G + 1, 2 * G, 2 * G + 1, 3 * G] if G > 1 else [1, 2]), (k, K)
            assert all(1 <= L <= walks.MAX_NSUB for L in walks.ls(k, K))
    assert walks.classify(4, 16, 16) == ("1 step", "last step full", "G > 1")
    assert walks.classify(4, 16, 33) == (">= 3 steps", "last step ragged", "G > 1")
    assert walks.classify(4, 144, 2) == walks.classify(4, 515, 2) == ("2 steps", "G = 1")


def test_the_suite_before_did_not():
    """What the docstring above says, as assertions: before, one partial step was the only walk at every G > 3 but
    two, no (log2 M, K) but (4, 16) and (10, 2) had two full steps one after the other, no item g >= 3 was live beside
    other slices, and L = 1, 2 ran nowhere in the matrix."""
    cover = walks.coverage()
    assert all(now == occurs for occurs, _, now in cover.values())
    assert any(before < occurs for occurs, before, _ in cover.values())
    for k in ksum.LOG2_MS:
        for K in below_a_tile(k):
            G = ksum.geometry(k, K)[1]
            old = walks.old_ls(k, K)
            if G > 3 and (k, K) not in [(kk, KK) for kk, KK, _ in walks.OLD_OUTSIDE]:
                assert {walks.classify(k, K, L) for L in old} == {walks.ONE_PARTIAL_STEP}, (k, K)
            if G > 1:
                assert (max(old) > 2 * G) == ((k, K) in ((4, 16), (10, 2))), (k, K)
    # the one (log2 M, K) before with an item g >= 3 live has a single slice
    assert [ksum.geometry(k, K)[3] for k, K, L in walks.OLD_OUTSIDE if min(L, ksum.geometry(k, K)[1]) > 3] == [1, 1]
    assert not any(L in (1, 2) for k in ksum.LOG2_MS for K in ksum.cases(k) for L in walks.old_ls(k, K))


def test_the_last_sub_integration_of_a_tile_and_two_full_steps():
    """Wherever a tile holds four sub-integrations or more, some launched L makes its last one (g = G - 1) live and
    some L takes two full steps one after the other: part1 / part2 written over a tile that a further pass reuses,
    clean[] and kept[] carried across.  And the "+0 behind the step's last sub-integration" rule is launched at both
    of its borders: a last step of G - 1 sub-integrations, and one of a single one behind a full step."""
    many = 0
    for k in ksum.LOG2_MS:
        for K in below_a_tile(k):
            G = ksum.geometry(k, K)[1]
            if G == 1:
                continue
            shapes = [walks.walk(k, K, L)[2:] for L in launched(k, K)]
            assert any(L >= G for L in launched(k, K)), (k, K)                              # g = G - 1 live
            assert any(L >= 2 * G for L in launched(k, K)), (k, K)                          # two full steps
            assert (1, G - 1) in shapes and (2, 1) in shapes and (3, 1) in shapes, (k, K)
            many += G >= 4
    assert many == 31                                                      # of the 42 (log2 M, K) with G > 1


def test_every_slice_count_meets_every_sub_integration_of_its_tile():
    """M = 16: every nsl = 1 .. 8 with G > 1 is launched with every g < G live (the split (g, s) of an item by the
    reciprocal of nsl, at every g that the tile holds), in a first step and in a later one."""
    seen = {}
    for K in below_a_tile(4):
        _, G, _, nsl, _ = ksum.geometry(4, K)
        if G > 1:
            seen.setdefault(nsl, []).append((G, [L for L in walks.ls(4, K) if L >= G], [L for L in walks.ls(4, K) if L >= 2 * G]))
    assert sorted(seen) == list(range(1, 9))
    assert all(first and later for runs in seen.values() for _, first, later in runs)
    assert max(G for G, _, _ in seen[1]) == 256 and {G for n in range(4, 9) for G, _, _ in seen[n]} == {2, 3, 4}


def test_the_item_split_is_exact():
    """pfbsk.hip's item w = (g nsl + s) M + c: gs = w / M is split by g = (gs * inv) >> 16 with inv = 65536 / nsl + 1.
    Equal to gs // nsl for every (log2 M, K < F, gs < G nsl), the items fit the tile (items = gn nsl M <= 4096: a thread
    has at most 16), the source rows g K + s SLICE .. of a live item lie inside the tile, and the fold's
    w = g nsl M + c with its slices w + s M is the same numbering."""
    for k in ksum.LOG2_MS:
        M, F, SLICE = 1 << k, ksum.tile_frames(k), ksum.slice_frames(k)
        assert F * M == ksum.TILE_POINTS == 4096 and SLICE == min(16, F)
        for K in range(1, F):
            G, nsl = F // K, -(-K // SLICE)
            assert (False, G, 1, nsl, K) == ksum.geometry(k, K)
            assert G * nsl * M <= ksum.TILE_POINTS, (k, K)
            inv = 65536 // nsl + 1
            gs = np.arange(G * nsl, dtype=np.int64)
            g = (gs * inv) >> 16
            assert np.array_equal(g, gs // nsl) and int(gs[-1]) * inv < 2 ** 31, (k, K)
            s = gs - g * nsl
            first = g * K + s * SLICE
            assert np.all(first + np.minimum(SLICE, K - s * SLICE) <= G * K) and G * K <= F, (k, K)
            assert np.array_equal(g * nsl * M + s * M, gs * M)
            # a dead item (w >= items) reads nothing, and its source row is still a row of the tile or the one behind it
            every = np.arange(ksum.TILE_POINTS // M, dtype=np.int64)
            ge = (every * inv) >> 16
            assert int((ge * K + (every - ge * nsl) * SLICE).min()) >= 0


def test_the_matrix_stays_small():
    """The runs are three rows of L K frames: 9 F frames at most where K < F (L <= 3 G, G K <= F), 6 (2 F + 3) where
    K >= F.  In points, rows L K M <= 12 * 4096 + 18 M: under 68 000 complex samples in the longest run of all."""
    counts = {}
    for k in ksum.LOG2_MS:
        M, F = 1 << k, ksum.tile_frames(k)
        cases = walks.walk_cases(k)
        counts[k] = len(cases)
        assert len(set(cases)) == len(cases) and not any(L == walks.OLD_NSUB for _, L in cases)
        assert {K for K, _ in cases} == set(walks.ks(k)) and set(walks.ks(k)) - set(below_a_tile(k)) == {F, 2 * F + 3}
        for K, L in cases:
            assert walks.frames(K, L) * M <= (9 * ksum.TILE_POINTS if K < F else 12 * ksum.TILE_POINTS + 18 * M), (k, K, L)
        assert max(walks.frames(K, L) for K, L in cases) == walks.frames(2 * F + 3, 2) == 6 * (2 * F + 3)
        assert max(walks.frames(K, L) for K, L in cases if K < F) == walks.frames(1, 3 * F) == 9 * F
    assert max(walks.frames(K, L) << k for k in ksum.LOG2_MS for K, L in walks.walk_cases(k)) == 67584
    assert counts == {4: 81, 5: 54, 6: 47, 7: 35, 8: 29, 9: 24, 10: 16}, counts
    assert sum(counts.values()) == 286


@pytest.mark.parametrize("k", ksum.LOG2_MS)
def test_the_definition_alone_flags_some_and_keeps_some(k):
    """tests/test_pfbsk_gpu.py::test_every_walk_geometry_to_the_bit asks at every (log2 M, hop) that, over its cases,
    the device flags a sub-integration and keeps one under the bounds of thresholds 0.5 and 1.6.  The f64 definition
    (pfbsk_ref) on the same capture and taps does both, so the condition is the input's and not the kernel's."""
    M = 1 << k
    cases = walks.walk_cases(k)
    longest = max(walks.frames(K, L) for K, L in cases)
    iq, taps = capture(k, 0, longest), the_taps(k)
    scale = pfbsk_ref.power_scale(taps)
    for D in (M, M // 2):
        y = frames64(k, D, 0, longest)
        flagged = kept = 0
        for K, L in cases:
            s1, s2 = pfbsk_ref.sub_sums(y[:walks.frames(K, L)], K, scale)
            flags = pfbsk_ref.flagged(s1, s2, K, scale, *pfbsk_ref.bounds(K, pfbsk_ref.SK_LO, pfbsk_ref.SK_HI))
            assert flags.shape == (walks.ROWS * L, M)
            flagged, kept = flagged + int(flags.sum()), kept + int((~flags).sum())
        assert flagged > 0 and kept > 0, (k, D, flagged, kept)
    # the same through the definition's own entry point, once: the longest case, hop M, against the end of the capture
    K, L = max(cases, key=lambda c: walks.frames(*c))
    assert len(iq) == pfbsk_ref.samples_needed(M, T, M, K, L, walks.ROWS)
    lo, hi = pfbsk_ref.bounds(K, pfbsk_ref.SK_LO, pfbsk_ref.SK_HI)
    _, n, s1, s2 = pfbsk_ref.pfbsk_ref(iq, k, taps, K, L, lo, hi, scale, M, nspectra=walks.ROWS)
    want1, want2 = pfbsk_ref.sub_sums(frames64(k, M, 0, longest), K, scale)
    assert s1.shape == (walks.ROWS * L, M) and np.array_equal(s1, want1) and np.array_equal(s2, want2)
    assert np.array_equal(n, pfbsk_ref.clean_rows(want1, pfbsk_ref.flagged(want1, want2, K, scale, lo, hi), L)[1])

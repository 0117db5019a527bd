"""The polyphase family's launch-table model (tests/pfb_family_matrix.py) against the five libraries' gfx950 code
objects, both ways: every instantiation a library holds is named by a case of the model, and every case names an
instantiation a library holds.  So a table entry cannot land without a case that tests/test_pfb_family_matrix_gpu.py
launches, and a model that drifts from the tables fails here, without a GPU.  Kernel names only are read."""
import re

import pfb_family_matrix as fm
import pfb_ksum_cases as ksum
import pfb_ref


def _arg(s):
    s = s.strip()
    return s == "true" if s in ("true", "false") else int(s)


def _library_kernels(built, lib):
    """The instantiations of librtlws_<lib>.so as (name, args)."""
    from rtlws import codeobj
    getattr(built, lib + "_lib")()
    found = set()
    for k in codeobj.kernels(getattr(built, lib.upper() + "_LIB")):
        d = k.get("demangled", k["name"])
        m = re.match(r"^(?:void )?rtlws::%s::(\w+)<([^>]*)>\(" % lib, d)
        assert m, d
        assert m.group(1) in fm.KERNELS[lib], d
        t = (m.group(1), tuple(_arg(a) for a in m.group(2).split(",")))
        assert t not in found, d
        found.add(t)
    return found


def test_every_instantiation_has_a_case_and_every_case_an_instantiation(built):
    held = {lib: _library_kernels(built, lib) for lib in fm.LIBRARIES}
    modelled = {}
    for c in fm.CASES:
        modelled.setdefault((c.lib, fm.instantiation(c)), []).append(c)
    everything = {(lib, t) for lib in fm.LIBRARIES for t in held[lib]}
    untested = sorted(everything - set(modelled))
    phantom = sorted((t, [c.label() for c in modelled[t]]) for t in set(modelled) - everything)
    assert not untested, "instantiations no case reaches: %s" % untested
    assert not phantom, "cases that name no instantiation: %s" % phantom
    counts = {lib: len(held[lib]) for lib in fm.LIBRARIES}
    print("%d polyphase instantiations, matched by %d cases: %s" % (len(everything), len(fm.CASES), counts))
    assert counts == fm.COUNTS == {"pfb": 7, "pfbspec": 7, "pfbxc": 21, "pfbbf": 84, "pfbsk": 14}
    assert len(everything) == 133
    # one case per instantiation
    assert len(fm.CASES) == 133 and all(len(cs) == 1 for cs in modelled.values())
    assert len({c.label() for c in fm.CASES}) == 133


def test_model_restates_the_rules():
    """Spot checks of the rules the model restates (pfb_bank.h, the launch functions), so that a slip in the model
    shows as such and not as a library mismatch."""
    assert fm.LOG2_MS == ksum.LOG2_MS and [fm.tile_frames(k) for k in fm.LOG2_MS] == [256, 128, 64, 32, 16, 8, 4]
    assert all(fm.tile_frames(k) == ksum.tile_frames(k) for k in fm.LOG2_MS)
    # WHOLE = k_avg >= tile_frames(k), at the boundary
    for k, F in ((4, 256), (10, 4)):
        assert [fm.whole(k, K) for K in (F - 1, F, F + 1)] == [False, True, True]
        assert all(fm.whole(k, K) == ksum.geometry(k, K)[0] for K in (1, F - 1, F, F + 1, ksum.MAX_K_AVG))
        for lib, name, lead in (("pfbbf", "pfbbf_power_kernel", (k, 3)), ("pfbsk", "pfbsk_kernel", (k,))):
            B = 3 if lib == "pfbbf" else 0
            got = [fm.instantiation(fm.Case(lib, k, 1, 1, B, K)) for K in (F - 1, F, F + 1)]
            assert got == [(name, lead + (False,)), (name, lead + (True,)), (name, lead + (True,))]
    assert fm.instantiation(fm.Case("pfbbf", 7, 3, 5, 3, 49)) == ("pfbbf_power_kernel", (7, 3, True))
    assert fm.instantiation(fm.Case("pfbbf", 7, 3, 5, 3, 0)) == ("pfbbf_kernel", (7, 3))
    assert fm.instantiation(fm.Case("pfbxc", 9, 1, 4, 0, 0)) == ("pfbxc_kernel", (9, 4))
    assert fm.spell(("pfbbf_power_kernel", (7, 3, True))) == "pfbbf_power_kernel<7, 3, true>"
    # T: the first that pfb_ref.SHAPES lists for the log2 M
    assert fm.TAPS_PER_BRANCH == {4: 1, 5: 2, 6: 8, 7: 3, 8: 8, 9: 1, 10: 4}
    assert all((c.k, c.T) in pfb_ref.SHAPES for c in fm.CASES)


def test_the_k_of_the_sum_kernels_lands_in_its_class():
    """WHOLE: K = F + 17, two or more tile iterations with the last one ending inside a slice; else K = 17 where
    F > 34 (several slices, the last one ragged, several spectra in the tile) and K = 3 below (one ragged slice)."""
    for k in fm.LOG2_MS:
        F = ksum.tile_frames(k)
        K = fm.sum_k(k, True)                                            # it asserts its class itself
        whole, G, nit, nsl, last = ksum.geometry(k, K)
        assert K == F + 17 and whole and nit >= 2 and last % ksum.slice_frames(k) != 0 and last < F, (k, K)
        K = fm.sum_k(k, False)
        whole, G, nit, nsl, last = ksum.geometry(k, K)
        assert K == (17 if k <= 6 else 3) and not whole and K % ksum.slice_frames(k) != 0, (k, K)
        assert (nsl, G > 1) == ((2, True) if K == 17 else (1, F // 3 > 1)), (k, K)
    for c in fm.CASES:
        ks = fm.run_ks(c)
        if c.lib in ("pfbspec", "pfbxc"):
            assert c.K == 0 and [fm.whole(c.k, K) for K in ks] == [False, True], c.label()
        elif c.lib == "pfb" or (c.lib == "pfbbf" and c.K == 0):
            assert ks == ()
        else:
            assert ks == (c.K,) and c.K in (fm.sum_k(c.k, False), fm.sum_k(c.k, True)), c.label()


def test_every_capture_count_meets_every_beam_count():
    """The beamformer's A is a run-time loop over BfParams::src[8]: every A = 1 .. 8 occurs with every B, and A = 5,
    6 and 7 occur with every B at log2 M <= 8 (one channel to a thread) and at log2 M >= 9 (M / 256 channels)."""
    bf = fm.by_library("pfbbf")
    assert len(bf) == 84
    for B in fm.BEAMS:
        mine = [c for c in bf if c.B == B]
        assert len(mine) == 21
        assert {c.A for c in mine} == set(range(1, fm.MAX_BF_INPUTS + 1)), B
        for A in (5, 6, 7):
            assert any(c.A == A and c.k <= 8 for c in mine) and any(c.A == A and c.k >= 9 for c in mine), (B, A)
    assert all(c.A == 1 and c.B == 0 for c in fm.CASES if c.lib in ("pfb", "pfbspec", "pfbsk"))
    assert sorted((c.k, c.A) for c in fm.by_library("pfbxc")) == [(k, A) for k in fm.LOG2_MS for A in fm.XC_INPUTS]


def _launched_before():
    """The beamformer's and the correlator's instantiations that the earlier suites and smoke() launch, from their own
    parametrisations (imported where they are data, restated where a test fixes its shape in its body)."""
    import test_pfb_family_digest_gpu as digest
    import test_pfb_ksum_gpu as sums
    import test_pfbbf_gpu as bf
    import test_pfbxc_gpu as xc

    def k_list(F):
        assert bf.k_list(F) == xc.k_list(F)
        return bf.k_list(F)

    seen = set()

    def beam(k, B, ks, voltage=True):
        if voltage:
            seen.add(("pfbbf_kernel", (k, B)))
        seen.update(("pfbbf_power_kernel", (k, B, fm.whole(k, K))) for K in ks)

    for k, T, A, B in bf.CASES:                                          # the four parametrised bit and f64 tests
        beam(k, B, k_list(4096 >> k))
    for k, T, A, B in bf.MULTI_CASES:                                    # reproducible, and beam b alone: B and 1
        for nb in (B, 1):
            beam(k, nb, (3, (4096 >> k) + 1))
    for k, T in bf.MULTI_SHAPES:                                         # test_degenerate_inputs: two beams
        beam(k, 2, (1, 3, (4096 >> k) + 1))
    beam(5, 2, (3,))                                                     # test_strides_and_nothing_outside, and smoke()
    beam(6, 2, (5,))                                                     # test_capture_and_replay
    beam(6, 2, (65,))                                                    # test_the_delay_case_on_the_device
    for k in sums.ksum.LOG2_MS:                                          # the K-sum suite: its reference is a voltage run
        for A, B in sums.BEAMS:
            beam(k, B, ksum.cases(k))
    beam(sums.BIG[0], sums.BEAMS[0][1], (sums.BIG[1],))
    for k in digest.LOG2_MS:                                             # the digests: weights_of() holds two beams
        assert digest.weights_of(k).shape[0] == 2
        beam(k, 2, [digest.k_and_spectra(k, kind)[0] for kind in digest.K_KINDS])

    seen.update(("pfbxc_kernel", (k, A)) for k, T, A in xc.CASES)
    seen.update(("pfbxc_kernel", (k, A)) for k, T in xc.ORDER_SHAPES for A in (2, 3))
    seen.update(("pfbxc_kernel", (k, 3)) for k, T in xc.MULTI_SHAPES)                      # test_degenerate_inputs
    seen.update({("pfbxc_kernel", (5, 3)), ("pfbxc_kernel", (6, 2))})                      # strides and smoke(); graph, delay
    seen.update(("pfbxc_kernel", (k, A)) for k in sums.ksum.LOG2_MS for A in ((2, 3, 4) if k in sums.MULTI else (3,)))
    seen.update(("pfbxc_kernel", (k, 3)) for k in digest.LOG2_MS)
    return seen


def test_first_launched_here_is_what_no_earlier_suite_reached():
    """The pinned list is a part of the matrix, holds every B = 3 kernel, and is exactly what is left of the
    beamformer's and the correlator's 105 instantiations when those that the earlier suites' parametrisations reach are
    taken away.  (The channelizer's, the spectrometer's and the kurtosis spectrometer's kernels all ran at every log2 M
    and, the last, at a K of each side: tests/test_pfb_gpu.py, test_pfbspec_gpu.py, test_pfbsk_gpu.py.)"""
    matrix = {fm.instantiation(c) for c in fm.CASES}
    first = set(fm.FIRST_LAUNCHED_HERE)
    assert len(first) == len(fm.FIRST_LAUNCHED_HERE) == 32
    assert first <= matrix
    three = {t for t in matrix if t[0] in ("pfbbf_kernel", "pfbbf_power_kernel") and t[1][1] == 3}
    assert len(three) == 21 and three <= first
    both = {t for t in matrix if t[0] in ("pfbbf_kernel", "pfbbf_power_kernel", "pfbxc_kernel")}
    before = _launched_before()
    assert before <= both and len(both) == 105
    assert both - before == first, (sorted(both - before - first), sorted(first - (both - before)))
    print("first launched by the matrix: %d instantiations (%d of the beamformer, %d of the correlator): %s"
          % (len(first), sum(t[0] != "pfbxc_kernel" for t in first), sum(t[0] == "pfbxc_kernel" for t in first),
             ", ".join(fm.spell(t) for t in fm.FIRST_LAUNCHED_HERE)))

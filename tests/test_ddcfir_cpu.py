"""CPU suite of include/rtlws_ddcfir.h (librtlws_ddcfir.so): the ABI, the kernels' resources from the code-object
metadata, the filter design, the sizes, the refusals -- and the numpy restatement's own properties
(tests/ddcfir_ref.py), which hold the yardstick rather than the code under test.  No GPU is used."""
import ctypes
import re
import subprocess

import numpy as np
import pytest

import ddc_ref
import ddcfir_ref as ref
from test_abi_cpu import _declared_functions, _exported

P = ref.P
FIRST = 123456789


def test_ddcfir_library_exports_its_header_and_nothing_else(built):
    built.ddcfir_lib()
    declared = _declared_functions("rtlws_ddcfir.h")
    assert len(declared) == 9
    assert _exported(built.DDCFIR_LIB) == set(declared)
    assert set(built.DDCFIR_SYMBOLS) == set(declared)
    dyn = subprocess.run(["readelf", "-d", built.DDCFIR_LIB], capture_output=True, text=True, check=True).stdout
    assert "librtlws_hip.so" in dyn and "$ORIGIN" in dyn
    assert (built.DDCFIR_MAX_TAPS, built.DDCFIR_MAX_TAP) == (ref.MAX_TAPS, ref.MAX_TAP)
    # the tuning word is rtlws_ddc.h's: this library has none of its own
    assert not any("tuning_word" in name for name in declared)


def test_ddcfir_kernels_do_not_spill(built):
    """Every kernel of the library: no scratch, no spilled register; the kernel names are exactly the two
    instantiations the launch table reaches; the operands live in dynamic LDS, so the code object fixes none."""
    from rtlws import codeobj
    built.ddcfir_lib()
    ks = codeobj.kernels(built.DDCFIR_LIB)
    names = set()
    for k in ks:
        d = k.get("demangled", k["name"])
        m = re.search(r"rtlws::ddcfir::(ddcfir_bank_kernel<\w+>)", d)
        assert m, d
        names.add(m.group(1))
        assert k["vgpr_spill_count"] == 0 and k["private_segment_fixed_size"] == 0, d
        assert not k.get("sgpr_spill_count", 0), d
        assert k["max_flat_workgroup_size"] == 256 and k["group_segment_fixed_size"] == 0, d
    assert names == {"ddcfir_bank_kernel<true>", "ddcfir_bank_kernel<false>"} and len(ks) == 2


def test_design_equals_the_documented_formula(built):
    for R, L in ((12, 96), (12, 12), (8, 64), (10, 80), (1, 1), (5, 1), (128, 256), (3, 255), (12, 13), (16, 17), (7, 2)):
        got = built.ddcfir_design(R, L)
        assert got.dtype == np.int16 and got.shape == (L,)
        assert np.array_equal(got, ref.design(R, L)), (R, L)
        assert np.array_equal(got, got[::-1]), (R, L)                        # linear phase
        assert np.abs(got.astype(np.int64)).max() <= ref.MAX_TAP, (R, L)
        assert got.astype(np.int64).sum() <= 16384 * R + L // 2, (R, L)
    # long enough filters reach the CIC's gain but for the taps' rounding; the shortest are held by the tap limit
    for R, L in ((12, 96), (8, 64), (10, 80), (128, 256)):
        assert abs(int(built.ddcfir_design(R, L).astype(np.int64).sum()) - 16384 * R) <= L // 2, (R, L)
    assert list(built.ddcfir_design(1, 1)) == [16384] and list(built.ddcfir_design(5, 1)) == [ref.MAX_TAP]
    assert built.ddcfir_design(12, 12).max() == ref.MAX_TAP
    L = built.ddcfir_lib()
    taps = np.zeros(256, np.int16)
    for R, n, word in ((0, 8, "decim"), (129, 8, "decim"), (8, 0, "ntaps"), (8, 257, "ntaps")):
        assert L.rtlws_ddcfir_design(R, n, taps.ctypes.data) == -1 and word in built.ddcfir_last_error(), (R, n)
    assert L.rtlws_ddcfir_design(8, 8, None) == -1 and "null" in built.ddcfir_last_error()


def test_bound_equals_the_documented_formula(built):
    for taps, s in ((ref.design(12, 96), 14), (np.full(256, ref.MAX_TAP), 0), (ref.random_taps(255, 1), 30), ([-5], 3)):
        assert built.ddcfir_bound(taps, s) == pytest.approx(ref.bound(taps, s), rel=1e-14)
    L = built.ddcfir_lib()
    t, b = np.ones(4, np.int16), ctypes.c_double(0.0)
    for n, tp, s, bp, word in ((0, t.ctypes.data, 0, ctypes.byref(b), "ntaps"), (257, t.ctypes.data, 0, ctypes.byref(b), "ntaps"),
                               (4, t.ctypes.data, -1, ctypes.byref(b), "out_shift"), (4, t.ctypes.data, 31, ctypes.byref(b), "out_shift"),
                               (4, None, 0, ctypes.byref(b), "null"), (4, t.ctypes.data, 0, None, "null")):
        assert L.rtlws_ddcfir_bound(n, tp, s, bp) == -1 and word in built.ddcfir_last_error(), (n, s)


def test_sizes_need_no_gpu(built):
    need, grid = built.ddcfir_samples_needed, built.ddcfir_grid
    for R, L, n in ((12, 96, 1000), (1, 1, 1), (128, 256, 5), (16, 7, 3), (3, 255, 1 << 40)):
        assert need(R, L, n) == (n - 1) * R + L == ref.samples_needed(R, L, n) and built.ddcfir_last_error() == ""
    assert need(12, 96, 0) == 0
    for args, word in (((0, 8, 1), "decim"), ((129, 8, 1), "decim"), ((8, 0, 1), "ntaps"), ((8, 257, 1), "ntaps"),
                       ((8, 8, -1), "dec_len"), ((8, 8, 1 << 62), "grid")):
        assert need(*args) == -1 and word in built.ddcfir_last_error(), args

    rc, blocks, threads, lds, t = grid(8, 64, 2, 1)
    assert (rc, blocks, threads) == (0, 1, 256) and t > 0 and t % 32 == 0
    for dec_len, want in ((0, 0), (1, 1), (t - 1, 1), (t, 1), (t + 1, 2), (3 * t + 5, 4), (1 << 27, -(-(1 << 27) // t))):
        assert grid(8, 64, 2, dec_len)[:2] == (0, want), dec_len
    # the filter's operands: 1 KiB per eight channels and 16 taps, 64 KiB at the most
    for L, C, want in ((1, 1, 1), (16, 8, 1), (17, 8, 2), (16, 9, 2), (96, 32, 24), (255, 7, 16), (256, 32, 64), (33, 17, 9)):
        assert grid(12, L, C, 1)[3] == want * 1024, (L, C)
    for args, word in (((0, 8, 1, 1), "decim"), ((8, 257, 1, 1), "ntaps"), ((8, 8, 0, 1), "nchannels"), ((8, 8, 33, 1), "nchannels"),
                       ((8, 8, 1, -1), "dec_len"), ((8, 8, 1, 1 << 62), "grid")):
        assert grid(*args)[0] == -1 and word in built.ddcfir_last_error(), args
    assert built.ddcfir_lib().rtlws_ddcfir_grid(8, 8, 1, 1, None, None, None, None) == 0


def test_ddcfir_refusals_need_no_gpu(built):
    ok = built.ddcfir_supported
    for r in (1, 3, 8, 10, 12, 16, 17, 128):
        for n in (1, r, 17, 255, 256):
            for c in (1, 8, 9, 32):
                assert ok(r, n, c) == 1 and built.ddcfir_last_error() == "", (r, n, c)
    for r, n, c, word in ((0, 8, 1, "decim"), (129, 8, 1, "decim"), (-1, 8, 1, "decim"), (8, 0, 1, "ntaps"), (8, 257, 1, "ntaps"),
                          (8, 8, 0, "nchannels"), (8, 8, 33, "nchannels")):
        assert ok(r, n, c) == 0 and word in built.ddcfir_last_error(), (r, n, c)

    # open: the shape, the taps, their limit (and why), then the engine -- no engine, no plan: a text, never a crash
    L = built.ddcfir_lib()
    good = np.full(8, 16384, np.int16)

    def open_(r, n, taps):
        return L.rtlws_ddcfir_open(None, r, n, None if taps is None else taps.ctypes.data), built.ddcfir_last_error()

    for r, n, taps, word in ((0, 8, good, "decim"), (129, 8, good, "decim"), (8, 0, good, "ntaps"), (8, 257, good, "ntaps"),
                             (8, 8, None, "null taps"), (8, 8, good, "no CPU path")):
        h, why = open_(r, n, taps)
        assert not h and word in why, (r, n, why)
    for bad in (32640, 32767, -32640, -32768):
        taps = good.copy()
        taps[5] = bad
        h, why = open_(8, 8, taps)
        assert not h and "32639" in why and "int8" in why, (bad, why)
    for edge in (32639, -32639):                              # the ends of the range pass that check
        taps = good.copy()
        taps[5] = edge
        assert "no CPU path" in open_(8, 8, taps)[1]
    with pytest.raises(RuntimeError):
        built.DdcFirPlan(None, 8, good)
    L.rtlws_ddcfir_close(None)

    # every refusal of rtlws_ddcfir_run that needs no plan is made before the plan is looked at
    A, B = 1 << 20, 2 << 20                                   # stand-ins for device pointers: never dereferenced
    words = (ctypes.c_int * 32)(*([0] * 32))

    def run(**kw):
        w = kw.pop("words", words)
        args = [kw.get(k, d) for k, d in (("plan", None), ("iq", A), ("n", 100), ("first", 0), ("c", 2), ("w", w), ("s", 14),
                                          ("out", B), ("stride", 100), ("st", None))]
        return L.rtlws_ddcfir_run(*args), built.ddcfir_last_error()

    for kw, word in (({"c": 0}, "nchannels"), ({"c": 33}, "nchannels"), ({"n": -1}, "dec_len"), ({"n": 1 << 62, "stride": 1 << 62}, "grid"),
                     ({"first": -1}, "first_dec_index"), ({"s": -1}, "out_shift"), ({"s": 31}, "out_shift"),
                     ({"stride": 99}, "out_stride"), ({"w": None}, "tuning_words"), ({"iq": None}, "null pointer"),
                     ({"out": None}, "null pointer"), ({"iq": A + 8}, "16-byte"), ({"out": B + 4}, "8-byte"), ({}, "null plan"),
                     ({"n": 0, "stride": 0}, "null plan")):
        rc, why = run(**kw)
        assert rc == -1 and word in why and why.startswith("rtlws_ddcfir_run: "), (kw, why)
    for bad in (P // 2, -P // 2 - 1, 1 << 20):
        rc, why = run(words=(ctypes.c_int * 2)(0, bad))
        assert rc == -1 and "tuning word" in why, bad
    assert "null plan" in run(words=(ctypes.c_int * 2)(-P // 2, P // 2 - 1))[1]       # the ends of the range pass
    assert "null plan" in run(words=(ctypes.c_int * 3)(0, 0, P))[1]                   # a word behind nchannels is not read
    assert "null plan" in run(s=0)[1] and "null plan" in run(s=30)[1]
    # a refusal here leaves the unfiltered bank's error slot alone
    assert built.ddc_supported(8, 1) == 1 and run(c=0)[0] == -1 and built.ddc_last_error() == ""


# ---- the yardstick's own properties ---------------------------------------------------------------------------

CASES = [  # (R, L, taps, s)
    (12, 96, ref.design(12, 96), 14), (12, 96, ref.design(12, 96), 0), (8, 64, ref.random_taps(64, 1), 7),
    (128, 256, np.full(256, ref.MAX_TAP), 0), (3, 256, np.full(256, -ref.MAX_TAP), 0), (17, 255, ref.random_taps(255, 2), 30),
    (1, 1, np.array([ref.MAX_TAP]), 0), (10, 11, ref.random_taps(11, 3), 14), (16, 7, np.array([1, -1, 2, -2, 0, 75, -74]), 0)]


@pytest.mark.parametrize("case", range(len(CASES)))
def test_reference_stays_within_the_bound_of_the_ideal(case):
    """|ddcfir_ref - ideal| <= ref.bound per component, at g0 = 123 456 789, over random and 0 / 255
    bytes, extreme taps and the extreme words."""
    R, L, taps, s = CASES[case]
    limit = ref.bound(taps, s)
    worst = 0.0
    for make in (ref.random_iq, ref.full_scale_iq):
        iq = make(ref.samples_needed(R, L, 300), seed=100 + case)
        got = ref.ddcfir_ref(iq, R, taps, ref.K_SET, s, FIRST)
        worst = max(worst, np.abs(got - ref.ddcfir_ideal(iq, R, taps, ref.K_SET, s, FIRST)).max())
    print("R = %d, L = %d, s = %d: worst |ref - ideal| = %.4f, bound %.4f" % (R, L, s, worst, limit))
    assert worst <= limit


def test_reference_boxcar_is_the_unfiltered_reference():
    """L = R, h = 16384 throughout, s = 14: G = T exactly and the shift is 28."""
    for R in ddc_ref.R_SET:
        for make in (ref.random_iq, ref.full_scale_iq):
            iq = make(R * 257, seed=R)
            got = ref.ddcfir_ref(iq, R, ref.boxcar(R), ddc_ref.K_SET, 14, FIRST)
            assert np.array_equal(got, ddc_ref.ddc_ref(iq, R, ddc_ref.K_SET, FIRST)), R


def test_reference_of_a_capture_of_128s_is_zero():
    for R, L, taps, s in CASES:
        iq = np.full((ref.samples_needed(R, L, 50), 2), 128, np.uint8)
        assert not ref.ddcfir_ref(iq, R, taps, ref.K_SET, s, FIRST).any()


def test_reference_chunks_equal_the_whole():
    for R, L, first in ((8, 64, 0), (7, 33, FIRST), (12, 5, (1 << 40) + 12345)):
        taps = ref.random_taps(L, seed=L)
        words = [777, -20001, -32768, 32767, 1]
        n = 300
        iq = ref.random_iq(ref.samples_needed(R, L, n), seed=R)
        whole = ref.ddcfir_ref(iq, R, taps, words, 9, first)
        cuts = (0, 1, 130, n)
        parts = [ref.ddcfir_ref(iq[a * R:ref.samples_needed(R, L, b - a) + a * R], R, taps, words, 9, first + a)
                 for a, b in zip(cuts, cuts[1:])]
        assert np.array_equal(np.concatenate(parts, axis=1), whole), R
        assert not np.array_equal(ref.ddcfir_ref(iq[130 * R:], R, taps, words, 9, first), whole[:, 130:])     # the index matters


def test_selectivity_of_the_designed_filter_and_of_the_boxcar(built):
    """A u8 tone of amplitude 100, 1.5 output bandwidths (1.5 / R cycles per sample) off the centre of an R = 12
    channel, against the same tone at the centre: the designed 96-tap filter holds it below -40 dB (measured -57.66 dB;
    the Hamming window's stop band is about -53 dB, the threshold the margin of DESIGN.md 4.14), the boxcar's sinc lets
    it through above -15 dB (measured -13.24 dB)."""
    designed = ref.selectivity_db(ref.ddcfir_ref, built.ddcfir_design(12, 96))
    boxcar = ref.selectivity_db(ref.ddcfir_ref, ref.boxcar(12))
    print("designed L = 96: %.2f dB, boxcar L = 12: %.2f dB" % (designed, boxcar))
    assert designed <= -40.0
    assert boxcar >= -15.0

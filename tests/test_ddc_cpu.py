"""CPU suite of include/rtlws_ddc.h (librtlws_ddc.so): the ABI, the kernels' resources from the code-object metadata,
the phasor table, the tuning word, the refusals -- and the numpy restatement's own properties (tests/ddc_ref.py),
which hold the yardstick rather than the code under test.  No GPU is used."""
import ctypes
import re
import subprocess

import numpy as np
import pytest

import ddc_ref
from test_abi_cpu import _declared_by_lib, _declared_functions, _exported

P = ddc_ref.P


def test_ddc_library_exports_its_header_and_nothing_else(built):
    built.ddc_lib()
    declared = _declared_functions("rtlws_ddc.h")
    assert len(declared) == 8
    assert _exported(built.DDC_LIB) == set(declared)
    assert set(built.DDC_SYMBOLS) == set(declared)
    dyn = subprocess.run(["readelf", "-d", built.DDC_LIB], capture_output=True, text=True, check=True).stdout
    assert "librtlws_hip.so" in dyn and "$ORIGIN" in dyn
    # the existing libraries export what they exported
    for lib, names in _declared_by_lib().items():
        assert _exported(getattr(built, lib)) == set(names), lib
    for lib, header in (("FM_LIB", "rtlws_fm.h"), ("LONG_LIB", "rtlws_long.h"), ("ANYLEN_LIB", "rtlws_anylen.h")):
        assert _exported(getattr(built, lib)) == set(_declared_functions(header)), lib
    assert built.DDC_LOG2_PERIOD == ddc_ref.LOG2_P


def test_ddc_kernels_do_not_spill(built):
    """Every kernel of the library: no scratch, no spilled register; the kernel names are exactly the
    instantiations the launch table reaches (R = 8, 10, 12 and the generic one)."""
    from rtlws import codeobj
    built.ddc_lib()
    ks = codeobj.kernels(built.DDC_LIB)
    names = {}
    for k in ks:
        d = k.get("demangled", k["name"])
        m = re.search(r"rtlws::ddc::(ddc_bank_kernel<\d+>)", d)
        assert m, d
        names[m.group(1)] = k
        assert k["vgpr_spill_count"] == 0 and k["private_segment_fixed_size"] == 0, d
        assert not k.get("sgpr_spill_count", 0), d
        assert k["max_flat_workgroup_size"] == 256
    assert set(names) == {"ddc_bank_kernel<%d>" % r for r in (0, 8, 10, 12)} and len(ks) == 4
    # rtlws_ddc_grid reports what the code objects ask for
    for r, name in ((8, "ddc_bank_kernel<8>"), (10, "ddc_bank_kernel<10>"), (12, "ddc_bank_kernel<12>"),
                    (7, "ddc_bank_kernel<0>"), (128, "ddc_bank_kernel<0>")):
        rc, blocks, threads, lds, tile = built.ddc_grid(r, 8, 1)
        assert rc == 0 and threads == 256 and blocks == 1
        assert lds == names[name]["group_segment_fixed_size"], (r, lds)


def test_phasor_table_equals_numpy(built):
    got = built.ddc_table()
    want = ddc_ref.table()
    assert got.shape == (P, 2) and got.dtype == np.int16
    assert np.array_equal(got, want)
    assert tuple(got[0]) == (16384, 0) and tuple(got[P // 4]) == (0, 16384) and tuple(got[P // 2]) == (-16384, 0)
    assert built.ddc_lib().rtlws_ddc_table(None) == -1 and "null" in built.ddc_last_error()


def test_tuning_word(built):
    tw = built.ddc_tuning_word
    fs = 2.4e6
    assert tw(0.0, fs) == (0, 0)
    assert tw(fs / 2, fs) == (0, -P // 2) and tw(-fs / 2, fs) == (0, -P // 2)        # +fs/2 wraps
    assert tw(fs / 4, fs) == (0, P // 4) and tw(-fs / 4, fs) == (0, -P // 4)
    assert tw(fs, fs) == (0, 0) and tw(fs + fs / 4, fs) == (0, P // 4)
    for off in (100e3, -100e3, 433.0e3, -1.19e6, 12.5):                              # offsets that round
        x = off / fs * P
        assert x != np.rint(x)
        want = int((int(np.rint(x)) + P // 2) % P - P // 2)
        assert tw(off, fs) == (0, want), off
    assert tw(100e3, fs)[1] == 2731
    for bad in ((1.0, 0.0), (1.0, -1.0), (float("nan"), fs), (1.0, float("inf")), (float("inf"), fs), (1.0, float("nan"))):
        assert tw(*bad)[0] == -1 and built.ddc_last_error(), bad
    assert built.ddc_lib().rtlws_ddc_tuning_word(1.0, 2.0, None) == -1


def test_ddc_refusals_need_no_gpu(built):
    ok = built.ddc_supported
    for r in (1, 7, 8, 10, 12, 16, 17, 128):
        for c in (1, 8, 9, 32):
            assert ok(r, c) == 1 and built.ddc_last_error() == "", (r, c)
    for r, c, word in ((0, 1, "cic_r"), (129, 1, "cic_r"), (-1, 1, "cic_r"), (8, 0, "nchannels"), (8, 33, "nchannels")):
        assert ok(r, c) == 0 and word in built.ddc_last_error(), (r, c)

    # the grid at a tile border
    rc, blocks, threads, lds, t = built.ddc_grid(8, 2, 1)
    assert rc == 0 and t > 0 and t % 16 == 0
    for dec_len, want in ((0, 0), (1, 1), (t - 1, 1), (t, 1), (t + 1, 2), (3 * t + 5, 4), (1 << 27, -(-(1 << 27) // t))):
        assert built.ddc_grid(8, 2, dec_len)[:2] == (0, want), dec_len
    assert built.ddc_grid(0, 1, 1)[0] == -1 and built.ddc_grid(8, 33, 1)[0] == -1 and built.ddc_grid(8, 1, -1)[0] == -1
    assert built.ddc_grid(8, 1, 1 << 62)[0] == -1 and "grid" in built.ddc_last_error()
    L = built.ddc_lib()
    assert L.rtlws_ddc_grid(8, 1, 1, None, None, None, None) == 0

    # no engine, no plan: a text, never a crash
    assert not L.rtlws_ddc_open(None) and "no CPU path" in built.ddc_last_error()
    with pytest.raises(RuntimeError):
        built.DdcPlan(None)
    L.rtlws_ddc_close(None)

    # every refusal of rtlws_ddc_run is made before the plan is asked for anything
    A, B = 1 << 20, 2 << 20                                   # stand-ins for device pointers: never dereferenced
    words = (ctypes.c_int * 32)(*([0] * 32))

    def run(**kw):
        w = kw.pop("words", words)
        args = [kw.get(k, d) for k, d in (("plan", None), ("r", 8), ("iq", A), ("n", 100), ("first", 0), ("c", 2),
                                          ("w", w), ("out", B), ("stride", 100), ("st", None))]
        return L.rtlws_ddc_run(*args), built.ddc_last_error()

    for kw, word in (({"r": 0}, "cic_r"), ({"r": 129}, "cic_r"), ({"c": 0}, "nchannels"), ({"c": 33}, "nchannels"),
                     ({"n": -1}, "dec_len"), ({"first": -1}, "first_dec_index"), ({"stride": 99}, "out_stride"),
                     ({"w": None}, "tuning_words"), ({"iq": None}, "null pointer"), ({"out": None}, "null pointer"),
                     ({"iq": A + 8}, "16-byte"), ({"out": B + 4}, "8-byte"), ({}, "null plan")):
        rc, why = run(**kw)
        assert rc == -1 and word in why, (kw, why)
    for bad in (P // 2, -P // 2 - 1, 1 << 20):
        w = (ctypes.c_int * 2)(0, bad)
        rc, why = run(words=w)
        assert rc == -1 and "tuning word" in why, bad
    w = (ctypes.c_int * 2)(-P // 2, P // 2 - 1)               # the ends of the range pass that check
    assert "null plan" in run(words=w)[1]
    w = (ctypes.c_int * 3)(0, 0, P)                           # a word behind nchannels is not read
    assert "null plan" in run(words=w)[1]


# ---- the yardstick's own properties ---------------------------------------------------------------------------

def test_reference_with_word_zero_is_the_block_sum():
    for R in ddc_ref.R_SET:
        for make in (ddc_ref.random_iq, ddc_ref.full_scale_iq):
            iq = make(R * 257, seed=R)
            got = ddc_ref.ddc_ref(iq, R, [0], first_dec_index=123456789)
            assert np.array_equal(got[0], ddc_ref.block_sums(iq, R)), R


def test_reference_chunks_equal_the_whole():
    for R, first in ((8, 0), (7, 123456789), (12, (1 << 40) + 12345)):
        iq = ddc_ref.random_iq(R * 300, seed=R)
        words = [777, -20001, -32768, 32767, 1]
        whole = ddc_ref.ddc_ref(iq, R, words, first)
        cuts = (0, 1, 130, 300)
        parts = [ddc_ref.ddc_ref(iq[a * R:b * R], R, words, first + a) for a, b in zip(cuts, cuts[1:])]
        assert np.array_equal(np.concatenate(parts, axis=1), whole), R
        assert not np.array_equal(ddc_ref.ddc_ref(iq[130 * R:], R, words, first), whole[:, 130:])     # the index matters


@pytest.mark.parametrize("R", ddc_ref.R_SET)
def test_reference_stays_within_the_bound_of_the_ideal(R):
    """|ddc_ref - ideal| <= 0.5 + R / 64 per component: the output rounding (0.5), R phasors each rounded by at most
    0.5 / S in each part against samples of at most 128 per part (R * 2 * 128 * 0.5 / 16384 = R / 128), and the
    rounded block phasor against |U| <= R * 181 * S (at most another R / 128 with the cross terms)."""
    words = list(ddc_ref.K_SET)
    first = 123456789
    worst = 0.0
    for make in (ddc_ref.random_iq, ddc_ref.full_scale_iq):
        iq = make(R * 400, seed=100 + R)
        err = np.abs(ddc_ref.ddc_ref(iq, R, words, first) - ddc_ref.ddc_ideal(iq, R, words, first)).max()
        worst = max(worst, err)
    print("R = %d: worst |ref - ideal| = %.4f, bound %.4f" % (R, worst, 0.5 + R / 64))
    assert worst <= 0.5 + R / 64

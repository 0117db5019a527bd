"""CPU suite of the tuned-channel family as a family (include/rtlws_ddc.h, rtlws_fmbank.h, rtlws_ddcfir.h): the rules
the three libraries share -- the nchannels and cic_r ranges, the count of decimated samples and "one grid holds",
first_dec_index, the tuning words, the capture's pointer and alignment, null engine, null plan -- are refused in the
same words by every entry point that has the rule (the text behind the "function: " prefix); and every library keeps
an error slot of its own: a refusal in one leaves the other two's *_last_error(), and rtlws_pfb's, empty.  No GPU is
used."""
import ctypes as C

import numpy as np
import pytest

LIBS = ("ddc", "fmbank", "ddcfir")
P = 1 << 16
A, B, S, T = 1 << 20, 2 << 20, 3 << 20, 4 << 20                  # stand-ins for device pointers: never dereferenced
ZEROS = (C.c_int * 32)(*([0] * 32))

NCHANNELS = "nchannels must be 1 .. 32"
CIC_R = "cic_r must be 1 .. 128"
DEC_LEN = "dec_len must be >= 0"
GRID = "more decimated samples than one grid holds"
FIRST = "first_dec_index must be >= 0"
OUT_STRIDE = "out_stride must be >= dec_len"
NULL_WORDS = "null tuning_words"
WORD = "a tuning word lies outside [-32768, 32768)"
NULL_POINTER = "null pointer"
CAPTURE_ALIGNED = "d_iq_cu8 must be 16-byte aligned"
OUT_ALIGNED = "d_out_cs32 must be 8-byte aligned"
NULL_ENGINE = "null engine (no usable HIP device: there is no CPU path)"
NULL_PLAN = "null plan (no usable HIP device: there is no CPU path)"


@pytest.fixture(scope="module")
def fam(built):
    class Family:
        lib = {n: getattr(built, n + "_lib")() for n in LIBS}

        @staticmethod
        def err(n):
            return getattr(built, n + "_last_error")()

        @classmethod
        def why(cls, n, fn):
            """The text behind "<fn>: " of library n's last error."""
            text = cls.err(n)
            assert text.startswith(fn + ": "), (n, fn, text)
            return text[len(fn) + 2:]

        @classmethod
        def f(cls, n, what):
            return getattr(cls.lib[n], "rtlws_%s_%s" % (n, what))

        # one call per entry point with the shared arguments named and otherwise valid ones; r is cic_r (the filtered
        # bank's decim and ntaps are its plan's and stay valid), n the count of decimated samples (the FM bank: blocks)
        @classmethod
        def supported(cls, n, r=8, c=1):
            return cls.f(n, "supported")(*{"ddc": (r, c), "fmbank": (r, c, 20, 1), "ddcfir": (8, 8, c)}[n])

        @classmethod
        def grid(cls, n, r=8, c=1, count=1):
            head = {"ddc": (r, c, count), "fmbank": (r, c, 20, count), "ddcfir": (8, 8, c, count)}[n]
            return cls.f(n, "grid")(*head, None, None, None, None)

        @classmethod
        def open(cls, n):
            taps = np.full(8, 16384, np.int16)
            return cls.f(n, "open")(None, *((8, 8, taps.ctypes.data) if n == "ddcfir" else ()))

        # the runs without a plan: 100 decimated samples (the FM bank: 10 blocks of 20) of two channels
        @classmethod
        def run(cls, n, r=8, iq=A, count=None, first=0, c=2, w=ZEROS, out=B, stride=None):
            if n == "fmbank":
                count = 10 if count is None else count
                return cls.f(n, "run")(None, r, iq, 20, count, first, c, w, S, T, out, 5 * max(count, 0) if stride is None else stride, None)
            count = 100 if count is None else count
            stride = count if stride is None else stride
            if n == "ddc":
                return cls.f(n, "run")(None, r, iq, count, first, c, w, out, stride, None)
            return cls.f(n, "run")(None, iq, count, first, c, w, 14, out, stride, None)

    return Family


def run_fn(n):
    return "rtlws_%s_run" % n


COUNTED = ("ddc", "ddcfir")                                     # the libraries that count decimated samples
FACTORED = ("ddc", "fmbank")                                    # the libraries whose calls take cic_r


def test_the_nchannels_range_is_refused_in_the_same_words(fam):
    for c in (0, 33, -1):
        for n in LIBS:
            assert fam.supported(n, c=c) == 0 and fam.why(n, "rtlws_" + n) == NCHANNELS, (n, c)
            assert fam.grid(n, c=c) == -1 and fam.why(n, "rtlws_%s_grid" % n) == NCHANNELS, (n, c)
            assert fam.run(n, c=c) == -1 and fam.why(n, run_fn(n)) == NCHANNELS, (n, c)
    for c in (1, 32):
        for n in LIBS:
            assert fam.supported(n, c=c) == 1 and fam.err(n) == "", (n, c)


def test_the_cic_r_range_is_refused_in_the_same_words(fam):
    for r in (0, 129, -1):
        for n in FACTORED:
            assert fam.supported(n, r=r) == 0 and fam.why(n, "rtlws_" + n) == CIC_R, (n, r)
            assert fam.grid(n, r=r) == -1 and fam.why(n, "rtlws_%s_grid" % n) == CIC_R, (n, r)
            assert fam.run(n, r=r) == -1 and fam.why(n, run_fn(n)) == CIC_R, (n, r)
    for r in (1, 128):
        for n in FACTORED:
            assert fam.supported(n, r=r) == 1 and fam.err(n) == "", (n, r)
    # the factor comes before the channels where a call takes both
    for n in FACTORED:
        assert fam.supported(n, r=0, c=0) == 0 and fam.why(n, "rtlws_" + n) == CIC_R, n


def test_the_count_and_one_grid_holds_are_refused_in_the_same_words(fam):
    need = fam.f("ddcfir", "samples_needed")
    for count, want in ((-1, DEC_LEN), (1 << 62, GRID), (((1 << 31) - 1) * 1024 + 1, GRID)):
        for n in COUNTED:
            assert fam.grid(n, count=count) == -1 and fam.why(n, "rtlws_%s_grid" % n) == want, (n, count)
            assert fam.run(n, count=count) == -1 and fam.why(n, run_fn(n)) == want, (n, count)
        assert need(8, 8, count) == -1 and fam.why("ddcfir", "rtlws_ddcfir_samples_needed") == want, count
    # 1024 decimated samples to a workgroup: the largest grid passes
    for n in COUNTED:
        assert fam.grid(n, count=((1 << 31) - 1) * 1024) == 0 and fam.err(n) == "", n
    assert need(8, 8, ((1 << 31) - 1) * 1024) > 0 and fam.err("ddcfir") == ""
    # the rows hold the count
    for n in COUNTED:
        assert fam.run(n, count=100, stride=99) == -1 and fam.why(n, run_fn(n)) == OUT_STRIDE, n


def test_first_dec_index_is_refused_in_the_same_words(fam):
    for n in LIBS:
        assert fam.run(n, first=-1) == -1 and fam.why(n, run_fn(n)) == FIRST, n
        assert fam.run(n, first=(1 << 62)) == -1 and fam.why(n, run_fn(n)) == NULL_PLAN, n


def test_the_tuning_words_are_refused_in_the_same_words(fam):
    for n in LIBS:
        assert fam.run(n, w=None) == -1 and fam.why(n, run_fn(n)) == NULL_WORDS, n
        for bad in (P // 2, -P // 2 - 1, 1 << 20):
            for words in ((C.c_int * 2)(0, bad), (C.c_int * 2)(bad, 0)):
                assert fam.run(n, w=words) == -1 and fam.why(n, run_fn(n)) == WORD, (n, bad)
        # the ends of the range pass, and a word behind nchannels is not read
        assert fam.run(n, w=(C.c_int * 2)(-P // 2, P // 2 - 1)) == -1 and fam.why(n, run_fn(n)) == NULL_PLAN, n
        assert fam.run(n, w=(C.c_int * 3)(0, 0, P)) == -1 and fam.why(n, run_fn(n)) == NULL_PLAN, n
        assert fam.run(n, c=32, w=(C.c_int * 32)(*([P // 2 - 1] * 31 + [P // 2]))) == -1 and fam.why(n, run_fn(n)) == WORD, n


def test_the_capture_is_refused_in_the_same_words(fam):
    for n in LIBS:
        assert fam.run(n, iq=None) == -1 and fam.why(n, run_fn(n)) == NULL_POINTER, n
        assert fam.run(n, out=None) == -1 and fam.why(n, run_fn(n)) == NULL_POINTER, n
        for off in (1, 4, 8):
            assert fam.run(n, iq=A + off) == -1 and fam.why(n, run_fn(n)) == CAPTURE_ALIGNED, (n, off)
        # nothing to do: the pointers may be null, their alignment is still looked at
        assert fam.run(n, count=0, iq=None, out=None) == -1 and fam.why(n, run_fn(n)) == NULL_PLAN, n
        assert fam.run(n, count=0, iq=A + 8) == -1 and fam.why(n, run_fn(n)) == CAPTURE_ALIGNED, n
    for n in COUNTED:
        assert fam.run(n, out=B + 4) == -1 and fam.why(n, run_fn(n)) == OUT_ALIGNED, n
        assert fam.run(n, iq=A + 8, out=B + 4) == -1 and fam.why(n, run_fn(n)) == CAPTURE_ALIGNED, n


def test_null_engine_and_plan_are_refused_in_the_same_words(fam):
    for n in LIBS:
        assert not fam.open(n) and fam.why(n, "rtlws_%s_open" % n) == NULL_ENGINE, n
        fam.f(n, "close")(None)
        assert fam.run(n) == -1 and fam.why(n, run_fn(n)) == NULL_PLAN, n
        assert fam.run(n, count=0) == -1 and fam.why(n, run_fn(n)) == NULL_PLAN, n


@pytest.mark.parametrize("refuser", LIBS)
def test_a_refusal_stays_in_its_own_library(built, fam, refuser):
    """Every library's error slot is its own: after a refusal by one -- of a size function, of open, of a run -- the
    other two's *_last_error(), and the polyphase channelizer's, are as empty as their last accepted call left them."""
    refusals = [lambda: fam.supported(refuser, c=0), lambda: fam.grid(refuser, c=33), lambda: fam.open(refuser),
                lambda: fam.run(refuser), lambda: fam.run(refuser, w=None), lambda: fam.run(refuser, iq=A + 8)]
    for refuse in refusals:
        for n in LIBS:
            assert fam.supported(n) == 1 and fam.err(n) == "", n
        assert built.pfb_supported(6, 8, 64) == 1 and built.pfb_last_error() == ""
        refuse()
        assert fam.err(refuser).startswith("rtlws_" + refuser), refuser
        for n in LIBS:
            if n != refuser:
                assert fam.err(n) == "", (refuser, n, fam.err(n))
        assert built.pfb_last_error() == "", refuser

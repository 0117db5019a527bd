"""CPU suite of the polyphase family as a family (include/rtlws_pfb.h, rtlws_pfbspec.h, rtlws_pfbxc.h, rtlws_pfbbf.h):
the rules the four libraries share -- the bank's shape, the hop, the k_avg range, "one grid holds", null taps, null
engine, null plan -- are refused in the same words by every library that has the rule (the text behind the
"function: " prefix), the beamformer's documented k_avg wording apart; and every library keeps an error slot of its
own: a refusal in one leaves the other three's *_last_error() empty.  No GPU is used."""
import ctypes as C

import numpy as np
import pytest

LIBS = ("pfb", "pfbspec", "pfbxc", "pfbbf")
A, W, X, Y = 1 << 20, 2 << 20, 3 << 20, 4 << 20                 # stand-ins for device pointers: never dereferenced
IQS = (C.c_void_p * 2)(A, A + 4096)

SHAPE = "log2_channels must be 4 .. 10"
TAPS = "taps_per_branch must be 1 .. 32"
HOP = "hop must be M or M / 2"
K_AVG = "k_avg must be 1 .. 65536"
K_AVG_BF = "k_avg must be 1 .. 65536 (0: voltage mode)"         # rtlws_pfbbf.h: its size functions take k_avg 0
GRID_FRAMES = "more frames than one grid holds"
GRID_SPECTRA = "more spectra than one grid holds"
NULL_TAPS = "null taps"
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

        # one call per entry point with the bank's arguments in front and otherwise valid ones: (library, function) -> call
        @classmethod
        def supported(cls, n, k, T, hop, k_avg=1):
            tail = {"pfb": (), "pfbspec": (k_avg, 0), "pfbxc": (k_avg, 2), "pfbbf": (2, 1)}[n]
            return cls.f(n, "supported")(k, T, hop, *tail)

        @classmethod
        def samples_needed(cls, n, k, T, hop, k_avg, count):
            return cls.f(n, "samples_needed")(*((k, T, hop, count) if n == "pfb" else (k, T, hop, k_avg, count)))

        @classmethod
        def grid(cls, n, k, T, hop, k_avg, count):
            head = {"pfb": (k, T, hop, count), "pfbspec": (k, T, hop, k_avg, count), "pfbxc": (k, T, hop, k_avg, 2, count),
                    "pfbbf": (k, T, hop, k_avg, count)}[n]
            return cls.f(n, "grid")(*head, None, None, None, None)

        @classmethod
        def open(cls, n, k, T, taps):
            tail = {"pfb": (), "pfbspec": (), "pfbxc": (2,), "pfbbf": (2, 1)}[n]
            return cls.f(n, "open")(None, k, T, None if taps is None else taps.ctypes.data, *tail)

        # the runs without a plan: 100 frames or spectra of a 64-channel bank, rows 64 apart
        @classmethod
        def run(cls, fn, hop=64, k_avg=3, n=100):
            if fn == "rtlws_pfb_run":
                return cls.lib["pfb"].rtlws_pfb_run(None, A, n, hop, 0, 1, X, 64, None)
            if fn == "rtlws_pfbspec_run":
                return cls.lib["pfbspec"].rtlws_pfbspec_run(None, A, n, hop, k_avg, 0, 0, 1.0, X, 64, None)
            if fn == "rtlws_pfbxc_run":
                return cls.lib["pfbxc"].rtlws_pfbxc_run(None, IQS, n, hop, k_avg, 0, X, 64, Y, 64, None)
            if fn == "rtlws_pfbbf_run":
                return cls.lib["pfbbf"].rtlws_pfbbf_run(None, IQS, 2, W, 1, n, hop, 0, 1, X, 64, 64 * min(max(n, 1), 1 << 40), None)
            assert fn == "rtlws_pfbbf_power"
            return cls.lib["pfbbf"].rtlws_pfbbf_power(None, IQS, 2, W, 1, n, hop, k_avg, 0, X, 64, None)

    return Family


RUNS = (("pfb", "rtlws_pfb_run"), ("pfbspec", "rtlws_pfbspec_run"), ("pfbxc", "rtlws_pfbxc_run"), ("pfbbf", "rtlws_pfbbf_run"),
        ("pfbbf", "rtlws_pfbbf_power"))
SUMS = ("pfbspec", "pfbxc", "pfbbf")                            # the libraries whose size functions take k_avg


def test_the_bank_shape_is_refused_in_the_same_words(fam):
    taps = np.ones(64, np.int16)
    for k, T, hop, want in ((3, 1, 8, SHAPE), (11, 1, 2048, SHAPE), (6, 0, 64, TAPS), (6, 33, 64, TAPS)):
        for n in LIBS:
            assert fam.supported(n, k, T, hop) == 0 and fam.why(n, "rtlws_" + n) == want, (n, k, T)
            assert fam.samples_needed(n, k, T, hop, 1, 1) == -1 and fam.why(n, "rtlws_%s_samples_needed" % n) == want, (n, k, T)
            assert fam.grid(n, k, T, hop, 1, 1) == -1 and fam.why(n, "rtlws_%s_grid" % n) == want, (n, k, T)
            assert not fam.open(n, k, T, taps) and fam.why(n, "rtlws_%s_open" % n) == want, (n, k, T)
    # the shape comes before the hop, K and the count in every library
    for n in LIBS:
        assert fam.samples_needed(n, 3, 33, 48, 65537, -1) == -1 and fam.why(n, "rtlws_%s_samples_needed" % n) == SHAPE, n
        assert fam.samples_needed(n, 6, 33, 48, 65537, -1) == -1 and fam.why(n, "rtlws_%s_samples_needed" % n) == TAPS, n


def test_the_hop_is_refused_in_the_same_words(fam):
    for hop in (0, 4, 16, 48, 128, 2048, -64):
        for n in LIBS:
            assert fam.supported(n, 6, 8, hop) == 0 and fam.why(n, "rtlws_" + n) == HOP, (n, hop)
            assert fam.samples_needed(n, 6, 8, hop, 1, 1) == -1 and fam.why(n, "rtlws_%s_samples_needed" % n) == HOP, (n, hop)
            assert fam.grid(n, 6, 8, hop, 1, 1) == -1 and fam.why(n, "rtlws_%s_grid" % n) == HOP, (n, hop)
    # a run says it before it looks at its plan: no power of two 8 .. 1024
    for hop in (0, 4, 48, 2048, -64):
        for n, fn in RUNS:
            assert fam.run(fn, hop=hop) == -1 and fam.why(n, fn) == HOP, (fn, hop)


def test_the_k_avg_range_is_refused_in_the_same_words(fam):
    for k_avg in (-1, 65537):
        for n in SUMS:
            want = K_AVG_BF if n == "pfbbf" else K_AVG
            assert fam.samples_needed(n, 6, 8, 64, k_avg, 1) == -1 and fam.why(n, "rtlws_%s_samples_needed" % n) == want, (n, k_avg)
            assert fam.grid(n, 6, 8, 64, k_avg, 1) == -1 and fam.why(n, "rtlws_%s_grid" % n) == want, (n, k_avg)
    for k_avg in (0, -1, 65537):
        for n in ("pfbspec", "pfbxc"):
            assert fam.supported(n, 6, 8, 64, k_avg) == 0 and fam.why(n, "rtlws_" + n) == K_AVG, (n, k_avg)
        for n, fn in RUNS[1:3] + RUNS[4:]:
            assert fam.run(fn, k_avg=k_avg) == -1 and fam.why(n, fn) == K_AVG, (fn, k_avg)
    # 0 is the beamformer's voltage mode where it counts frames, and no K anywhere else
    assert fam.samples_needed("pfbbf", 6, 8, 64, 0, 1) == 512 and fam.err("pfbbf") == ""
    for n in ("pfbspec", "pfbxc"):
        assert fam.samples_needed(n, 6, 8, 64, 0, 1) == -1 and fam.why(n, "rtlws_%s_samples_needed" % n) == K_AVG, n


def test_one_grid_holds_is_refused_in_the_same_words(fam):
    # frames: 64 to a workgroup of the 64-channel bank; spectra: one to a workgroup at K >= 64, 64 / K below
    for n, k_avg in (("pfb", 0), ("pfbbf", 0)):
        assert fam.samples_needed(n, 6, 8, 64, k_avg, 1 << 40) == -1 and fam.why(n, "rtlws_%s_samples_needed" % n) == GRID_FRAMES, n
        assert fam.grid(n, 6, 8, 64, k_avg, 1 << 40) == -1 and fam.why(n, "rtlws_%s_grid" % n) == GRID_FRAMES, n
        assert fam.samples_needed(n, 6, 8, 64, k_avg, ((1 << 31) - 1) * 64) > 0 and fam.err(n) == "", n
    for n in SUMS:
        for k_avg, count in ((1, 1 << 40), (64, 1 << 31), (65536, 1 << 31)):
            assert fam.samples_needed(n, 6, 8, 64, k_avg, count) == -1, (n, k_avg)
            assert fam.why(n, "rtlws_%s_samples_needed" % n) == GRID_SPECTRA, (n, k_avg)
            assert fam.grid(n, 6, 8, 64, k_avg, count) == -1 and fam.why(n, "rtlws_%s_grid" % n) == GRID_SPECTRA, (n, k_avg)
        assert fam.samples_needed(n, 6, 8, 64, 1, ((1 << 31) - 1) * 64) > 0 and fam.err(n) == "", n
        assert fam.samples_needed(n, 6, 8, 64, 64, (1 << 31) - 1) > 0 and fam.err(n) == "", n
    # a run says it before it looks at its plan, for the smallest bank's workgroups
    for n, fn in RUNS:
        want = GRID_FRAMES if fn in ("rtlws_pfb_run", "rtlws_pfbbf_run") else GRID_SPECTRA
        assert fam.run(fn, n=1 << 62) == -1 and fam.why(n, fn) == want, fn
    for n, fn in RUNS[1:3] + RUNS[4:]:
        assert fam.run(fn, k_avg=300, n=1 << 31) == -1 and fam.why(n, fn) == GRID_SPECTRA, fn


def test_null_taps_engine_and_plan_are_refused_in_the_same_words(fam):
    taps = np.ones(64, np.int16)
    for n in LIBS:
        assert not fam.open(n, 6, 1, None) and fam.why(n, "rtlws_%s_open" % n) == NULL_TAPS, n
        assert not fam.open(n, 6, 1, taps) and fam.why(n, "rtlws_%s_open" % n) == NULL_ENGINE, n
        fam.f(n, "close")(None)
    for n, fn in RUNS:
        assert fam.run(fn) == -1 and fam.why(n, fn) == NULL_PLAN, fn
        assert fam.run(fn, n=0) == -1 and fam.why(n, fn) == NULL_PLAN, fn


@pytest.mark.parametrize("refuser", LIBS)
def test_a_refusal_stays_in_its_own_library(fam, refuser):
    """Every library's error slot is its own: after a refusal by one -- of a size function, of open, of a run -- the
    other three's *_last_error() are as empty as their last accepted call left them."""
    taps = np.ones(64, np.int16)
    refusals = [lambda: fam.supported(refuser, 3, 1, 8), lambda: fam.samples_needed(refuser, 6, 8, 48, 1, 1),
                lambda: fam.grid(refuser, 6, 8, 64, 1, 1 << 62), lambda: fam.open(refuser, 6, 1, None),
                lambda: fam.open(refuser, 6, 1, taps)]
    refusals += [lambda fn=fn: fam.run(fn) for n, fn in RUNS if n == refuser]
    for refuse in refusals:
        for n in LIBS:
            assert fam.supported(n, 6, 8, 64) == 1 and fam.err(n) == "", n
        refuse()
        assert fam.err(refuser).startswith("rtlws_" + refuser), refuser
        for n in LIBS:
            if n != refuser:
                assert fam.err(n) == "", (refuser, n, fam.err(n))

"""CPU suite of include/rtlws_periodlong.h (librtlws_periodlong.so): the ABI, the kernels' resources from the code-object
metadata, the geometry, the refusals and their order, rtlws_periodlong_samples -- and the properties of the numpy
restatement of stage 1 (tests/periodlong_ref.py), which hold the yardstick of tests/test_periodlong_gpu.py rather than
the code under test.  No GPU is used."""
import os
import re
import subprocess

import numpy as np
import pytest

import period_ref
import periodlong_ref
from test_abi_cpu import INCLUDE, _declared_functions, _exported

LOG2NS = range(16, 23)


def test_periodlong_library_exports_its_header_and_nothing_else(built):
    built.periodlong_lib()
    declared = _declared_functions("rtlws_periodlong.h")
    assert len(declared) == 8
    assert _exported(built.PERIODLONG_LIB) == set(declared) == set(built.PERIODLONG_SYMBOLS)
    dyn = subprocess.run(["readelf", "-d", built.PERIODLONG_LIB], capture_output=True, text=True, check=True).stdout
    assert "librtlws_hip.so" in dyn and "$ORIGIN" in dyn
    txt = open(os.path.join(INCLUDE, "rtlws_periodlong.h")).read()
    for name, value in (("MIN_LOG2N", 16), ("MAX_LOG2N", 22), ("MAX_LEVELS", 5), ("MIN_NORM", 16), ("MAX_NORM", 16384), ("MIN_SEG", 64),
                        ("MAX_SEG", 16384), ("MAX_TRIALS", 65536), ("STAGES", 6)):
        assert re.search(r"#define RTLWS_PERIODLONG_%s %d\b" % (name, value), txt) and getattr(built, "PERIODLONG_" + name) == value
        assert getattr(periodlong_ref, name) == value
    assert re.search(r"#define RTLWS_PERIODLONG_WORKSPACE_CAP \(\(size_t\)1 << 30\)", txt)
    assert built.PERIODLONG_WORKSPACE_CAP == periodlong_ref.WORKSPACE_CAP == 1 << 30
    # the false-alarm probability is the short library's: pointed to, not repeated
    assert "rtlws_period_lnq" in txt and "rtlws_periodlong_lnq" not in txt
    # the short library is as it was
    assert len(_declared_functions("rtlws_period.h")) == 8 and _exported(built.PERIOD_LIB) == set(built.PERIOD_SYMBOLS)


def test_periodlong_header_is_strict_c99(built, tmp_path):
    src = tmp_path / "uses_periodlong.c"
    src.write_text('#include "rtlws_periodlong.h"\nint main(void) { return rtlws_periodlong_supported(0, 0, 0, 0, 0) + '
                   '(int)rtlws_periodlong_workspace_bytes(0) + (RTLWS_PERIODLONG_WORKSPACE_CAP > 0); }\n')
    subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Wextra", "-Werror", "-I", INCLUDE, "-fsyntax-only", str(src)], check=True)


def _kernels(built):
    """{(stage name, template argument or None): metadata} of every kernel of the library"""
    from rtlws import codeobj
    built.periodlong_lib()
    names = {}
    for k in codeobj.kernels(built.PERIODLONG_LIB):
        d = k.get("demangled", k["name"])
        m = re.search(r"rtlws::periodlong::(\w+)_kernel(?:<(\d+)>)?", d)
        assert m, d
        names[(m.group(1), int(m.group(2)) if m.group(2) else None)] = k
    return names


# the kernel of every stage at a frame length: (name, template argument)
def _stage_kernels(log2n):
    l1, l2 = periodlong_ref.split(log2n)
    return (("mean", None), ("cols16" if l1 == 4 else "cols256", None), ("rows", l2), ("untangle", l1), ("whiten", None), ("peaks", None))


def test_periodlong_kernels_do_not_spill(built):
    """Every kernel of the library: no scratch, no spilled register, the thread count the geometry names, static plus
    dynamic LDS within the 160 KiB of a compute unit, and no more registers than its workgroup may have: 512 / (threads
    / 256) a thread, so that a workgroup fits one compute unit's 4 x 512 x 64 lanes of registers"""
    names = _kernels(built)
    assert set(names) == {("mean", None), ("cols16", None), ("cols256", None), ("rows", 11), ("rows", 12), ("rows", 13), ("rows", 14),
                          ("untangle", 4), ("untangle", 8), ("whiten", None), ("peaks", None)}
    for key, k in names.items():
        assert k["vgpr_spill_count"] == 0 and k["private_segment_fixed_size"] == 0, key
        assert not k.get("sgpr_spill_count", 0), key
    seen = set()
    for log2n in LOG2NS:
        _, threads, lds, _ = periodlong_ref.geometry(log2n, 64, 1)
        for stage, key in enumerate(_stage_kernels(log2n)):
            k = names[key]
            seen.add(key)
            assert k["max_flat_workgroup_size"] == threads[stage], (log2n, key)
            allowed = min(512, 512 * 256 // threads[stage])
            assert k["vgpr_count"] + (k.get("agpr_count") or 0) <= allowed, (log2n, key, k["vgpr_count"], k.get("agpr_count"))
            static = k["group_segment_fixed_size"]
            # a stage's LDS is either the kernel's own or the launch's
            assert static in (0, lds[stage]) and max(static, lds[stage]) <= 160 * 1024, (log2n, key, static, lds[stage])
    assert seen == set(names)
    assert periodlong_ref.geometry(19, 64, 1)[2][2] == 136 * 1024


def test_geometry_is_the_rule(built):
    for log2n in LOG2NS:
        m = 1 << (log2n - 1)
        for seg in (64, 16384):
            for norm in (16, 16384):
                for ntrials in (1, 257, 65536):
                    got = built.periodlong_geometry(log2n, 5, norm, seg, 1, ntrials)
                    assert got[0] == 0 and built.periodlong_last_error() == "", (log2n, seg, norm)
                    assert got[1:] == periodlong_ref.geometry(log2n, seg, ntrials), (log2n, got)
                    assert got[4] == m // seg and len(got[1]) == len(got[2]) == len(got[3]) == 6
        l1, l2 = periodlong_ref.split(log2n)
        assert l1 + l2 == log2n - 1 and 11 <= l2 <= 14 and l1 in (4, 8)
        # every stage covers the trial once
        blocks, threads, _, _ = periodlong_ref.geometry(log2n, 64, 1)
        assert blocks[0] * (1 << (log2n - 6)) == 1 << log2n                       # mean: stretches of N / 64 samples
        assert blocks[1] * (256 if l1 == 4 else 16) == 1 << l2                    # columns
        assert blocks[2] == 1 << l1 and threads[2] * 16 >= 1 << l2                # rows, a thread a radix-16 butterfly
        assert blocks[3] * 2 * (64 if l1 == 4 else 16) == 1 << l2                 # tiles of bins and of their mirrors
        assert blocks[4] * 16384 == blocks[5] * 16384 == m
    # any pointer may be null
    assert built.periodlong_lib().rtlws_periodlong_geometry(16, 1, 16, 64, 1, 1, None, None, None, None) == 0
    # what is in flight
    assert periodlong_ref.in_flight(16, 65536) == (1 << 30) // (12 * 32768 + 512) and periodlong_ref.in_flight(22, 65536) == 42
    assert periodlong_ref.in_flight(22, 3) == 3


def test_periodlong_refusals_need_no_gpu(built):
    L = built.periodlong_lib()
    err = built.periodlong_last_error
    for log2n in LOG2NS:
        m = 1 << (log2n - 1)
        for levels in (1, 5):
            for norm, seg, klo in ((16, 64, 1), (16384, 16384, m - 1), (64, 256, 8)):
                assert built.periodlong_supported(log2n, levels, norm, seg, klo) == 1 and err() == ""

    def each(log2n=16, levels=5, norm=64, seg=64, klo=8):
        yield "rtlws_periodlong_open", not L.rtlws_periodlong_open(None, log2n, levels, norm, seg, klo, 1), err()
        yield "rtlws_periodlong", L.rtlws_periodlong_supported(log2n, levels, norm, seg, klo) == 0, err()
        yield "rtlws_periodlong_geometry", L.rtlws_periodlong_geometry(log2n, levels, norm, seg, klo, 1, None, None, None, None) == -1, err()

    for kw, word in (({"log2n": 15}, "log2n must be 16 .. 22"), ({"log2n": 23}, "log2n must be"), ({"log2n": -1}, "log2n"),
                     ({"levels": 0}, "levels must be 1 .. 5"), ({"levels": 6}, "levels must be"),
                     ({"norm": 8}, "norm must be a power of two 16 .. 16384"), ({"norm": 48}, "norm must be"), ({"norm": 32768}, "norm must be"),
                     ({"norm": 0}, "norm must be"), ({"norm": -16}, "norm must be"),
                     ({"seg": 32}, "seg must be a power of two 64 .. 16384"), ({"seg": 96}, "seg must be"), ({"seg": 32768}, "seg must be"),
                     ({"seg": 0}, "seg must be"), ({"klo": 0}, "klo must be 1 .. N / 2 - 1"), ({"klo": 32768}, "klo must be"), ({"klo": -3}, "klo must be"),
                     ({"log2n": 22, "klo": 1 << 21}, "klo must be")):
        for fn, refused, why in each(**kw):
            assert refused and word in why and why.startswith(fn + ": "), (kw, fn, why)
    # the borders that are served
    for kw in ({"norm": 16}, {"norm": 16384}, {"seg": 64}, {"seg": 16384}, {"klo": 32767}, {"klo": 1}, {"log2n": 22, "klo": (1 << 21) - 1}):
        assert L.rtlws_periodlong_supported(*[kw.get(k, v) for k, v in (("log2n", 16), ("levels", 5), ("norm", 64), ("seg", 64), ("klo", 8))]) == 1
    # the plan's rules in order: log2n, levels, norm, seg, klo
    chain = (({"log2n": 15}, "log2n"), ({"levels": 0}, "levels"), ({"norm": 3}, "norm must be"), ({"seg": 3}, "seg must be"), ({"klo": 0}, "klo must be"))
    for i, (_, word) in enumerate(chain):
        kw = {}
        for later, _ in reversed(chain[i:]):
            kw.update(later)
        for fn, refused, why in each(**kw):
            assert refused and word in why, (i, fn, why)
    # geometry: the plan's rules, then ntrials
    for ntrials in (0, 65537, -1):
        assert L.rtlws_periodlong_geometry(16, 5, 64, 64, 8, ntrials, None, None, None, None) == -1 and "ntrials must be 1 .. 65536" in err()
    assert L.rtlws_periodlong_geometry(16, 5, 64, 64, 0, 0, None, None, None, None) == -1 and "klo must be" in err()
    # open: the plan's rules, max_trials, the engine
    assert not L.rtlws_periodlong_open(None, 16, 5, 64, 64, 0, 0) and "klo must be" in err()
    assert not L.rtlws_periodlong_open(None, 16, 5, 64, 64, 8, 0) and err() == "rtlws_periodlong_open: max_trials must be >= 1"
    h = L.rtlws_periodlong_open(None, 16, 5, 64, 64, 8, 1)
    assert not h and err() == "rtlws_periodlong_open: null engine (no usable HIP device: there is no CPU path)"
    with pytest.raises(RuntimeError):
        built.PeriodLongPlan(None, 16, 5, 64, 64, 8)
    L.rtlws_periodlong_close(None)
    assert L.rtlws_periodlong_workspace_bytes(None) == 0

    A, B, Cc, D, E = 1 << 20, 2 << 20, 3 << 20, 4 << 20, 5 << 20          # stand-ins for device pointers: never dereferenced
    base = (("plan", None), ("din", A), ("istride", 50004), ("ntrials", 2), ("nsamp", 50000), ("best", B), ("at", Cc), ("power", D),
            ("white", E), ("st", None))

    def run(**kw):
        assert set(kw) <= {k for k, _ in base}
        return L.rtlws_periodlong_run(*[kw.get(k, v) for k, v in base]), err()

    big = 1 << 22
    for kw, word in (({"ntrials": 0}, "ntrials must be 1 .. 65536"), ({"ntrials": 65537}, "ntrials must be"), ({"nsamp": 0}, "nsamp must be 1 .. 4194304"),
                     ({"nsamp": -1}, "nsamp must be"), ({"nsamp": big + 1, "istride": big + 4}, "nsamp must be 1 .. 4194304"),
                     ({"istride": 49996}, "in_stride must be >= nsamp"), ({"istride": 0}, "in_stride must be >="),
                     ({"istride": 50002}, "in_stride must be a multiple of 4"), ({"din": None}, "null pointer"), ({"best": None}, "null pointer"),
                     ({"at": None}, "null pointer"), ({"din": A + 4}, "d_in must be 16-byte aligned"), ({"din": A + 8}, "d_in must be 16-byte"),
                     ({"best": B + 2}, "d_best must be 4-byte aligned"), ({"at": Cc + 1}, "d_at must be 4-byte aligned"),
                     ({"power": D + 2}, "d_power must be 4-byte aligned"), ({"white": E + 3}, "d_white must be 4-byte aligned"),
                     ({}, "null plan"), ({"power": None, "white": None}, "null plan"), ({"nsamp": big, "istride": big}, "null plan"),
                     ({"nsamp": 1, "istride": 4}, "null plan"), ({"istride": 1 << 40}, "null plan"), ({"ntrials": 65536}, "null plan")):
        rc, why = run(**kw)
        assert rc == -1 and word in why and why.startswith("rtlws_periodlong_run: "), (kw, why)
    # the order: a call that breaks rule i and every later rule it still can is refused for rule i
    chain = (({"ntrials": 0}, "ntrials"), ({"nsamp": 0}, "nsamp must be"), ({"istride": 2}, "in_stride must be >="), ({"istride": 50002}, "multiple of 4"),
             ({"best": None}, "null pointer"), ({"din": A + 4}, "d_in"), ({"best": B + 2}, "d_best"), ({"at": Cc + 2}, "d_at"),
             ({"power": D + 1}, "d_power"), ({"white": E + 1}, "d_white"), ({}, "null plan"))
    for i, (_, word) in enumerate(chain):
        kw = {}
        for later, _ in reversed(chain[i:]):
            kw.update(later)
        rc, why = run(**kw)
        assert rc == -1 and word in why, (i, kw, why)
    # the header's wording of the order names the same things in the same order
    txt = re.sub(r"\s+\*\s+", " ", open(os.path.join(INCLUDE, "rtlws_periodlong.h")).read())
    order = re.search(r"in this order: (ntrials.*?)0; -1 bad argument", txt, re.S).group(1)
    places = [order.index(word) for word in ("ntrials", "nsamp", "in_stride at least", "multiple of 4", "null pointers", "alignments", "null plan",
                                             "nsamp at most N")]
    assert places == sorted(places)
    assert "must be ordered" in txt                               # runs of one plan share its workspace
    # a refusal here leaves a sibling's error slot empty
    assert built.period_samples(10, 0, 1) != 0
    assert run(nsamp=0)[0] == -1 and err() != "" and built.period_last_error() == ""


def test_samples_is_the_quotient(built):
    for log2n in LOG2NS:
        for level in range(5):
            for k in (1, 2, 3, 7, 27, (1 << (log2n - 1)) - 1):
                got = built.periodlong_samples(log2n, level, k)
                assert got == float(1 << (log2n + level)) / float(k) == periodlong_ref.samples(log2n, level, k) and built.periodlong_last_error() == ""
    assert built.periodlong_samples(22, 4, 437) == float(1 << 26) / 437.0
    for args, word in (((15, 0, 1), "log2n must be 16 .. 22"), ((23, 0, 1), "log2n must be"), ((16, -1, 1), "level must be 0 .. 4"), ((16, 5, 1), "level must be"),
                       ((16, 0, 0), "k must be 1 .. N / 2 - 1"), ((16, 0, -5), "k must be"), ((16, 0, 32768), "k must be")):
        assert built.periodlong_samples(*args) == 0.0 and word in built.periodlong_last_error(), args
    # the short library keeps its own limit
    for level, k in ((0, 1), (4, 437)):
        assert built.period_samples(16, level, k) == 0.0 and "log2n must be 10 .. 15" in built.period_last_error()
    assert built.period_samples(15, 0, 3) == 32768.0 / 3.0


# ---- the yardstick's own properties ---------------------------------------------------------------------------

def test_bound_grows_and_lies_above_the_short_frames():
    bounds = [periodlong_ref.bound(l) for l in LOG2NS]
    assert bounds == sorted(bounds) and len(set(bounds)) == 7
    assert bounds[0] > period_ref.bound(15)
    # the route is period_ref.bound's: at the same t the twist's one product is all that is added
    t15 = periodlong_ref.bound(15) - period_ref.bound(15)
    tau = periodlong_ref.U * (1.0 + 3.0 * 2.0 ** 0.5)             # mu + sqrt 2 gamma_3 to first order; it enters as 2 sqrt 3 tau
    assert 2.0 * 3.0 ** 0.5 * tau < t15 < 1.001 * 2.0 * 3.0 ** 0.5 * tau
    assert bounds[-1] < 600 * periodlong_ref.U and periodlong_ref.U == period_ref.U
    print("c(log2n) in units of 2^-24: " + ", ".join("%.1f" % (b / periodlong_ref.U) for b in bounds))
    print("c(log2n): " + ", ".join("%.3g" % b for b in bounds))
    # the premise on the mean: the f64 sum's error nsamp 2^-53 mean|x| stays under u sigma up to nsamp 2^22
    assert (1 << 22) * 2.0 ** -53 * (periodlong_ref.MEAN_LIMIT + 1.0) <= periodlong_ref.U
    assert (1 << 22) * 2.0 ** -53 * (256.0 + 1.0) > periodlong_ref.U              # the short frames' premise would not do


def test_the_two_restatements_agree_where_they_meet():
    rng = np.random.default_rng(6)
    for nsamp in (1, 5, 30000, 32768):
        x = (10.0 + rng.standard_normal(nsamp)).astype(np.float32)
        assert np.array_equal(periodlong_ref.power(x, 15), period_ref.power(x, 15))
        assert periodlong_ref.nyquist_power(x, 15) == period_ref.nyquist_power(x, 15)
    n = np.arange(1 << 16)
    x = (5.0 + 2.0 * np.cos(2.0 * np.pi * 4099 * n / (1 << 16))).astype(np.float32)
    p = periodlong_ref.power(x, 16)
    assert p.shape == (32768,) and p.argmax() == 4099 and abs(p[4099] - 65536.0 ** 2) < 1e-3 * 65536.0 ** 2 and p[0] < 1e-12 * p[4099]
    assert periodlong_ref.power(x[:1], 16).max() == 0.0
    assert periodlong_ref.premises(x, 16) == (True, True)
    assert periodlong_ref.premises(x + np.float32(1000.0), 16) == (True, False)          # a mean of 700 standard deviations
    alt = np.where(n % 2 == 0, 1.0, -1.0).astype(np.float32)                              # all its power in the Nyquist bin
    assert periodlong_ref.premises(alt, 16) == (False, True)
    assert periodlong_ref.samples(16, 2, 3) == period_ref.samples(16, 2, 3)

"""CPU suite of include/rtlws_period.h (librtlws_period.so): the ABI, the kernels' resources from the code-object
metadata, the geometry, the refusals and their order, rtlws_period_samples, rtlws_period_lnq -- and the numpy
restatement's own properties (tests/period_ref.py), which hold the yardstick of tests/test_period_gpu.py rather than the
code under test.  No GPU is used."""
import math
import os
import re
import subprocess

import numpy as np
import pytest

import period_ref
from test_abi_cpu import INCLUDE, _declared_functions, _exported


def test_period_library_exports_its_header_and_nothing_else(built):
    built.period_lib()
    declared = _declared_functions("rtlws_period.h")
    assert len(declared) == 8
    assert _exported(built.PERIOD_LIB) == set(declared) == set(built.PERIOD_SYMBOLS)
    dyn = subprocess.run(["readelf", "-d", built.PERIOD_LIB], capture_output=True, text=True, check=True).stdout
    assert "librtlws_hip.so" in dyn and "$ORIGIN" in dyn
    txt = open(os.path.join(INCLUDE, "rtlws_period.h")).read()
    for name, value in (("MIN_LOG2N", 10), ("MAX_LOG2N", 15), ("MAX_LEVELS", 5), ("MIN_NORM", 16), ("MIN_SEG", 64), ("MAX_TRIALS", 65536)):
        assert re.search(r"#define RTLWS_PERIOD_%s %d\b" % (name, value), txt) and getattr(built, "PERIOD_" + name) == value
        assert getattr(period_ref, name) == value


def test_period_header_is_strict_c99(built, tmp_path):
    src = tmp_path / "uses_period.c"
    src.write_text('#include "rtlws_period.h"\nint main(void) { return rtlws_period_supported(0, 0, 0, 0, 0); }\n')
    subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Wextra", "-Werror", "-I", INCLUDE, "-fsyntax-only", str(src)], check=True)


def _kernels(built):
    """{log2n: metadata} of every kernel of the library"""
    from rtlws import codeobj
    built.period_lib()
    names = {}
    for k in codeobj.kernels(built.PERIOD_LIB):
        d = k.get("demangled", k["name"])
        m = re.search(r"rtlws::period::period_kernel<(\d+)>", d)
        assert m, d
        names[int(m.group(1))] = k
    return names


def test_period_kernels_do_not_spill(built):
    """Every kernel of the library: no scratch, no spilled register, the thread count of its frame length, no static LDS
    (the tile is the launch's: 17 M / 2 bytes, never above the 160 KiB of a compute unit), and no more registers than a
    workgroup of 1024 threads may have (128)"""
    names = _kernels(built)
    assert set(names) == set(range(10, 16))
    for log2n, k in names.items():
        assert k["vgpr_spill_count"] == 0 and k["private_segment_fixed_size"] == 0, log2n
        assert not k.get("sgpr_spill_count", 0), log2n
        assert k["max_flat_workgroup_size"] == max(64, 1 << (log2n - 5)), log2n
        assert k["group_segment_fixed_size"] == 0
        assert k["vgpr_count"] + (k.get("agpr_count") or 0) <= 128, (log2n, k["vgpr_count"], k.get("agpr_count"))
        assert period_ref.geometry(log2n, 64, 1)[2] <= 160 * 1024


def test_geometry_is_the_rule_and_the_code_objects(built):
    names = _kernels(built)
    for log2n in range(10, 16):
        m = 1 << (log2n - 1)
        for seg in (64, m):
            for norm in (16, m):
                for ntrials in (1, 257, 65536):
                    got = built.period_geometry(log2n, 5, norm, seg, 1, ntrials)
                    assert got[0] == 0 and built.period_last_error() == "", (log2n, seg, norm)
                    assert got[1:] == period_ref.geometry(log2n, seg, ntrials)
                    assert got[2] == names[log2n]["max_flat_workgroup_size"] and got[4] == m // seg
    assert built.period_geometry(15, 1, 16, 64, 1)[3] == 136 * 1024
    # any pointer may be null
    assert built.period_lib().rtlws_period_geometry(10, 1, 16, 64, 1, 1, None, None, None, None) == 0


def test_period_refusals_need_no_gpu(built):
    L = built.period_lib()
    err = built.period_last_error
    for log2n in range(10, 16):
        m = 1 << (log2n - 1)
        for levels in (1, 5):
            for norm, seg, klo in ((16, 64, 1), (m, m, m - 1), (64, 256, 8)):
                assert built.period_supported(log2n, levels, norm, seg, klo) == 1 and err() == ""

    def each(log2n=10, levels=5, norm=64, seg=64, klo=8):
        yield "rtlws_period_open", not L.rtlws_period_open(None, log2n, levels, norm, seg, klo), err()
        yield "rtlws_period", L.rtlws_period_supported(log2n, levels, norm, seg, klo) == 0, err()
        yield "rtlws_period_geometry", L.rtlws_period_geometry(log2n, levels, norm, seg, klo, 1, None, None, None, None) == -1, err()

    for kw, word in (({"log2n": 9}, "log2n must be 10 .. 15"), ({"log2n": 16}, "log2n must be"), ({"log2n": -1}, "log2n"),
                     ({"levels": 0}, "levels must be 1 .. 5"), ({"levels": 6}, "levels must be"),
                     ({"norm": 8}, "norm must be a power of two 16 .. N / 2"), ({"norm": 48}, "norm must be"), ({"norm": 1024}, "norm must be"),
                     ({"norm": 0}, "norm must be"), ({"norm": -16}, "norm must be"),
                     ({"seg": 32}, "seg must be a power of two 64 .. N / 2"), ({"seg": 96}, "seg must be"), ({"seg": 1024}, "seg must be"),
                     ({"seg": 0}, "seg must be"), ({"klo": 0}, "klo must be 1 .. N / 2 - 1"), ({"klo": 512}, "klo must be"), ({"klo": -3}, "klo must be")):
        for fn, refused, why in each(**kw):
            assert refused and word in why and why.startswith(fn + ": "), (kw, fn, why)
    # the borders that are served
    for kw in ({"norm": 512}, {"seg": 512}, {"klo": 511}, {"klo": 1}, {"log2n": 15, "norm": 16384, "seg": 16384, "klo": 16383}):
        assert L.rtlws_period_supported(*[kw.get(k, v) for k, v in (("log2n", 10), ("levels", 5), ("norm", 64), ("seg", 64), ("klo", 8))]) == 1
    # the plan's rules in order: log2n, levels, norm, seg, klo
    chain = (({"log2n": 9}, "log2n"), ({"levels": 0}, "levels"), ({"norm": 3}, "norm must be"), ({"seg": 3}, "seg must be"), ({"klo": 0}, "klo must be"))
    for i, (_, word) in enumerate(chain):
        kw = {}
        for later, _ in reversed(chain[i:]):
            kw.update(later)
        for fn, refused, why in each(**kw):
            assert refused and word in why, (i, fn, why)
    # geometry: the plan's rules, then ntrials
    for ntrials in (0, 65537, -1):
        assert L.rtlws_period_geometry(10, 5, 64, 64, 8, ntrials, None, None, None, None) == -1 and "ntrials must be 1 .. 65536" in err()
    assert L.rtlws_period_geometry(10, 5, 64, 64, 0, 0, None, None, None, None) == -1 and "klo must be" in err()
    h = L.rtlws_period_open(None, 10, 5, 64, 64, 8)
    assert not h and err() == "rtlws_period_open: null engine (no usable HIP device: there is no CPU path)"
    with pytest.raises(RuntimeError):
        built.PeriodPlan(None, 10, 5, 64, 64, 8)
    L.rtlws_period_close(None)

    A, B, Cc, D, E = 1 << 20, 2 << 20, 3 << 20, 4 << 20, 5 << 20          # stand-ins for device pointers: never dereferenced
    base = (("plan", None), ("din", A), ("istride", 604), ("ntrials", 2), ("nsamp", 600), ("best", B), ("at", Cc), ("power", D),
            ("white", E), ("st", None))

    def run(**kw):
        assert set(kw) <= {k for k, _ in base}
        return L.rtlws_period_run(*[kw.get(k, v) for k, v in base]), err()

    for kw, word in (({"ntrials": 0}, "ntrials must be 1 .. 65536"), ({"ntrials": 65537}, "ntrials must be"), ({"nsamp": 0}, "nsamp must be 1 .. 32768"),
                     ({"nsamp": -1}, "nsamp must be"), ({"nsamp": 32769, "istride": 32772}, "nsamp must be 1 .. 32768"),
                     ({"istride": 596}, "in_stride must be >= nsamp"), ({"istride": 0}, "in_stride must be >="),
                     ({"istride": 602}, "in_stride must be a multiple of 4"), ({"din": None}, "null pointer"), ({"best": None}, "null pointer"),
                     ({"at": None}, "null pointer"), ({"din": A + 4}, "d_in must be 16-byte aligned"), ({"din": A + 8}, "d_in must be 16-byte"),
                     ({"best": B + 2}, "d_best must be 4-byte aligned"), ({"at": Cc + 1}, "d_at must be 4-byte aligned"),
                     ({"power": D + 2}, "d_power must be 4-byte aligned"), ({"white": E + 3}, "d_white must be 4-byte aligned"),
                     ({}, "null plan"), ({"power": None, "white": None}, "null plan"), ({"nsamp": 32768, "istride": 32768}, "null plan"),
                     ({"nsamp": 1, "istride": 4}, "null plan"), ({"istride": 1 << 40}, "null plan")):
        rc, why = run(**kw)
        assert rc == -1 and word in why and why.startswith("rtlws_period_run: "), (kw, why)
    # the order: a call that breaks rule i and every later rule it still can is refused for rule i
    chain = (({"ntrials": 0}, "ntrials"), ({"nsamp": 0}, "nsamp must be"), ({"istride": 2}, "in_stride must be >="), ({"istride": 602}, "multiple of 4"),
             ({"best": None}, "null pointer"), ({"din": A + 4}, "d_in"), ({"best": B + 2}, "d_best"), ({"at": Cc + 2}, "d_at"),
             ({"power": D + 1}, "d_power"), ({"white": E + 1}, "d_white"), ({}, "null plan"))
    for i, (_, word) in enumerate(chain):
        kw = {}
        for later, _ in reversed(chain[i:]):
            kw.update(later)
        rc, why = run(**kw)
        assert rc == -1 and word in why, (i, kw, why)
    # the header's wording of the order names the same things in the same order
    txt = re.sub(r"\s+\*\s+", " ", open(os.path.join(INCLUDE, "rtlws_period.h")).read())
    order = re.search(r"in this order: (ntrials.*?)0; -1 bad argument", txt, re.S).group(1)
    places = [order.index(word) for word in ("ntrials", "nsamp", "in_stride at least", "multiple of 4", "null pointers", "alignments", "null plan",
                                             "nsamp at most N")]
    assert places == sorted(places)
    # a refusal here leaves a sibling's error slot empty
    assert built.fold_step(37.5) != 0
    assert run(nsamp=0)[0] == -1 and err() != "" and built.fold_last_error() == ""


def test_samples_is_the_quotient(built):
    for log2n in range(10, 16):
        for level in range(5):
            for k in (1, 2, 3, 7, 27, (1 << (log2n - 1)) - 1):
                got = built.period_samples(log2n, level, k)
                assert got == float(1 << (log2n + level)) / float(k) == period_ref.samples(log2n, level, k) and built.period_last_error() == ""
    assert built.period_samples(10, 4, 437) == 16384.0 / 437.0
    for args, word in (((9, 0, 1), "log2n must be"), ((16, 0, 1), "log2n must be"), ((10, -1, 1), "level must be 0 .. 4"), ((10, 5, 1), "level must be"),
                       ((10, 0, 0), "k must be 1 .. N / 2 - 1"), ((10, 0, -5), "k must be"), ((10, 0, 512), "k must be")):
        assert built.period_samples(*args) == 0.0 and word in built.period_last_error(), args


def test_lnq_is_the_expression(built):
    worst = 0.0
    for s in (1e-3, 1.0, 30.0, 500.0, 0.5, 7.25, 120.0):
        for h in (1, 2, 3, 8, 16):
            got, want = built.period_lnq(s, h), period_ref.lnq(s, h)
            assert math.isfinite(want) and want <= 0.0 and abs(got - want) <= 1e-12 * abs(want), (s, h, got, want)
            worst = max(worst, abs(got - want) / abs(want) if want else 0.0)
            if s <= 30.0:                                        # where the plain expression neither under- nor overflows
                plain = math.log(math.exp(-s) * sum(s ** j / math.factorial(j) for j in range(h)))
                assert abs(want - plain) <= 1e-9 * abs(plain) + 1e-15, (s, h, want, plain)
    print("rtlws_period_lnq: at most %.3g relative from the Python expression" % worst)
    for h in (1, 2, 16):
        assert built.period_lnq(0.0, h) == 0.0 and built.period_lnq(-3.0, h) == 0.0 and period_ref.lnq(0.0, h) == 0.0
    assert built.period_lnq(1e-3, 1) == -1e-3 and built.period_lnq(500.0, 1) == -500.0
    assert -500.0 < built.period_lnq(500.0, 16) < -400.0                     # e^-500 alone underflows nothing here
    for s, h in ((1.0, 0), (1.0, 17), (1.0, -1), (float("nan"), 4), (float("inf"), 4), (float("-inf"), 4)):
        assert math.isnan(built.period_lnq(s, h)) and math.isnan(period_ref.lnq(s, h)), (s, h)
    # more harmonics of the same sum are less surprising
    assert built.period_lnq(30.0, 1) < built.period_lnq(30.0, 2) < built.period_lnq(30.0, 16) < 0.0


# ---- the yardstick's own properties ---------------------------------------------------------------------------

def _signed_rows(m, seed):
    rng = np.random.default_rng(seed)
    return (rng.uniform(1.0, 2.0, m) * np.exp2(rng.integers(-6, 7, m))).astype(np.float32)


def test_sums_are_the_closed_form_on_integers():
    """on integer-valued W every partial sum is exact in f32: S_l[k] = sum_{h=1..H} W[floor(k h / H + 1/2)]"""
    rng = np.random.default_rng(1)
    m = 2048
    w = rng.integers(0, 1000, m).astype(np.float32)
    s = period_ref.sums(w, 5)
    assert s.shape == (5, m) and s.dtype == np.float32
    k = np.arange(m)
    for l in range(5):
        big = 1 << l
        want = sum(w.astype(np.int64)[(2 * k * h + big) // (2 * big)] for h in range(1, big + 1))
        assert np.array_equal(s[l].astype(np.int64), want), l
        assert all(((k * h + big // 2) >> l).max() <= m - 1 for h in range(1, big + 1))
    # the identity behind it: the even harmonics of level l are level l - 1's terms
    for l in range(1, 5):
        for h in range(2, (1 << l) + 1, 2):
            assert np.array_equal((2 * k * h + (1 << l)) // (2 << l), (2 * k * (h // 2) + (1 << (l - 1))) // (1 << l))


def test_the_order_is_not_idle():
    """on rows with exponents over 2^-6 .. 2^6 the reversed odd-harmonic order and the other balanced tree change bits: a
    kernel that reorders is caught"""
    w = _signed_rows(2048, 2)
    a, b = period_ref.sums(w, 5), period_ref.sums(w, 5, descending=True)
    differ = [int((a[l].view(np.uint32) != b[l].view(np.uint32)).sum()) for l in range(5)]
    assert differ[0] == differ[1] == 0 and min(differ[2:]) >= 100, differ
    assert np.allclose(a, b, rtol=1e-5)
    p = _signed_rows(4096, 3)
    differ_tree = {}
    for norm in (16, 64, 4096):
        t1, t2 = period_ref.tree_sums(p, norm), period_ref.tree_sums(p, norm, pairs_first=False)
        differ_tree[norm] = int((t1.view(np.uint32) != t2.view(np.uint32)).sum())
        assert np.allclose(t1, t2, rtol=1e-5)
        w1, w2 = period_ref.whiten(p, norm), period_ref.whiten(p, norm, pairs_first=False)
        assert (differ_tree[norm] > 0) == bool((w1.view(np.uint32) != w2.view(np.uint32)).any())
    print("reversed harmonics differ in %s bins per level; halves-first trees differ in %s blocks" % (differ, differ_tree))
    assert differ_tree[16] >= 20 and differ_tree[64] >= 10
    # the tree by the letter on one block
    blk = p[:16]
    s = [np.float32(v) for v in blk]
    while len(s) > 1:
        s = [np.float32(s[2 * i] + s[2 * i + 1]) for i in range(len(s) // 2)]
    assert period_ref.tree_sums(p, 16)[0].view(np.uint32) == s[0].view(np.uint32)
    mean = np.float32(s[0] * np.float32(1.0 / 16.0))
    assert np.array_equal(period_ref.whiten(p, 16)[:16].view(np.uint32), (blk / mean).astype(np.float32).view(np.uint32))


def _peaks_loop(s, seg, klo):
    levels, m = s.shape
    best = np.full((levels, m // seg), -np.inf, np.float32)
    at = np.full((levels, m // seg), -1, np.int32)
    for l in range(levels):
        for k in range(klo, m):
            if s[l, k] > best[l, k // seg]:
                best[l, k // seg], at[l, k // seg] = s[l, k], k
    return best, at


def test_peaks_are_the_plain_loop():
    rng = np.random.default_rng(4)
    m, seg = 512, 64
    s = rng.integers(0, 50, (3, m)).astype(np.float32)            # many ties
    s[0, 70], s[0, 100] = 99.0, 99.0                            # equal maxima in one segment
    s[1, 128], s[1, 191] = 77.0, 77.0                           # at the first and the last k of a segment
    s[2, 200:210] = np.nan                                      # NaNs inside a segment
    s[2, 256:320] = np.nan                                      # a segment of NaN alone
    s[0, 330], s[1, 340], s[1, 384:448] = np.inf, -np.inf, -np.inf
    for klo in (1, 63, 64, 100, 101, 511):
        best, at = period_ref.peaks(s, seg, klo)
        want_best, want_at = _peaks_loop(s, seg, klo)
        assert np.array_equal(best.view(np.uint32), want_best.view(np.uint32)) and np.array_equal(at, want_at), klo
        assert best.dtype == np.float32 and at.dtype == np.int32
    best, at = period_ref.peaks(s, seg, 1)
    assert at[0, 1] == 70 and at[1, 2] == 128 and at[2, 4] == -1 and np.isneginf(best[2, 4]) and at[1, 6] == -1 and best[0, 5] == np.inf
    best, at = period_ref.peaks(s, seg, 101)                     # a segment cut by klo, one wholly below it
    assert at[0, 0] == -1 and np.isneginf(best[0, 0]) and at[0, 1] >= 101 and best[0, 1] < 99.0
    assert period_ref.peaks(s, seg, 100)[1][0, 1] == 100


def test_whiten_zero_block_is_nan():
    p = _signed_rows(256, 5)
    p[64:128] = 0.0
    w = period_ref.whiten(p, 64)
    assert np.isnan(w[64:128]).all() and np.isfinite(w[:64]).all() and np.isfinite(w[128:]).all()
    best, at = period_ref.peaks(period_ref.sums(w, 1), 64, 1)
    assert at[0, 1] == -1 and np.isneginf(best[0, 1])
    assert abs(float(w[:64].astype(np.float64).mean()) - 1.0) < 1e-6


def test_power_and_bound():
    """power() is the mean-removed, padded rfft; an exact-bin tone lands in its bin; bound() grows with log2n and stays
    a small multiple of the f32 unit roundoff per stage"""
    n = np.arange(1024)
    x = (5.0 + 2.0 * np.cos(2.0 * np.pi * 37 * n / 1024)).astype(np.float32)
    p = period_ref.power(x, 10)
    assert p.shape == (512,) and p.argmax() == 37 and abs(p[37] - 1024.0 ** 2) < 1e-3 * 1024.0 ** 2 and p[0] < 1e-12 * p[37]
    assert period_ref.power(x[:1], 10).max() == 0.0
    bounds = [period_ref.bound(l) for l in range(10, 16)]
    assert bounds == sorted(bounds) and 100 * period_ref.U < bounds[0] and bounds[-1] < 400 * period_ref.U
    print("c(log2n) in units of 2^-24: " + ", ".join("%.1f" % (b / period_ref.U) for b in bounds))

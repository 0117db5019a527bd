"""CPU suite of include/rtlws_accel.h (librtlws_accel.so): the ABI, the kernels' resources from the code-object metadata,
the geometry, the refusals and their order, the index map against Python's integers (ties among them) and its range
properties, and the two coefficient helpers against fractions.Fraction -- and the numpy restatement (tests/accel_ref.py)
against the same integers, which holds the yardstick of tests/test_accel_gpu.py rather than the code under test.  No GPU
is used."""
import os
import re
import subprocess
from fractions import Fraction

import numpy as np
import pytest

import accel_ref
import periodlong_ref
from test_abi_cpu import INCLUDE, _declared_functions, _exported

TOP = 1 << 40
BIG = 1 << 22


def _seeded_coefs(seed, count):
    rng = np.random.default_rng(seed)
    return [int(c) for c in rng.integers(-TOP, TOP + 1, count)]


def test_accel_library_exports_its_header_and_nothing_else(built):
    built.accel_lib()
    declared = _declared_functions("rtlws_accel.h")
    assert len(declared) == 11
    assert _exported(built.ACCEL_LIB) == set(declared) == set(built.ACCEL_SYMBOLS)
    dyn = subprocess.run(["readelf", "-d", built.ACCEL_LIB], capture_output=True, text=True, check=True).stdout
    assert "librtlws_hip.so" in dyn and "$ORIGIN" in dyn and "librtlws_periodlong.so" not in dyn
    txt = open(os.path.join(INCLUDE, "rtlws_accel.h")).read()
    for name, value in (("MAX_NACCEL", 1024), ("MAX_VIRTUAL", 65536), ("STAGES", 6)):
        assert re.search(r"#define RTLWS_ACCEL_%s %d\b" % (name, value), txt) and getattr(built, "ACCEL_" + name) == value
        assert getattr(accel_ref, name) == value
    assert re.search(r"#define RTLWS_ACCEL_MAX_COEF \(\(int64_t\)1 << 40\)", txt) and built.ACCEL_MAX_COEF == accel_ref.MAX_COEF == TOP
    # the long-frame library is as it was
    assert len(_declared_functions("rtlws_periodlong.h")) == 8 and _exported(built.PERIODLONG_LIB) == set(built.PERIODLONG_SYMBOLS)


def test_accel_header_is_strict_c99(built, tmp_path):
    src = tmp_path / "uses_accel.c"
    src.write_text('#include "rtlws_accel.h"\nint main(void) { int64_t c = RTLWS_ACCEL_MAX_COEF; return rtlws_accel_supported(0, 0, 0, 0, 0, 1, &c) + '
                   '(int)rtlws_accel_workspace_bytes(0) + (int)rtlws_accel_shift(c, 2, 1); }\n')
    subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Wextra", "-Werror", "-I", INCLUDE, "-fsyntax-only", str(src)], check=True)


def _kernels(built):
    """{demangled name up to its arguments: metadata} of every kernel of the library"""
    from rtlws import codeobj
    built.accel_lib()
    names = {}
    for k in codeobj.kernels(built.ACCEL_LIB):
        d = k.get("demangled", k["name"])
        m = re.search(r"rtlws::(accel|periodlong)::(\w+)_kernel(?:<(\d+)>)?", d)
        assert m, d
        names[(m.group(1), m.group(2), int(m.group(3)) if m.group(3) else None)] = k
    return names


def _stage_kernels(log2n):
    l1, l2 = periodlong_ref.split(log2n)
    return (("accel", "mapped_mean", None), ("accel", "mapped_cols16" if l1 == 4 else "mapped_cols256", None), ("periodlong", "rows", l2),
            ("periodlong", "untangle", l1), ("periodlong", "whiten", None), ("periodlong", "peaks", None))


def test_accel_kernels_do_not_spill(built):
    """test_periodlong_kernels_do_not_spill's rule for every kernel of this library: no scratch, no spilled register, the
    thread count the geometry names, static plus dynamic LDS within the 160 KiB of a compute unit, and no more registers
    than its workgroup may have"""
    names = _kernels(built)
    own = {k for k in names if k[0] == "accel"}
    assert own == {("accel", "mapped_mean", None), ("accel", "mapped_cols16", None), ("accel", "mapped_cols256", None), ("accel", "resample", None)}
    # the stages behind the columns are the long-frame library's object: its eleven kernels by name
    assert {k[1:] for k in names if k[0] == "periodlong"} == {("mean", None), ("cols16", None), ("cols256", None), ("rows", 11), ("rows", 12),
                                                               ("rows", 13), ("rows", 14), ("untangle", 4), ("untangle", 8), ("whiten", None),
                                                               ("peaks", None)}
    for key, k in names.items():
        assert k["vgpr_spill_count"] == 0 and k["private_segment_fixed_size"] == 0, key
        assert not k.get("sgpr_spill_count", 0), key
    seen = set()
    coefs = [0]
    for log2n in range(16, 23):
        rc, _, threads, lds, _ = built.accel_geometry(log2n, 5, 64, 64, 1, coefs)
        assert rc == 0
        for stage, key in enumerate(_stage_kernels(log2n)):
            k = names[key]
            seen.add(key)
            assert k["max_flat_workgroup_size"] == threads[stage], (log2n, key)
            allowed = min(512, 512 * 256 // threads[stage])
            assert k["vgpr_count"] + (k.get("agpr_count") or 0) <= allowed, (log2n, key, k["vgpr_count"], k.get("agpr_count"))
            static = k["group_segment_fixed_size"]
            assert static in (0, lds[stage]) and max(static, lds[stage]) <= 160 * 1024, (log2n, key, static, lds[stage])
    assert own - seen == {("accel", "resample", None)}
    k = names[("accel", "resample", None)]
    assert k["max_flat_workgroup_size"] == 256 and k["group_segment_fixed_size"] == 0 and k["vgpr_count"] + (k.get("agpr_count") or 0) <= 512


def test_geometry_is_the_rule(built):
    for log2n in (16, 19, 20, 22):
        for coefs in ([0], [TOP, -TOP, 5]):
            naccel = len(coefs)
            for ntrials in (1, 3, 65536 // naccel):
                for seg in (64, 16384):
                    got = built.accel_geometry(log2n, 5, 64, seg, 1, coefs, ntrials)
                    assert got[0] == 0 and built.accel_last_error() == "", (log2n, naccel, ntrials)
                    assert got[1:] == accel_ref.geometry(log2n, seg, ntrials, naccel), (log2n, got)
                    # the stages of rtlws_periodlong.h over as many plain trials
                    assert got == built.periodlong_geometry(log2n, 5, 64, seg, 1, ntrials * naccel)
    assert built.accel_lib().rtlws_accel_geometry(16, 1, 16, 64, 1, 1, np.zeros(1, np.int64).ctypes.data_as(built._i64p), 1, None, None, None, None) == 0


def test_accel_refusals_need_no_gpu(built):
    L = built.accel_lib()
    err = built.accel_last_error
    ok = np.array([0, 1, -1, TOP, -TOP], np.int64)
    ptr = lambda a: None if a is None else a.ctypes.data_as(built._i64p)
    for log2n in range(16, 23):
        m = 1 << (log2n - 1)
        for norm, seg, klo in ((16, 64, 1), (16384, 16384, m - 1)):
            assert L.rtlws_accel_supported(log2n, 5, norm, seg, klo, ok.size, ptr(ok)) == 1 and err() == ""
    assert built.accel_supported(16, 5, 64, 64, 8, np.zeros(1024, np.int64)) == 1

    def each(log2n=16, levels=5, norm=64, seg=64, klo=8, naccel=ok.size, coefs=ok):
        yield "rtlws_accel_open", not L.rtlws_accel_open(None, log2n, levels, norm, seg, klo, naccel, ptr(coefs), 1), err()
        yield "rtlws_accel", L.rtlws_accel_supported(log2n, levels, norm, seg, klo, naccel, ptr(coefs)) == 0, err()
        yield "rtlws_accel_geometry", L.rtlws_accel_geometry(log2n, levels, norm, seg, klo, naccel, ptr(coefs), 1, None, None, None, None) == -1, err()

    over = lambda c: np.array([0, 3, c], np.int64)
    for kw, word in (({"log2n": 15}, "log2n must be 16 .. 22"), ({"log2n": 23}, "log2n must be"), ({"levels": 0}, "levels must be 1 .. 5"),
                     ({"levels": 6}, "levels must be"), ({"norm": 8}, "norm must be a power of two 16 .. 16384"), ({"norm": 48}, "norm must be"),
                     ({"seg": 32}, "seg must be a power of two 64 .. 16384"), ({"seg": 32768}, "seg must be"), ({"klo": 0}, "klo must be 1 .. N / 2 - 1"),
                     ({"klo": 32768}, "klo must be"), ({"naccel": 0}, "naccel must be 1 .. 1024"), ({"naccel": 1025}, "naccel must be"),
                     ({"naccel": -1}, "naccel must be"), ({"coefs": None}, "null table of coefficients"),
                     ({"naccel": 3, "coefs": over(TOP + 1)}, "every coefficient must be -2^40 .. 2^40"),
                     ({"naccel": 3, "coefs": over(-TOP - 1)}, "every coefficient must be"),
                     ({"naccel": 3, "coefs": over(-(1 << 63))}, "every coefficient must be")):
        for fn, refused, why in each(**kw):
            assert refused and word in why and why.startswith(fn + ": "), (kw, fn, why)
    # an entry behind naccel is not looked at
    assert L.rtlws_accel_supported(16, 5, 64, 64, 8, 2, ptr(over(TOP + 1))) == 1
    # the rules in order: periodlong's five, naccel, the table, its entries
    chain = (({"log2n": 15}, "log2n"), ({"levels": 0}, "levels"), ({"norm": 3}, "norm must be"), ({"seg": 3}, "seg must be"), ({"klo": 0}, "klo must be"),
             ({"naccel": 0}, "naccel must be"), ({"coefs": None}, "null table"))
    for i, (_, word) in enumerate(chain):
        kw = {}
        for later, _ in reversed(chain[i:]):
            kw.update(later)
        for fn, refused, why in each(**kw):
            assert refused and word in why, (i, fn, why)
    for fn, refused, why in each(naccel=1025, coefs=over(TOP + 1)):
        assert refused and "naccel must be" in why
    # geometry: the plan's rules, then ntrials and the product
    geo = lambda naccel, ntrials: L.rtlws_accel_geometry(16, 5, 64, 64, 8, naccel, ptr(np.zeros(naccel, np.int64)), ntrials, None, None, None, None)
    for ntrials in (0, 65537, -1):
        assert geo(1, ntrials) == -1 and "ntrials must be 1 .. 65536" in err()
    assert geo(1, 65536) == 0 and geo(3, 21845) == 0 and geo(1024, 64) == 0
    for naccel, ntrials in ((3, 21846), (2, 32769), (1024, 65)):
        assert geo(naccel, ntrials) == -1 and "ntrials * naccel must be at most 65536" in err()
    assert L.rtlws_accel_geometry(16, 5, 64, 64, 8, 0, None, 0, None, None, None, None) == -1 and "naccel must be" in err()
    # open: the plan's rules, max_trials, the engine
    assert not L.rtlws_accel_open(None, 16, 5, 64, 64, 8, 1, None, 0) and "null table" in err()
    assert not L.rtlws_accel_open(None, 16, 5, 64, 64, 8, ok.size, ptr(ok), 0) and err() == "rtlws_accel_open: max_trials must be >= 1"
    assert not L.rtlws_accel_open(None, 16, 5, 64, 64, 8, ok.size, ptr(ok), 1)
    assert err() == "rtlws_accel_open: null engine (no usable HIP device: there is no CPU path)"
    with pytest.raises(RuntimeError):
        built.AccelPlan(None, 16, 5, 64, 64, 8, ok)
    L.rtlws_accel_close(None)
    assert L.rtlws_accel_workspace_bytes(None) == 0

    A, B, Cc, D, E = 1 << 20, 2 << 20, 3 << 20, 4 << 20, 5 << 20          # stand-ins for device pointers: never dereferenced
    base = (("plan", None), ("din", A), ("istride", 50004), ("ntrials", 2), ("nsamp", 50000), ("best", B), ("at", Cc), ("power", D),
            ("white", E), ("st", None))

    def search(**kw):
        assert set(kw) <= {k for k, _ in base}
        return L.rtlws_accel_search(*[kw.get(k, v) for k, v in base]), err()

    for kw, word in (({"ntrials": 0}, "ntrials must be 1 .. 65536"), ({"ntrials": 65537}, "ntrials must be"), ({"nsamp": 0}, "nsamp must be 1 .. 4194304"),
                     ({"nsamp": BIG + 1, "istride": BIG + 4}, "nsamp must be 1 .. 4194304"), ({"istride": 49996}, "in_stride must be >= nsamp"),
                     ({"istride": 50002}, "in_stride must be a multiple of 4"), ({"din": None}, "null pointer"), ({"best": None}, "null pointer"),
                     ({"at": None}, "null pointer"), ({"din": A + 4}, "d_in must be 16-byte aligned"), ({"best": B + 2}, "d_best must be 4-byte aligned"),
                     ({"at": Cc + 1}, "d_at must be 4-byte aligned"), ({"power": D + 2}, "d_power must be 4-byte aligned"),
                     ({"white": E + 3}, "d_white must be 4-byte aligned"), ({}, "null plan"), ({"power": None, "white": None}, "null plan"),
                     ({"nsamp": BIG, "istride": BIG}, "null plan"), ({"ntrials": 65536}, "null plan")):
        rc, why = search(**kw)
        assert rc == -1 and word in why and why.startswith("rtlws_accel_search: "), (kw, why)
    chain = (({"ntrials": 0}, "ntrials"), ({"nsamp": 0}, "nsamp must be"), ({"istride": 2}, "in_stride must be >="), ({"istride": 50002}, "multiple of 4"),
             ({"best": None}, "null pointer"), ({"din": A + 4}, "d_in"), ({"best": B + 2}, "d_best"), ({"at": Cc + 2}, "d_at"),
             ({"power": D + 1}, "d_power"), ({"white": E + 1}, "d_white"), ({}, "null plan"))
    for i, (_, word) in enumerate(chain):
        kw = {}
        for later, _ in reversed(chain[i:]):
            kw.update(later)
        rc, why = search(**kw)
        assert rc == -1 and word in why, (i, kw, why)

    rbase = (("plan", None), ("din", A), ("istride", 50004), ("ntrials", 2), ("nsamp", 50000), ("first", 0), ("count", 1), ("dout", B),
             ("ostride", 50000), ("st", None))

    def resample(**kw):
        assert set(kw) <= {k for k, _ in rbase}
        return L.rtlws_accel_resample(*[kw.get(k, v) for k, v in rbase]), err()

    for kw, word in (({"ntrials": 0}, "ntrials must be 1 .. 65536"), ({"ntrials": 65537}, "ntrials must be"), ({"nsamp": 0}, "nsamp must be 1 .. 4194304"),
                     ({"istride": 49996}, "in_stride must be >= nsamp"), ({"istride": 50002}, "in_stride must be a multiple of 4"),
                     ({"ostride": 49996}, "out_stride must be >= nsamp"), ({"ostride": 0}, "out_stride must be >="),
                     ({"ostride": 50002}, "out_stride must be a multiple of 4"), ({"count": 0}, "a_count must be >= 1"), ({"count": -2}, "a_count must be"),
                     ({"first": -1}, "a_first must be >= 0"), ({"first": 1024}, "a_first + a_count must be at most naccel"),
                     ({"first": 1000, "count": 25}, "a_first + a_count must be at most naccel"), ({"first": (1 << 31) - 1, "count": (1 << 31) - 1}, "a_first + a_count"),
                     ({"din": None}, "null pointer"), ({"dout": None}, "null pointer"), ({"din": A + 4}, "d_in must be 16-byte aligned"),
                     ({"dout": B + 4}, "d_out must be 16-byte aligned"), ({"dout": B + 8}, "d_out must be 16-byte"), ({}, "null plan"),
                     ({"first": 1023}, "null plan"), ({"first": 0, "count": 1024}, "null plan"), ({"ostride": 1 << 40}, "null plan")):
        rc, why = resample(**kw)
        assert rc == -1 and word in why and why.startswith("rtlws_accel_resample: "), (kw, why)
    chain = (({"ntrials": 0}, "ntrials"), ({"nsamp": 0}, "nsamp must be"), ({"istride": 2}, "in_stride must be >="), ({"istride": 50002}, "in_stride must be a multiple"),
             ({"ostride": 2}, "out_stride must be >="), ({"ostride": 50002}, "out_stride must be a multiple"), ({"count": 0}, "a_count"),
             ({"first": -1}, "a_first must be"), ({"dout": None}, "null pointer"), ({"din": A + 4}, "d_in"), ({"dout": B + 4}, "d_out"), ({}, "null plan"))
    for i, (_, word) in enumerate(chain):
        kw = {}
        for later, _ in reversed(chain[i:]):
            kw.update(later)
        rc, why = resample(**kw)
        assert rc == -1 and word in why, (i, kw, why)
    # the header's wording of the two orders names the same things in the same order
    txt = re.sub(r"\s+\*\s+", " ", open(os.path.join(INCLUDE, "rtlws_accel.h")).read())
    orders = re.findall(r"in this order: (ntrials.*?)0; -1 bad argument", txt, re.S)
    assert len(orders) == 2
    for order, words in zip(orders, (("ntrials", "nsamp", "in_stride at least", "multiple of 4", "null pointers", "alignments", "null plan",
                                      "naccel at most 65536", "nsamp at most N"),
                                     ("ntrials", "nsamp", "in_stride at least", "out_stride at least", "a_count at least 1", "a_first at least 0",
                                      "at most 1024", "null pointers", "alignments", "null plan", "at most naccel", "a_count at most 65536",
                                      "nsamp at most N"))):
        places = [order.index(word) for word in words]
        assert places == sorted(places), order
    assert "must be ordered" in txt
    # a refusal here leaves a sibling's error slot empty
    assert built.periodlong_samples(16, 0, 1) != 0
    assert search(nsamp=0)[0] == -1 and err() != "" and built.periodlong_last_error() == ""


SHIFT_NSAMPS = (1, 2, 5, 60000, BIG)


def test_shift_is_the_definition(built):
    """rtlws_accel_shift and accel_ref.shift against Python's integers: c = 0, +-1, +-2^40 and seeded c; nsamp 1, 2, 5,
    60 000 and 2^22; and arguments where c n (L - n) is an exact odd multiple of 2^63, found by a search, both signs: the
    tie goes up both times"""
    coefs = [0, 1, -1, TOP, -TOP] + _seeded_coefs(11, 6)
    rng = np.random.default_rng(12)
    for nsamp in SHIFT_NSAMPS:
        ns = sorted(set([0, nsamp - 1, nsamp // 2, (nsamp - 1) // 2] + [int(n) for n in rng.integers(0, nsamp, 40)]))
        for c in coefs:
            want = [accel_ref.shift_exact(c, nsamp, n) for n in ns]
            assert [built.accel_shift(c, nsamp, n) for n in ns] == want and built.accel_last_error() == "", (c, nsamp)
            ref = accel_ref.shift(c, nsamp)
            assert ref.dtype == np.int64 and ref.shape == (nsamp,) and [int(ref[n]) for n in ns] == want, (c, nsamp)
    # the restatement over every n of the shorter series
    for nsamp in (1, 2, 5, 60000):
        for c in coefs:
            assert accel_ref.shift(c, nsamp).tolist() == [accel_ref.shift_exact(c, nsamp, n) for n in range(nsamp)], (c, nsamp)
    # the mid-frame shift the header names
    assert built.accel_shift(TOP, BIG, BIG // 2) == 262144 and built.accel_shift(-TOP, BIG, BIG // 2) == -262144
    # exact ties: the search finds them at series lengths whose last index is 4 or 8 times an odd number
    found = 0
    for nsamp in (BIG - 3, BIG - 7, 65281, 65025):
        pairs = accel_ref.ties(nsamp)
        assert pairs, nsamp
        for c, n in pairs:
            prod = c * n * (nsamp - 1 - n)
            assert prod % (1 << 64) == 1 << 63                              # an odd multiple of 2^63
            up, down = (prod + (1 << 63)) >> 64, (-prod + (1 << 63)) >> 64
            assert up + down == 1                                           # x.5 -> x + 1 and -x.5 -> -x: both up
            assert built.accel_shift(c, nsamp, n) == up == accel_ref.shift_exact(c, nsamp, n) == int(accel_ref.shift(c, nsamp)[n])
            assert built.accel_shift(-c, nsamp, n) == down == accel_ref.shift_exact(-c, nsamp, n) == int(accel_ref.shift(-c, nsamp)[n])
            found += 1
    assert found >= 4
    for args, word in (((TOP + 1, 5, 0), "the coefficient must be -2^40 .. 2^40"), ((-TOP - 1, 5, 0), "the coefficient must be"),
                       ((1, 0, 0), "nsamp must be 1 .. 4194304"), ((1, BIG + 1, 0), "nsamp must be"), ((1, 5, -1), "n must be 0 .. nsamp - 1"),
                       ((1, 5, 5), "n must be")):
        assert built.accel_shift(*args) == 0 and word in built.accel_last_error(), args


@pytest.mark.parametrize("nsamp", [BIG, 65536])
def test_the_map_stays_inside_the_series(built, nsamp):
    """f_c has fixed ends, does not decrease and stays in 0 .. nsamp - 1 at c = +-2^40; the library's shift at the ends,
    the middle and seeded n agrees with the restatement that the properties are shown on"""
    rng = np.random.default_rng(nsamp)
    for c in (TOP, -TOP):
        f = accel_ref.index(c, nsamp)                    # asserts the properties
        assert f[0] == 0 and f[-1] == nsamp - 1 and f.min() == 0 and f.max() == nsamp - 1 and np.diff(f).min() >= 0
        assert np.diff(f).max() <= 2
        mid = int(f[nsamp // 2]) - nsamp // 2
        assert abs(mid) == (262144 if nsamp == BIG else 64) and (mid > 0) == (c > 0)
        for n in [0, 1, nsamp // 2, nsamp - 2, nsamp - 1] + [int(v) for v in rng.integers(0, nsamp, 200)]:
            assert n + built.accel_shift(c, nsamp, n) == f[n]


def test_the_coefficients_are_the_nearest_integers(built):
    err = built.accel_last_error
    rng = np.random.default_rng(5)
    cases = [(500.0, 64e-6), (-500.0, 64e-6), (0.0, 64e-6), (3.7, 1e-3), (1e-300, 1e-300), (5e-324, 1.0), (-0.1, 0.1), (1.0, 1.0), (17.5, 1.0 / 3.0)]
    cases += [(float(a), float(t)) for a, t in zip(rng.normal(0.0, 800.0, 40), rng.uniform(1e-6, 1e-4, 40))]
    for a, t in cases:
        want = accel_ref.coef(a, t)
        assert want is not None
        assert built.accel_coef(a, t) == want and err() == "", (a, t)
    assert built.accel_coef(500.0, 64e-6) == accel_ref._nearest(Fraction(500.0) * Fraction(64e-6) * 2 ** 64 / (2 * 299792458)) > 0
    # the largest served and the first refused: c = 2^40 exactly needs accel tsamp = 2^40 2 c_light / 2^64
    edge = 2.0 ** -24 * 2 * 299792458
    assert built.accel_coef(edge, 1.0) == TOP and built.accel_coef(-edge, 1.0) == -TOP and err() == ""
    for a, t in ((np.nextafter(edge, np.inf) * 1.0000001, 1.0), (1e6, 1.0), (-1e6, 1.0), (1e300, 1e300), (np.inf, 1.0), (1.0, -np.inf), (np.nan, 1.0), (1.0, np.nan)):
        assert accel_ref.coef(a, t) is None if np.isfinite(a) and np.isfinite(t) else True
        assert built.accel_coef(a, t) == 0 and err().startswith("rtlws_accel_coef: "), (a, t)
    shifts = [10.0, -10.0, 0.0, 0.5, 1e-9, 53.0, -53.25, 1.0 / 3.0]
    for nsamp in (2, 5, 60000, 65536, BIG):
        top = (nsamp - 1) ** 2 / 4.0 * 2.0 ** -24            # the mid-frame shift of 2^40
        for s in shifts + [top, -top, float(np.nextafter(top, 0.0))] + [float(v) for v in rng.uniform(-top, top, 10)]:
            want = accel_ref.coef_from_shift(s, nsamp)
            if want is None:
                assert built.accel_coef_from_shift(s, nsamp) == 0 and "beyond" in err(), (s, nsamp)
            else:
                assert built.accel_coef_from_shift(s, nsamp) == want and err() == "", (s, nsamp)
                # the coefficient's own mid-frame shift is the one asked for, to the rounding of the map
                if nsamp % 2 == 1:
                    assert abs(accel_ref.shift_exact(want, nsamp, (nsamp - 1) // 2) - s) <= 0.5 + 1e-6 * abs(s) + (nsamp - 1) ** 2 * 2.0 ** -67
    assert built.accel_coef_from_shift(10.0, 60000) == 204970655339
    for s, nsamp, word in ((1.0, 1, "nsamp must be 2 .. 4194304"), (1.0, 0, "nsamp must be"), (1.0, BIG + 1, "nsamp must be"), (np.inf, 5, "finite"),
                           (np.nan, 5, "finite"), (1e9, 60000, "beyond"), (-1e9, 60000, "beyond"), (1e300, 2, "beyond")):
        assert built.accel_coef_from_shift(s, nsamp) == 0 and word in err(), (s, nsamp)
    # the scene's table: a step of 10 samples at mid-frame of 60 000; the library serves five steps and refuses six
    step = built.accel_coef_from_shift(10.0, 60000)
    assert 5 * step <= TOP < 6 * step

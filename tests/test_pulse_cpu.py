"""CPU suite of include/rtlws_pulse.h (librtlws_pulse.so): the ABI, the kernel's resources from the code-object
metadata, the tile and the LDS a table gets, the refusals and their order, rtlws_pulse_snr -- and the numpy
restatement's own properties (tests/pulse_ref.py), which hold the yardstick of tests/test_pulse_gpu.py rather than the
code under test.  No GPU is used."""
import math
import os
import re
import subprocess

import numpy as np
import pytest

import pulse_ref
from pulse_ref import LADDER, MIXED16
from test_abi_cpu import INCLUDE, _declared_functions, _exported

BOUND_WIDTHS = tuple(range(1, 65)) + (100, 255, 256, 257, 511, 512, 513, 1000, 1023, 1024)


def _i32(widths):
    return np.ascontiguousarray(widths, dtype=np.int32)


def test_pulse_library_exports_its_header_and_nothing_else(built):
    built.pulse_lib()
    declared = _declared_functions("rtlws_pulse.h")
    assert len(declared) == 9
    assert _exported(built.PULSE_LIB) == set(declared) == set(built.PULSE_SYMBOLS)
    dyn = subprocess.run(["readelf", "-d", built.PULSE_LIB], capture_output=True, text=True, check=True).stdout
    assert "librtlws_hip.so" in dyn and "$ORIGIN" in dyn
    txt = open(os.path.join(INCLUDE, "rtlws_pulse.h")).read()
    for name, value in (("MAX_WIDTHS", 16), ("MAX_WIDTH", 1024), ("MIN_SEG", 64), ("MAX_SEG", 1048576), ("MAX_TRIALS", 65536),
                        ("MAX_NOUT", 1 << 30)):
        assert re.search(r"#define RTLWS_PULSE_%s %d\b" % (name, value), txt) and getattr(built, "PULSE_" + name) == value
        assert getattr(pulse_ref, name) == value


def _kernels(built):
    """{(f32 words of LDS, outputs of a tile per thread): metadata} of every kernel of the library"""
    from rtlws import codeobj
    built.pulse_lib()
    names = {}
    for k in codeobj.kernels(built.PULSE_LIB):
        d = k.get("demangled", k["name"])
        m = re.search(r"rtlws::pulse::pulse_kernel<(\d+), (\d+)>", d)
        assert m, d
        names[(int(m.group(1)), int(m.group(2)))] = k
    return names


def test_pulse_kernels_do_not_spill(built):
    """Every kernel of the library: no scratch, no spilled register, 256 threads, its static LDS the size its name says,
    and no more registers than five workgroups a compute unit can have (96); the kernel names are exactly the
    instantiations the launch table reaches: the 1024 tile in every LDS, the smaller tiles in the largest."""
    names = _kernels(built)
    assert set(names) == {(words, 4) for words in pulse_ref.LDS_WORDS} | {(16384, 2), (16384, 1)}
    for key, k in names.items():
        assert k["vgpr_spill_count"] == 0 and k["private_segment_fixed_size"] == 0, key
        assert not k.get("sgpr_spill_count", 0), key
        assert k["max_flat_workgroup_size"] == 256
        assert k["group_segment_fixed_size"] == 4 * key[0] <= 65536
        assert k["vgpr_count"] + (k.get("agpr_count") or 0) <= 96, (key, k["vgpr_count"], k.get("agpr_count"))


def test_geometry_reports_the_code_objects_resources(built):
    """rtlws_pulse_geometry's LDS for a table of every size class is the static LDS of a kernel of the library"""
    names = _kernels(built)
    seen = set()
    for widths in ((1,), (3,), (1024,), (1, 1024), LADDER, MIXED16, (1023, 1024), (255, 256), (511, 512), tuple(range(1, 17))):
        rc, blocks, threads, lds, tile, kept, nseg = built.pulse_geometry(widths, 64, 3, 1000)
        k = names[(lds // 4, tile // 256)]
        assert rc == 0 and k["group_segment_fixed_size"] == lds and threads == k["max_flat_workgroup_size"] == 256, widths
        assert (tile, lds, kept) == pulse_ref.plan(widths)[:3], widths
        seen.add((tile, lds))
    assert {lds for _, lds in seen} == {16384, 32768, 65536} and {tile for tile, _ in seen} == {1024, 512, 256}, seen


def test_geometry_at_the_plans_borders(built):
    geo = built.pulse_geometry
    # levels_kept: the distinct bits set over the table
    for widths, kept in (((1,), 1), ((2,), 1), ((3,), 2), ((1023,), 10), ((1024,), 1), (LADDER, 11), ((5, 10), 4), ((1023, 1024), 11),
                         (MIXED16, 10), ((6, 24, 96), 6)):
        rc, _, threads, lds, tile, got, _ = geo(widths, 64)
        assert (rc, threads, got) == (0, 256, kept) and got == len({a for w in widths for a in pulse_ref.bits_of(w)}), widths
    # tile_out: every w_max behind a ladder of j + 1 kept levels; the tile falls exactly where rows * row passes 16384 words
    tiles, steps = set(), set()
    for j in range(11):
        head = [1 << a for a in range(j + 1)]
        last = None
        for w_max in range(head[-1], 1025):
            widths = head if w_max == head[-1] else head + [w_max]
            rc, _, _, lds, tile, kept, _ = geo(widths, 64)
            want_tile, want_lds, want_kept, rows, row = pulse_ref.plan(widths)
            assert (rc, tile, lds, kept) == (0, want_tile, want_lds, want_kept), widths
            assert rows * row <= lds // 4 and (tile == 1024 or rows * ((2 * tile + w_max - 1 + 3) // 4 * 4) > 16384), widths
            assert lds == 16384 or rows * row > lds // 8, widths
            if last is not None and tile != last:                  # a w_max one larger: another row length, or other bits
                steps.add((last, tile))
            last = tile
            tiles.add(tile)
    assert tiles == {1024, 512, 256} and steps >= {(1024, 512), (512, 256), (512, 1024)}, steps
    # written out: three rows of 2048 at {1024}; eleven of 1280 at {1023, 1024}; eight rows of 2048 fill 64 KiB, nine do not
    assert pulse_ref.plan((1024,)) == (1024, 32768, 1, 3, 2048) and geo((1024,), 64)[3:5] == (32768, 1024)
    assert pulse_ref.plan((1023, 1024)) == (256, 65536, 11, 11, 1280) and geo((1023, 1024), 64)[3:5] == (65536, 256)
    assert geo((1, 2, 4, 8, 16, 1024), 64)[3:5] == (65536, 1024) and geo((1, 2, 4, 8, 16, 32, 1024), 64)[3:5] == (65536, 512)
    assert geo((1, 2, 4, 8, 16, 32, 64, 128, 256, 1024), 64)[4] == 256
    # nseg = ceil(nout / seg), blocks = ntrials * nseg
    for seg in (64, 68, 1024, 1 << 20):
        for nout in (0, 1, seg - 1, seg, seg + 1, 5 * seg + 3, 1 << 30):
            for ntrials in (1, 3, 65536):
                rc, blocks, _, _, _, _, nseg = geo(LADDER, seg, ntrials, nout)
                if -(-nout // seg) * ntrials > 2 ** 31 - 1:
                    assert rc == -1 and "more workgroups than one grid holds" in built.pulse_last_error()
                else:
                    assert (rc, nseg, blocks) == (0, -(-nout // seg), ntrials * -(-nout // seg)), (seg, nout, ntrials)
                    assert built.pulse_last_error() == ""
    # any pointer behind nout may be null
    w = _i32(LADDER)
    assert built.pulse_lib().rtlws_pulse_geometry(11, w.ctypes.data, 64, 1, 10, None, None, None, None, None, None) == 0


def test_pulse_refusals_need_no_gpu(built):
    L = built.pulse_lib()
    err = built.pulse_last_error
    for widths in ((1,), (1024,), LADDER, MIXED16, tuple(range(1, 17))):
        for seg in (64, 68, 1 << 20):
            assert built.pulse_supported(widths, seg) == 1 and err() == ""
    w = _i32(LADDER)

    def each(nwidths=11, table=w.ctypes.data, seg=64, ntrials=1, nout=5):
        yield "rtlws_pulse_geometry", L.rtlws_pulse_geometry(nwidths, table, seg, ntrials, nout, None, None, None, None, None, None) == -1, err()
        yield "rtlws_pulse_open", not L.rtlws_pulse_open(None, nwidths, table, seg), err()
        yield "rtlws_pulse", L.rtlws_pulse_supported(nwidths, table, seg) == 0, err()

    def table_of(*widths):
        a = _i32(widths)
        return {"nwidths": a.size, "table": a.ctypes.data, "_keep": a}

    for kw, word in (({"nwidths": 0}, "nwidths must be 1 .. 16"), ({"nwidths": 17}, "nwidths must be"), ({"nwidths": -1}, "nwidths"),
                     ({"table": None}, "null widths"), (table_of(0), "every width must be 1 .. 1024"), (table_of(1, 1025), "every width"),
                     (table_of(-3, 4), "every width"), (table_of(1, 1), "the widths must be strictly ascending"),
                     (table_of(1, 5, 4), "strictly ascending"), ({"seg": 63}, "seg must be 64 .. 1048576 and a multiple of 4"),
                     ({"seg": 60}, "seg must be"), ({"seg": 66}, "seg must be"), ({"seg": (1 << 20) + 4}, "seg must be"), ({"seg": 0}, "seg")):
        args = {k: v for k, v in kw.items() if k != "_keep"}        # kw keeps the table's array alive
        for fn, refused, why in each(**args):
            assert refused and word in why and why.startswith(fn + ": "), (args, fn, why)
    # the table's rules in order: nwidths, null, the entries as they come, seg
    for fn, refused, why in each(nwidths=0, table=None, seg=0):
        assert refused and "nwidths" in why
    for fn, refused, why in each(table=None, seg=0):
        assert refused and "null widths" in why
    t = table_of(3, 2, 2000)
    for fn, refused, why in each(nwidths=3, table=t["table"], seg=0):
        assert refused and "strictly ascending" in why
    # geometry alone: ntrials, nout, the grid, in that order behind the table
    geo = lambda **kw: (L.rtlws_pulse_geometry(kw.get("nwidths", 11), w.ctypes.data, kw.get("seg", 64), kw.get("ntrials", 1), kw.get("nout", 5),
                                               None, None, None, None, None, None), err())
    assert geo() == (0, "")
    for kw, word in (({"ntrials": 0}, "ntrials must be 1 .. 65536"), ({"ntrials": 65537}, "ntrials must be"), ({"nout": -1}, "nout must be 0 .. 2^30"),
                     ({"nout": (1 << 30) + 1}, "nout must be"), ({"ntrials": 65536, "nout": 1 << 30}, "more workgroups than one grid holds"),
                     ({"seg": 0, "ntrials": 0, "nout": -1}, "seg must be"), ({"ntrials": 0, "nout": -1}, "ntrials"),
                     ({"ntrials": 65536, "nout": (1 << 30) + 1}, "nout must be")):
        rc, why = geo(**kw)
        assert rc == -1 and word in why and why.startswith("rtlws_pulse_geometry: "), (kw, why)
    h = L.rtlws_pulse_open(None, 11, w.ctypes.data, 64)
    assert not h and err() == "rtlws_pulse_open: null engine (no usable HIP device: there is no CPU path)"
    with pytest.raises(RuntimeError):
        built.PulsePlan(None, LADDER, 64)
    L.rtlws_pulse_close(None)
    for fn in (L.rtlws_pulse_samples_needed, L.rtlws_pulse_segments):
        assert fn(None, 5) == -1 and "null plan" in err()
        assert fn(None, -1) == -1 and "nout must be 0 .. 2^30" in err()
        assert fn(None, (1 << 30) + 1) == -1 and "nout must be" in err()

    A, B, Cc, D = 1 << 20, 2 << 20, 3 << 20, 4 << 20           # stand-ins for device pointers: never dereferenced
    base = (("plan", None), ("din", A), ("istride", 104), ("ntrials", 2), ("nout", 100), ("peak", B), ("at", Cc), ("mom", D), ("st", None))

    def run(**kw):
        assert set(kw) <= {k for k, _ in base}
        return L.rtlws_pulse_run(*[kw.get(k, v) for k, v in base]), err()

    for kw, word in (({"ntrials": 0}, "ntrials must be 1 .. 65536"), ({"ntrials": 65537}, "ntrials must be"), ({"nout": -1}, "nout must be 0 .. 2^30"),
                     ({"nout": (1 << 30) + 4, "istride": 1 << 31}, "nout must be"), ({"istride": 96}, "in_stride must be >= samples_needed"),
                     ({"istride": 0}, "in_stride must be >="), ({"istride": 102}, "in_stride must be a multiple of 4"),
                     ({"din": None}, "null pointer"), ({"peak": None}, "null pointer"), ({"at": None}, "null pointer"),
                     ({"din": A + 4}, "d_in must be 16-byte aligned"), ({"din": A + 8}, "d_in must be 16-byte"),
                     ({"peak": B + 2}, "d_peak must be 4-byte aligned"), ({"at": Cc + 1}, "d_at must be 4-byte aligned"),
                     ({"mom": D + 4}, "d_mom must be 8-byte aligned"), ({}, "null plan"), ({"mom": None}, "null plan"),
                     ({"nout": 0, "din": None, "peak": None, "at": None, "mom": None, "istride": 0}, "null plan"), ({"istride": 1 << 40}, "null plan")):
        rc, why = run(**kw)
        assert rc == -1 and word in why and why.startswith("rtlws_pulse_run: "), (kw, why)
    # the order: a call that breaks rule i and every later rule it still can (an earlier rule's value of an argument
    # stands) is refused for rule i
    chain = (({"ntrials": 0}, "ntrials"), ({"nout": -1}, "nout must be"), ({"istride": 2}, "in_stride must be >="), ({"istride": 102}, "multiple of 4"),
             ({"at": None}, "null pointer"), ({"din": A + 4}, "d_in"), ({"peak": B + 2}, "d_peak"), ({"at": Cc + 2}, "d_at"), ({"mom": D + 4}, "d_mom"),
             ({}, "null plan"))
    for i, (_, word) in enumerate(chain):
        kw = {}
        for later, _ in reversed(chain[i:]):
            kw.update(later)
        rc, why = run(**kw)
        assert rc == -1 and word in why, (i, kw, why)
    # the header's wording of the order names the same things in the same order
    txt = re.sub(r"\s+\*\s+", " ", open(os.path.join(INCLUDE, "rtlws_pulse.h")).read())
    order = re.search(r"in this order: (.*?)0; -1 bad argument", txt, re.S).group(1)
    places = [order.index(word) for word in ("ntrials", "nout", "in_stride at least", "multiple of 4", "null pointers", "alignments", "null plan",
                                             "in_stride >= samples_needed", "the grid")]
    assert places == sorted(places)
    # a refusal here leaves a sibling's error slot empty
    assert built.dedisp_supported(64, 3) == 1
    assert run(nout=-1)[0] == -1 and err() != "" and built.dedisp_last_error() == ""


def test_snr_is_the_expression(built):
    """rtlws_pulse_snr against the same expression in numpy f64 to 1e-12 relative, on sums whose variance is of the order
    of mean^2 (the subtraction in var then costs about one digit); NaN where it is not defined"""
    rng = np.random.default_rng(5)
    worst = 0.0
    for trial in range(200):
        count = int(rng.integers(2, 100000))
        mean, sigma = rng.uniform(0.5, 50.0) * rng.choice([-1.0, 1.0]), 0.0
        sigma = abs(mean) * rng.uniform(0.5, 2.0)
        x = rng.normal(mean, sigma, min(count, 4096))
        sum1, sum2 = float(x.sum()) * count / x.size, float((x * x).sum()) * count / x.size
        width = int(rng.integers(1, 1025))
        peak = width * mean + rng.uniform(-3.0, 30.0) * sigma * math.sqrt(width)
        got, want = built.pulse_snr(peak, width, sum1, sum2, count), float(pulse_ref.snr(peak, width, sum1, sum2, count))
        var = sum2 / count - (sum1 / count) ** 2
        assert 0.1 * mean * mean < var < 10 * mean * mean
        assert math.isfinite(want) and abs(got - want) <= 1e-12 * abs(want), (trial, got, want)
        worst = max(worst, abs(got - want) / abs(want))
    print("rtlws_pulse_snr: at most %.3g relative from the numpy expression" % worst)
    assert built.pulse_snr(10.0, 4, 8.0, 24.0, 8) == (10.0 - 4.0) / math.sqrt(4 * 2.0)          # mean 1, var 2
    nan = float("nan")
    for args in ((1.0, 1, 1.0, 1.0, 1), (1.0, 1, 1.0, 1.0, 0), (1.0, 1, 1.0, 1.0, -5), (1.0, 0, 0.0, 8.0, 8), (1.0, -2, 0.0, 8.0, 8),
                 (1.0, 4, 8.0, 8.0, 8), (1.0, 4, 8.0, 7.0, 8), (1.0, 4, nan, 24.0, 8), (1.0, 4, 8.0, nan, 8), (1.0, 4, float("inf"), 24.0, 8)):
        assert math.isnan(built.pulse_snr(*args)) and math.isnan(pulse_ref.snr(*args)), args
    assert math.isnan(built.pulse_snr(nan, 4, 8.0, 24.0, 8))


# ---- the yardstick's own properties ---------------------------------------------------------------------------

def test_boxcar_is_the_sum_in_its_own_order():
    x = pulse_ref.signed_series(2, 3000, seed=1)
    assert x.dtype == np.float32 and np.isfinite(x).all() and (x != 0).all() and 0.4 < np.signbit(x).mean() < 0.6
    expo = np.frexp(x)[1]
    assert expo.max() - expo.min() == 12                                           # 2^-6 .. 2^6
    # by hand: w = 1, 2, 3, 5, 7
    f = lambda a, b: (a + b).astype(np.float32)
    n = 2990
    s = lambda j: x[:, j:j + n]
    p1 = lambda j: f(s(j), s(j + 1))
    p2 = lambda j: f(p1(j), p1(j + 2))
    for w, want in ((1, s(0)), (2, p1(0)), (3, f(p1(0), s(2))), (4, p2(0)), (5, f(p2(0), s(4))), (6, f(p2(0), p1(4))),
                    (7, f(f(p2(0), p1(4)), s(6)))):
        got = pulse_ref.boxcar(x, w)
        assert got.dtype == np.float32 and np.array_equal(got[:, :n].view(np.uint32), want.view(np.uint32)), w
    # the order is part of the contract: from w = 5 on a good share of the outputs differ from the ascending sum
    for w in (1, 2):
        assert np.array_equal(pulse_ref.boxcar(x, w), pulse_ref.sequential(x, w))
    for w in (5, 7, 8, 15, 100, 1023, 1024):
        assert (pulse_ref.boxcar(x, w) != pulse_ref.sequential(x, w)).mean() > 0.15, w
    # the levels are built once for a table: the same bits as one width at a time
    for w, b in zip(MIXED16, pulse_ref.boxcars(x, MIXED16)):
        assert b.shape == (2, 3000 - w + 1) and np.array_equal(b.view(np.uint32), pulse_ref.boxcar(x, w).view(np.uint32))


def test_translation():
    """B of the samples from n0 on is B of the whole run from n0 on, bit for bit, at every width of the bound's list"""
    x = pulse_ref.signed_series(1, 2600, seed=2)
    for w in BOUND_WIDTHS:
        whole = pulse_ref.boxcar(x, w)
        for n0 in (1, 3, 64, 257):
            assert np.array_equal(pulse_ref.boxcar(x[:, n0:], w).view(np.uint32), whole[:, n0:].view(np.uint32)), (w, n0)
    # and the peaks of a run from a multiple of seg on: the same, `at` shifted
    seg, nout, widths = 64, 600, (1, 3, 8, 100)
    peak, at, mom = pulse_ref.pulse_ref(x, widths, seg, nout)
    peak3, at3, mom3 = pulse_ref.pulse_ref(x[:, 3 * seg:], widths, seg, nout - 3 * seg)
    assert np.array_equal(peak3.view(np.uint32), peak[:, :, 3:].view(np.uint32)) and np.array_equal(at3 + 3 * seg, at[:, :, 3:])
    assert np.array_equal(mom3.view(np.uint64), mom[:, 3:].view(np.uint64))


def test_the_f64_bound_holds_and_is_not_idle():
    x = pulse_ref.signed_series(3, 4096, seed=3)
    x64 = x.astype(np.float64)
    worst = {}
    for w in BOUND_WIDTHS:
        assert pulse_ref.depth(w) == int(math.log2(w)) + bin(w).count("1") - 1
        err = np.abs(pulse_ref.boxcar(x, w).astype(np.float64) - pulse_ref.boxcar(x64, w))
        lim = pulse_ref.bound(x, w)
        assert np.all(err <= lim), w
        worst[w] = float((err[lim > 0] / lim[lim > 0]).max()) if w > 1 else 0.0
    assert worst[1] == 0.0 and pulse_ref.depth(1) == 0 and 0.5 < worst[2] <= 1.0 and all(0 < worst[w] <= 1.0 for w in BOUND_WIDTHS[1:])
    print("worst |B - B64| / bound: %.3f at w = %d" % max((v, w) for w, v in worst.items()))
    assert pulse_ref.worst_ratio(x, BOUND_WIDTHS[:16], 1000) <= 1.0


def test_peaks_tie_rule_and_empty_segments():
    seg, nout = 64, 200
    b = pulse_ref.signed_series(3, nout, seed=4)
    b[0, 64:128] = 0.0
    b[0, 70], b[0, 90] = -0.0, 0.0                                # a segment of zeros of both signs: the first one, +0.0 at 64
    b[1, 64:128] = -0.0
    b[1, 100] = 0.0                                               # -0.0 first: it wins with its own bits over the later +0.0
    b[2, 0:64] = np.nan                                           # nothing above -Inf
    b[2, 64:128] = -np.inf
    b[2, 130], b[2, 150], b[2, 131] = 1e6, 1e6, np.nan         # equal maxima: the smaller n; a NaN next to it never wins
    b[1, 128:192] = np.nan
    b[1, 191] = -1e30                                             # one value in a segment of NaN, at its last n
    b[0, 192:200] = -5.0
    b[0, 199] = np.inf
    peak, at = pulse_ref.peaks(b, seg, nout)
    slow_peak, slow_at = pulse_ref.peaks_by_the_letter(b, seg, nout)
    assert np.array_equal(peak.view(np.uint32), slow_peak.view(np.uint32)) and np.array_equal(at, slow_at)
    assert peak.shape == (3, 4) and at.dtype == np.int32
    assert (at[0, 1], peak[0, 1].view(np.uint32)) == (64, 0) and (at[1, 1], peak[1, 1].view(np.uint32)) == (64, 0x80000000)
    assert (at[2, 0], at[2, 1]) == (-1, -1) and np.all(peak[2, :2].view(np.uint32) == 0xFF800000)
    assert (at[2, 2], peak[2, 2]) == (130, 1e6) and (at[1, 2], peak[1, 2]) == (191, np.float32(-1e30))
    assert (at[0, 3], peak[0, 3]) == (199, np.inf)
    # on data: against the letter, the last segment short
    x = pulse_ref.signed_series(2, 333, seed=6)
    for seg, nout in ((64, 333), (68, 330), (64, 1), (64, 65)):
        a, b2 = pulse_ref.peaks(x, seg, nout), pulse_ref.peaks_by_the_letter(x, seg, nout)
        assert np.array_equal(a[0].view(np.uint32), b2[0].view(np.uint32)) and np.array_equal(a[1], b2[1]) and a[0].shape == (2, -(-nout // seg))


def test_moments_against_fsum():
    """the residue classes and the tree against math.fsum: within 300 2^-53 sum|terms| (at most 256 + 8 additions on a path
    here); the classes by the letter on a short segment"""
    seg, nout = 5000, 12000
    x = pulse_ref.signed_series(2, nout, seed=7)
    mom = pulse_ref.moments(x, seg, nout)
    assert mom.shape == (2, 3, 2) and mom.dtype == np.float64
    for t in range(2):
        for s in range(3):
            part = [float(v) for v in x[t, s * seg:min((s + 1) * seg, nout)]]
            for j, terms in enumerate((part, [v * v for v in part])):
                assert abs(mom[t, s, j] - math.fsum(terms)) <= 300 * 2.0 ** -53 * math.fsum(abs(v) for v in terms), (t, s, j)
    # by the letter
    part = x[0, :700].astype(np.float64)
    q = [0.0] * 256
    for j, v in enumerate(part):
        q[j % 256] = q[j % 256] + v * v
    h = 128
    while h >= 1:
        for i in range(h):
            q[i] = q[i] + q[i + h]
        h //= 2
    assert pulse_ref.moments(x[:1, :700], 1024, 700)[0, 0, 1] == q[0]
    # a segment of -0.0 sums to +0.0; NaN and Inf propagate
    z = np.full((1, 64), -0.0, np.float32)
    assert not pulse_ref.moments(z, 64, 64).view(np.uint64).any()
    z[0, 5] = np.inf
    assert np.all(pulse_ref.moments(z, 64, 64) == np.inf)


def test_pulse_ref_reads_nothing_behind_samples_needed():
    widths, seg, nout = (1, 3, 8), 64, 150
    need = pulse_ref.samples_needed(widths, nout)
    assert need == 157 and pulse_ref.samples_needed(widths, 0) == 0 and pulse_ref.segments(nout, seg) == 3
    x = np.full((2, need + 5), np.nan, np.float32)
    x[:, :need] = pulse_ref.signed_series(2, need, seed=8)
    peak, at, mom = pulse_ref.pulse_ref(x, widths, seg, nout)
    assert np.isfinite(peak).all() and np.isfinite(mom).all() and at.min() >= 0 and at.max() < nout
    assert np.all(at // seg == np.arange(3)[None, None, :])
    # a planted pulse of width 8 wins at every width where it starts, and most clearly at its own
    x[0, 70:78] += 500.0
    peak, at, mom = pulse_ref.pulse_ref(x, widths, seg, nout)
    assert at[0, 2, 1] == 70 and 64 <= at[0, 0, 1] < 78
    snr = [pulse_ref.snr(peak[0, k, 1], w, mom[0, 0, 0], mom[0, 0, 1], 64) for k, w in enumerate(widths)]
    assert snr[2] > snr[1] > snr[0] > 5

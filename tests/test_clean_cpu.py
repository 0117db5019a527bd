"""CPU suite of include/rtlws_clean.h: the restatement's own properties (tests/clean_ref.py: its orders, the statistical
claim on the synthetic waterfall, the zero-DM property and its bound, the tie to dedisp_ref, the later-block property, what
a non-finite sample, a constant channel and a MAD of zero do), and what the library does without a GPU: the union mask, its
exports, the header as strict C99, the rules at every limit and the order of a run's refusals, the geometry, the
binding's place beside the pinned surface, the new sources' preprocessor lines, the kernels' registers and LDS."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import clean_ref
import dedisp_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "rtl-ws_amd", "csrc")
INCLUDE = os.path.join(ROOT, "include")
NEW_SOURCES = [os.path.join(CSRC, f) for f in ("clean.h", "clean.hip", "clean_shim.hip", "search_plan.h")] + [os.path.join(INCLUDE, "rtlws_clean.h")]
INF = float("inf")
SEEDS = range(20)


@pytest.fixture(scope="module")
def clean(built):
    import rtlws.clean
    return rtlws.clean


def bits(x):
    return np.ascontiguousarray(x).view(np.uint32 if x.dtype == np.float32 else np.uint64)


def same_bits(x, y):
    return x.shape == y.shape and x.dtype == y.dtype and np.array_equal(bits(x), bits(y))


@pytest.fixture(scope="module")
def skies():
    """the prototype's waterfall at every seed, cleaned once with and once without the zero-DM filter:
    seed -> (rows, delays, with, without), each of the last two clean_ref's four outputs"""
    made = {}
    for seed in SEEDS:
        rows, delays = clean_ref.sky(seed)
        made[seed] = (rows, delays, clean_ref.clean_ref(rows, clean_ref.SKY["B"], None, 6.0, 6.0, True),
                      clean_ref.clean_ref(rows, clean_ref.SKY["B"], None, 6.0, 6.0, False))
    return made


# ---- the restatement ----------------------------------------------------------------------------------------------

def test_the_orders_are_not_idle():
    rows = dedisp_ref.signed_rows(64, 24, seed=3)
    # 20 binades of 24-bit values add exactly in f64 in any order: spread them over 60 more
    rows = rows * np.exp2(dedisp_ref.hashed_ints(64 * 24, 60, 4).reshape(64, 24) - 30).astype(np.float32)
    s1, s2 = clean_ref.sums_ref(rows)
    t1, t2 = clean_ref.sums_ref(rows, residues=4)
    assert not same_bits(s1, t1) and not same_bits(s2, t2)
    assert np.allclose(s1, t1, rtol=1e-12, atol=1e-9) and np.allclose(s2, t2, rtol=1e-12)
    tree, plain = clean_ref.row_tree(rows), clean_ref.row_tree(rows, pairwise=False)
    assert not same_bits(tree, plain) and np.allclose(tree, plain, rtol=0, atol=24 * 2.0 ** -24 * np.abs(rows).sum(axis=1).max())
    # G = 8 for 24 channels: two padded lanes, which add +0.0
    assert clean_ref.pow2_at_least(24 // 4) == 8 and same_bits(clean_ref.row_tree(np.ones((1, 24), np.float32)), np.array([24], np.float32))


def test_the_statistical_claim(skies):
    """20 seeds of the prototype's waterfall: every planted channel flagged in every block, at most 1 % of the good (block,
    channel) pairs flagged (measured: 0 of 2250 per seed), the dedispersed series' maximum within one row of the planted
    pulse and above 8 sigma, sigma = sqrt(nkept) (measured: 11.3 .. 14.6)"""
    k = clean_ref.SKY
    good = np.ones(k["nchan"], bool)
    good[list(clean_ref.PLANTED)] = False
    snrs, wrong = [], []
    for seed in SEEDS:
        rows, delays, (out, keep, stats, nkept), _ = skies[seed]
        assert keep.shape == (9, k["nchan"]) and not keep[:, ~good].any(), (seed, np.argwhere(keep[:, ~good]))
        wrong.append(int((keep[:, good] == 0).sum()))
        assert wrong[-1] <= 0.01 * good.sum() * keep.shape[0], (seed, wrong[-1])
        assert np.array_equal(nkept, keep.sum(axis=1))
        series = dedisp_ref.dedisp_ref(out, delays[None, :])[0]
        at = int(np.argmax(series))
        snrs.append(float(series[at]) / np.sqrt(float(nkept.max())))
        assert k["pulse_row"] - 1 <= at <= k["pulse_row"] + k["pulse_width"], (seed, at)
        assert snrs[-1] > 8.0, (seed, snrs[-1])
        quiet = np.delete(series, np.arange(k["pulse_row"] - 4, k["pulse_row"] + 6))
        assert abs(quiet.mean()) < 0.1 * quiet.std() and 0.9 < quiet.std() / np.sqrt(nkept.mean()) < 1.1, (seed, quiet.mean(), quiet.std())
    print("good pairs flagged per seed:", wrong, "snr %.1f .. %.1f" % (min(snrs), max(snrs)))


def test_the_zero_dm_property(skies):
    """the row-sum bound on every row; the DM-0 series of the filtered rows below 1e-3 sqrt(nkept) at the burst's rows, and
    that of the unfiltered rows above 10 sigma there (measured: 13.6 .. 17.9 sigma at the middle row; the largest row sum 0.18 of its bound)"""
    k = clean_ref.SKY
    zero = np.zeros((1, k["nchan"]), np.int32)
    shares, peaks = [], []
    for seed in SEEDS:
        rows, _, (out, keep, stats, nkept), (v, keep_v, _, _) = skies[seed]
        assert np.array_equal(keep, keep_v)
        total = np.abs(out.astype(np.float64).sum(axis=1))
        bound = clean_ref.zerodm_bound(v)
        assert np.all(total <= bound), (seed, np.argmax(total / bound), (total / bound).max())
        shares.append(float((total / bound).max()))
        burst = slice(k["burst_row"], k["burst_row"] + k["burst_width"])
        sigma = np.sqrt(float(nkept[k["burst_row"] // k["B"]]))
        with_filter, without = dedisp_ref.dedisp_ref(out, zero)[0], dedisp_ref.dedisp_ref(v, zero)[0]
        assert np.all(np.abs(with_filter[burst]) < 1e-3 * sigma), (seed, with_filter[burst])
        assert np.all(without[burst] > 10.0 * sigma), (seed, without[burst] / sigma)
        assert int(np.argmax(without)) in range(burst.start, burst.stop), seed
        peaks.append(float(without[k["burst_row"] + 1] / sigma))
    print("largest share of the bound %.3f; burst %.1f .. %.1f sigma" % (max(shares), min(peaks), max(peaks)))


def test_cleaned_rows_need_no_mask(skies):
    """inside a block, dedispersing the cleaned rows with no mask gives the bits of dedispersing them with keep[b] as the
    mask: a flagged channel is +0.0, and the accumulator is never -0.0"""
    k = clean_ref.SKY
    rows, delays, (out, keep, _, _), _ = skies[0]
    assert not out[:, list(clean_ref.PLANTED)].any() and not np.signbit(out[:, list(clean_ref.PLANTED)]).any()
    table = np.stack([np.zeros(k["nchan"], np.int32), delays // 4, dedisp_ref.hashed_ints(k["nchan"], 70, 5)])
    for b in range(keep.shape[0]):
        part = out[b * k["B"]:min((b + 1) * k["B"], out.shape[0])]
        assert same_bits(dedisp_ref.dedisp_ref(part, table), dedisp_ref.dedisp_ref(part, table, keep[b])), b
    # signed rows, where sums cancel to zero
    signed = dedisp_ref.signed_rows(96, 16, seed=4)
    signed[:, 1::2] = -signed[:, 0::2]
    signed[:, 5] = 3.0
    out, keep, _, nkept = clean_ref.clean_ref(signed, 32, None, INF, INF, False)
    assert not keep[:, 5].any() and np.all(nkept == 15)
    small = np.array([[0] * 16, [3, 1] * 8], np.int32)
    for b in range(3):
        part = out[b * 32:(b + 1) * 32]
        assert same_bits(dedisp_ref.dedisp_ref(part, small), dedisp_ref.dedisp_ref(part, small, keep[b])), b


@pytest.mark.parametrize("zerodm", [False, True])
def test_a_run_from_a_later_block(zerodm):
    B, M = 32, 24
    for nrows in (B + 1, 2 * B + B // 2, 5 * B + 7):
        rows = dedisp_ref.signed_rows(nrows, M, seed=nrows)
        whole = clean_ref.clean_ref(rows, B, None, 6.0, 6.0, zerodm)
        for b0 in range(1, clean_ref.blocks_of(nrows, B)):
            if nrows - b0 * B < B:
                continue                                                       # fewer than B rows are no run
            part = clean_ref.clean_ref(rows[b0 * B:], B, None, 6.0, 6.0, zerodm)
            assert same_bits(part[0], whole[0][b0 * B:]) and np.array_equal(part[1], whole[1][b0:])
            assert same_bits(part[2], whole[2][b0:]) and np.array_equal(part[3], whole[3][b0:])


def test_the_last_block_looks_back():
    """nrows = B + 1: block 1 owns one row and takes its statistics from rows 1 .. B; nrows = 2B + B/2: from rows B + B/2 on"""
    B, M = 32, 8
    for nrows in (B + 1, 2 * B + B // 2):
        rows = dedisp_ref.hashed_rows(nrows, M, seed=nrows + 1)
        out, keep, stats, nkept = clean_ref.clean_ref(rows, B, None, INF, INF, False)
        last = clean_ref.blocks_of(nrows, B) - 1
        mu, sd, m, r, valid = clean_ref.stats_ref(rows[nrows - B:])
        assert valid.all() and same_bits(stats[last, :, 0], m) and same_bits(stats[last, :, 1], r)
        assert same_bits(out[last * B:], ((rows[last * B:] - m[None, :]) * r[None, :]).astype(np.float32))
        assert clean_ref.window_start(last, B, nrows) == nrows - B and clean_ref.window_start(0, B, nrows) == 0


def test_a_non_finite_sample_flags_its_channel_where_its_window_holds_it():
    B, M = 32, 12
    rows = dedisp_ref.hashed_rows(3 * B + 5, M, seed=8)
    rows[B + 3, 2], rows[7, 9], rows[3 * B + 1, 4] = np.nan, np.inf, -np.inf
    out, keep, stats, nkept = clean_ref.clean_ref(rows, B, None, INF, INF, True)
    want = np.ones((4, M), np.uint8)
    want[1, 2] = want[0, 9] = want[3, 4] = 0           # the last block's window is rows 2B + 5 .. 3B + 4
    assert np.array_equal(keep, want) and np.array_equal(nkept, want.sum(axis=1)) and np.isfinite(out).all()
    assert not stats[1, 2].any() and not stats[0, 9].any() and stats[0, 2].all()
    # a sample in the look-back's overlap flags both blocks that see it
    rows = dedisp_ref.hashed_rows(2 * B + 4, M, seed=9)
    rows[B + 20, 6] = np.nan
    keep = clean_ref.clean_ref(rows, B, None, INF, INF, True)[1]
    assert keep[:, 6].tolist() == [1, 0, 0] and keep.sum() == 3 * M - 2


def test_constant_channels_and_an_all_constant_block():
    B, M = 32, 8
    rows = dedisp_ref.hashed_rows(2 * B, M, seed=2)
    rows[:, 3] = 0.1                                     # 0.1f squared is not exact in f32, and exact in f64: var == 0
    rows[B:] = np.arange(M, dtype=np.float32)[None, :] + 0.3
    out, keep, stats, nkept = clean_ref.clean_ref(rows, B)
    assert np.isfinite(out).all()                        # nkept == 0: no division, 0 / 0 would be NaN
    assert keep[0].tolist() == [1, 1, 1, 0, 1, 1, 1, 1] and not keep[1].any() and nkept.tolist() == [M - 1, 0]
    assert not out[B:].any() and not np.signbit(out[B:]).any() and not stats[1].any() and not stats[0, 3].any()
    assert not out[:, 3].any() and not np.signbit(out[:, 3]).any()


def test_a_mad_of_zero():
    """t = +Inf makes no test, whatever the MAD; a finite t over a MAD of zero keeps only the channels at the median"""
    B, M = 32, 16
    base = dedisp_ref.hashed_rows(B, 1, seed=6)
    rows = np.repeat(base, M, axis=1)
    rows[:, 2] *= 2.0                                    # another mean and another sd
    rows[:, 11] = rows[::-1, 11] * 1.0                   # the same values in another order: the same sums?  not bit for bit
    mu, sd, m, r, valid = clean_ref.stats_ref(rows)
    assert valid.all() and len(set(mu.tolist())) >= 2
    for t in (0.0, 6.0, 1e300):
        keep = clean_ref.clean_ref(rows, B, None, t, INF, False)[1][0]
        assert np.array_equal(keep != 0, mu == clean_ref.med(mu)), t
        keep = clean_ref.clean_ref(rows, B, None, INF, t, False)[1][0]
        assert np.array_equal(keep != 0, sd == clean_ref.med(sd)), t
    assert not clean_ref.clean_ref(rows, B, None, 6.0, 6.0, False)[1][0, 2]
    assert clean_ref.clean_ref(rows, B, None, INF, INF, False)[1].all()
    # t = 0 with a positive MAD keeps the median's channel alone (and its equals)
    rows = dedisp_ref.hashed_rows(B, M, seed=7)
    mu = clean_ref.stats_ref(rows)[0]
    keep = clean_ref.clean_ref(rows, B, None, 0.0, INF, False)[1][0]
    assert keep.sum() == 1 and mu[np.argmax(keep)] == clean_ref.med(mu)


def test_the_median_is_an_element():
    assert clean_ref.med([3.0, 1.0, 2.0, 4.0]) == 2.0 and clean_ref.med([5.0]) == 5.0 and clean_ref.med([2.0, 1.0]) == 1.0


# ---- the library without a GPU ------------------------------------------------------------------------------------

def test_union_mask(clean):
    keep = (dedisp_ref.hashed_ints(7 * 12, 3, 5).reshape(7, 12) != 0).astype(np.uint8)
    keep[:, 0], keep[:, 1] = 1, 0
    for share in (0.0, 0.25, 0.5, 5.0 / 7.0, 0.75, 1.0):
        got = clean.union_mask(keep, share)
        assert got.dtype == np.uint8 and np.array_equal(got, clean_ref.union_mask(keep, share)), share
    assert clean.union_mask(keep, 0.0).all() and clean.union_mask(keep, 1.0)[0] == 1 and clean.union_mask(keep, 1e-9)[1] == 0
    assert np.array_equal(clean.union_mask(keep, 1.0), keep.all(axis=0).astype(np.uint8))
    L, out = clean.lib(), (C.c_uint8 * 4096)()
    buf = (C.c_uint8 * (4096 * 2))()
    for args, text in (((None, 2, 4, 0.5, out), "null pointer"), ((buf, 2, 4, 0.5, None), "null pointer"), ((buf, 0, 4, 0.5, out), "nblocks must be >= 1"),
                       ((buf, 2, 6, 0.5, out), "nchan must be 4 .. 4096"), ((buf, 2, 4100, 0.5, out), "nchan must be 4 .. 4096"),
                       ((buf, 2, 4, -0.1, out), "min_share must be 0 .. 1"), ((buf, 2, 4, 1.5, out), "min_share must be 0 .. 1"),
                       ((buf, 2, 4, float("nan"), out), "min_share must be 0 .. 1")):
        assert L.rtlws_clean_union_mask(*args) == -1 and text in clean.last_error(), (args, clean.last_error())
    assert L.rtlws_clean_union_mask(buf, 2, 4096, 1.0, out) == 0 and clean.last_error() == ""
    with pytest.raises(ValueError):
        clean.union_mask(keep, 2.0)


def test_exports_are_the_header(clean):
    import test_abi_cpu
    declared = test_abi_cpu._declared_functions("rtlws_clean.h")
    assert len(declared) == 8 and set(declared) == set(clean.SYMBOLS)
    assert test_abi_cpu._exported(clean.CLEAN_LIB) == set(declared)
    L = clean.lib()
    assert all(getattr(L, f).argtypes is not None for f in clean.SYMBOLS)


def test_the_header_is_strict_c99(tmp_path):
    src = tmp_path / "t_rtlws_clean.c"
    src.write_text('#include "rtlws_clean.h"\nint main(void) { return rtlws_clean_supported(4, 32) ? 0 : 1; }\n')
    out = subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Wextra", "-Werror", "-I", INCLUDE, "-c", str(src), "-o", os.devnull],
                         capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    code = re.sub(r"/\*.*?\*/", "", open(os.path.join(INCLUDE, "rtlws_clean.h")).read(), flags=re.S)
    assert "hipStream_t" not in code and "hipError_t" not in code
    for name, value in (("MIN_NCHAN", 4), ("MAX_NCHAN", 4096), ("MIN_BLOCK", 32), ("MAX_BLOCK", 16384), ("MAX_NROWS", 1 << 24),
                        ("MAX_CELLS", 1 << 22), ("ZERODM", 1)):
        assert re.search(r"#define RTLWS_CLEAN_%s %d\b" % (name, value), code) and getattr(clean_ref, name) == value, name


NCHAN_TEXT, BLOCK_TEXT = "nchan must be 4 .. 4096 and a multiple of 4", "block_rows must be 32 .. 16384"
# (nchan, block_rows) -> the refusal, None when served
SHAPE_LIMITS = [((4, 32), None), ((4096, 16384), None), ((0, 32), NCHAN_TEXT), ((3, 32), NCHAN_TEXT), ((6, 32), NCHAN_TEXT), ((4100, 32), NCHAN_TEXT),
                ((4, 31), BLOCK_TEXT), ((4, 16385), BLOCK_TEXT), ((4, 33), None), ((0, 0), NCHAN_TEXT), ((-4, 32), NCHAN_TEXT)]


def test_the_rules_at_every_limit(clean):
    for args, why in SHAPE_LIMITS:
        assert bool(clean.supported(*args)) == (why is None), args
        assert clean.last_error() == ("" if why is None else "rtlws_clean: " + why), (args, clean.last_error())
        got = clean.geometry(*args, nrows=args[1])
        assert (got[0] == 0) == (why is None), args
        if why is None:
            assert got[1:] == clean_ref.geometry(*args, args[1]), (args, got)
        else:
            assert clean.last_error() == "rtlws_clean_geometry: " + why
    assert clean.lib().rtlws_clean_geometry(4, 32, 32, None, None, None, None, None, None) == 0
    for nrows, text in ((-1, "nrows must be 0 .. 2^24"), ((1 << 24) + 1, "nrows must be 0 .. 2^24"), (1, "nrows must be 0 or at least block_rows"),
                        (31, "nrows must be 0 or at least block_rows")):
        assert clean.geometry(4, 32, nrows)[0] == -1 and clean.last_error() == "rtlws_clean_geometry: " + text
    assert clean.geometry(4, 32, 0)[:2] == (0, (0, 0, 0)) and clean.geometry(4, 32, 1 << 24)[4] == 1 << 19


def test_geometry_is_the_stated_rule(clean):
    for nchan in (4, 12, 64, 252, 256, 260, 1024, 2048, 2052, 4096):
        for B in (32, 33, 40, 512, 16384):
            for nrows in (B, B + 1, 2 * B, 2 * B + B // 2, 5 * B + 7):
                got = clean.geometry(nchan, B, nrows)
                assert got == (0,) + clean_ref.geometry(nchan, B, nrows), (nchan, B, nrows, got)
                assert max(got[3]) <= 65664 and got[4] == -(-nrows // B) and got[5] <= 16 * clean_ref.MAX_CELLS + 4 * got[6]
    # the workspace: 2^22 cells or the blocks of 2^24 rows, whichever is fewer
    assert clean.geometry(4096, 32, 32)[6] == 1024 and clean.geometry(4, 32, 32)[6] == 1 << 19 and clean.geometry(1024, 16384, 16384)[6] == 1024
    assert clean.geometry(4096, 32, 1024 * 32)[0] == 0 and clean.geometry(4096, 32, 1024 * 32 + 1)[0] == -1
    assert "more blocks than the plan's workspace holds" in clean.last_error()
    assert clean.geometry(4096, 16384, 1 << 24)[:2] == (0, (1024 * 16, 1024, 1024 * 1024))


def test_open_without_an_engine(clean):
    with pytest.raises(RuntimeError, match="rtlws_clean_open: null engine"):
        clean.CleanPlan(None, 4, 32)
    nan = float("nan")
    for kwargs, text in ((dict(nchan=6), "nchan must be 4 .. 4096"), (dict(nchan=4100), "nchan must be 4 .. 4096"), (dict(block_rows=31), "block_rows must be 32"),
                         (dict(block_rows=16385), "block_rows must be 32"), (dict(t_mean=-1.0), "t_mean must be >= 0"), (dict(t_mean=nan), "t_mean must be >= 0"),
                         (dict(t_sigma=-1e-300), "t_sigma must be >= 0"), (dict(t_sigma=nan), "t_sigma must be >= 0"), (dict(t_mean=-INF), "t_mean must be >= 0"),
                         (dict(flags=2), "unknown flag bits"), (dict(flags=-1), "unknown flag bits"), (dict(t_mean=INF, t_sigma=0.0, flags=1), "null engine")):
        args = dict(nchan=4, block_rows=32)
        args.update(kwargs)
        with pytest.raises(RuntimeError, match="rtlws_clean_open: " + text):                      # the arguments come before the engine
            clean.CleanPlan(None, **args)
    L = clean.lib()
    assert L.rtlws_clean_blocks(None, 32) == -1 and "null plan" in clean.last_error()
    assert L.rtlws_clean_blocks(None, -1) == -1 and "nrows must be 0 .. 2^24" in clean.last_error()
    L.rtlws_clean_close(None)
    # a run's refusals that need no plan come before the null plan's, in the header's order:
    # (d_rows, in_stride, nrows, d_out, out_stride, d_keep, d_stats, d_nkept)
    run = lambda *args: L.rtlws_clean_run(None, *args, None)
    for args, text in (((64, 4, -1, 128, 4, None, None, None), "nrows must be 0 .. 2^24"), ((64, 4, (1 << 24) + 1, 128, 4, None, None, None), "nrows must be 0 .. 2^24"),
                       ((64, 0, 32, 128, 4, None, None, None), "in_stride must be >= 4 and a multiple of 4"), ((64, 6, 32, 128, 4, None, None, None), "in_stride must be >= 4"),
                       ((64, 4, 32, 128, 2, None, None, None), "out_stride must be >= 4 and a multiple of 4"), ((64, 4, 32, 128, 10, None, None, None), "out_stride must be >= 4"),
                       ((None, 4, 32, 128, 4, None, None, None), "null pointer"), ((64, 4, 32, None, 4, None, None, None), "null pointer"),
                       ((72, 4, 32, 128, 4, None, None, None), "d_rows must be 16-byte aligned"), ((64, 4, 32, 132, 4, None, None, None), "d_out must be 16-byte aligned"),
                       ((64, 4, 32, 128, 4, 1, 66, None), "d_stats must be 4-byte aligned"), ((64, 4, 32, 128, 4, 1, 68, 70), "d_nkept must be 4-byte aligned"),
                       ((64, 4, 32, 128, 4, 1, 68, 72), "null plan"), ((64, 4, 0, 64, 4, None, None, None), "null plan")):
        assert run(*args) == -1 and text in clean.last_error(), (args, clean.last_error())


def test_the_pinned_surface_holds_with_the_submodule(built, clean):
    """tests/test_python_api_cpu.py's snapshot with rtlws.clean imported: no new public name, no new Engine method, the
    plan no _Plan subclass"""
    import test_python_api_cpu as api
    rec, now = api._recorded(), api.snapshot(built)
    assert built.clean is clean
    for part in ("names", "functions", "methods"):
        assert now[part] == rec[part], part
    assert not issubclass(clean.CleanPlan, built._Plan) and issubclass(clean.CleanPlan, built._PlanBase)
    assert "clean" not in api.SATELLITES
    assert "librtlws_clean.so (include/rtlws_clean.h)" in clean.lib.__doc__
    assert {"supported", "geometry", "union_mask", "clean", "CleanPlan", "GUARD", "ZERODM"} <= set(vars(clean))


def test_the_new_sources_carry_no_conditionals():
    for path in NEW_SOURCES:
        lines = [ln.strip() for ln in open(path) if re.match(r"\s*#", ln)]
        other = [ln for ln in lines if not re.match(r"#\s*(include|pragma|define)\b", ln)]
        guards = [ln for ln in other if re.match(r"#\s*(ifndef RTLWS_\w+_H|endif\b|ifdef __cplusplus)", ln)]
        assert other == guards, (path, [ln for ln in other if ln not in guards])
        assert sum(ln.startswith("#ifndef") for ln in lines) == (0 if path.endswith(".hip") else 1), path


def test_no_kernel_of_the_library_spills(built, clean):
    """the code object's metadata: one kernel each of the statistics and the flags and five of the rows (the wavefronts a
    row takes: 1, 2, 4, 8, 16); no spill, no scratch, no static LDS: what geometry reports is all the LDS a workgroup has"""
    from rtlws import codeobj
    mine = codeobj.kernels(clean.CLEAN_LIB)
    assert len([k for k in mine if "clean_stats_kernel" in k["name"]]) == 1 and len([k for k in mine if "clean_flags_kernel" in k["name"]]) == 1
    assert len([k for k in mine if "clean_apply_kernel" in k["name"]]) == 5 and len(mine) == 7
    for k in mine:
        assert not k["vgpr_spill_count"] and not k.get("sgpr_spill_count", 0) and not k["private_segment_fixed_size"], k["name"]
        assert k["vgpr_count"] <= 128 and k.get("agpr_count", 0) == 0, k["name"]
        assert k["group_segment_fixed_size"] == 0, k["name"]
    assert max(max(clean.geometry(nchan, 32, 32)[3]) for nchan in range(4, 4097, 4)) == 65664       # stage 2 at 4096 channels: raised at open


def test_the_makefile_builds_it():
    txt = open(os.path.join(ROOT, "rtl-ws_amd", "Makefile")).read()
    assert re.search(r"^SATELLITES := .*\bclean\b", txt, flags=re.M)
    assert re.search(r"^\$\(eval \$\(call SATELLITE,clean,clean clean_shim,", txt, flags=re.M)
    assert re.search(r"^\$\(BUILD\)/clean\.o:.*\n\t\$\(HIPCC\) \$\(HIPFLAGS\) -ffp-contract=off ", txt, flags=re.M)
    out = subprocess.run(["nm", "-D", "--undefined-only", os.path.join(ROOT, "rtl-ws_amd", "lib", "librtlws_clean.so")],
                         capture_output=True, text=True, check=True).stdout
    assert "rtlws_engine_device" in out and "rtlws_engine_stream" in out          # the engine is librtlws_hip.so's

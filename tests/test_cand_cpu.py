"""CPU suite of include/rtlws_cand.h: the restatement's own properties (tests/cand_ref.py: the plain loop, the order, the
translation, what is never read, its tie to fold_ref over dedisp_ref), and what the library does without a GPU: the host
helpers against numpy.longdouble and their sign conventions on a planted pulsar, its exports, the header as strict C99,
the rules at every limit and the order of a run's refusals, the geometry, the binding's place beside the pinned surface,
the new sources' preprocessor lines and the kernels' registers and LDS."""
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np
import pytest

import cand_ref
import dedisp_ref
import fold_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "rtl-ws_amd", "csrc")
INCLUDE = os.path.join(ROOT, "include")
NEW_SOURCES = [os.path.join(CSRC, f) for f in ("cand.h", "cand.hip", "cand_shim.hip", "search_plan.h")] + [os.path.join(INCLUDE, "rtlws_cand.h")]


@pytest.fixture(scope="module")
def cand(built):
    import rtlws.cand
    return rtlws.cand


def bits(x):
    return np.ascontiguousarray(x).view(np.uint32 if x.dtype == np.float32 else np.uint64)


def same_bits(x, y):
    return x.shape == y.shape and x.dtype == y.dtype and np.array_equal(bits(x), bits(y))


# ---- the restatement ----------------------------------------------------------------------------------------------

CUBE_CASE = dict(nchan=8, nbins=5, sub=16, nsamp=41)


def _cube_case(seed=1):
    k = CUBE_CASE
    steps, phases = fold_ref.table(2, seed=seed, first=3.3)
    delays = dedisp_ref.hashed_ints(2 * k["nchan"], 9, seed).reshape(2, k["nchan"])
    mask = np.ones(k["nchan"], np.uint8)
    mask[3] = 0
    rows = dedisp_ref.signed_rows(k["nsamp"] + 9, k["nchan"], seed)
    return rows, steps, phases, delays, mask


def test_the_cube_is_the_plain_loop():
    k = CUBE_CASE
    rows, steps, phases, delays, mask = _cube_case()
    cube, hits = cand_ref.cube_ref(rows, steps, phases, k["nchan"], k["nbins"], k["sub"], k["nsamp"], delays, mask)
    assert cube.shape == (2, 3, k["nchan"], k["nbins"]) and hits.shape == (2, 3, k["nbins"])
    for c in range(2):
        for s in range(3):
            n0, n1 = s * k["sub"], min((s + 1) * k["sub"], k["nsamp"])
            want, count = cand_ref.cube_by_the_letter(rows, steps[c], phases[c], k["nchan"], k["nbins"], n0, n1, delays[c], mask)
            assert same_bits(cube[c, s], want) and np.array_equal(hits[c, s], count)
            assert hits[c, s].sum() == n1 - n0
    assert not cube[:, :, 3].any() and not np.signbit(cube[:, :, 3]).any()          # the masked channel: +0.0


def test_the_cubes_order_is_not_idle():
    k = CUBE_CASE
    rows, steps, phases, delays, mask = _cube_case()
    up, _ = cand_ref.cube_by_the_letter(rows, steps[0], phases[0], k["nchan"], k["nbins"], 0, k["nsamp"], delays[0], mask)
    down, _ = cand_ref.cube_by_the_letter(rows, steps[0], phases[0], k["nchan"], k["nbins"], 0, k["nsamp"], delays[0], mask,
                                          order=range(k["nsamp"] - 1, -1, -1))
    assert not same_bits(up, down)


def test_the_search_is_the_plain_loop_and_its_orders_are_not_idle():
    nsub, nchan, nbins = 5, 8, 7
    cube = cand_ref.gaussian_cube(1, nsub, nchan, nbins, seed=3)
    a, g = cand_ref.shift_table((1, 2, nchan), nbins, 4), cand_ref.shift_table((1, 3, nsub), nbins, 5)
    stat, total, P, T = cand_ref.search_ref(cube, a, g)
    for q in range(2):
        for r in range(3):
            s1, t1, p1, tt = cand_ref.search_by_the_letter(cube[0], a[0, q], g[0, r])
            assert same_bits(P[0, q, r], p1) and same_bits(T[0, q], tt)
            assert bits(np.float64(stat[0, q, r])) == bits(np.float64(s1)) and bits(np.float64(total[0, q, r])) == bits(np.float64(t1))
    _, _, p_i, t_i = cand_ref.search_by_the_letter(cube[0], a[0, 0], g[0, 0], chan_order=range(nchan - 1, -1, -1))
    assert not same_bits(t_i, T[0, 0])
    _, _, p_s, t_s = cand_ref.search_by_the_letter(cube[0], a[0, 0], g[0, 0], sub_order=range(nsub - 1, -1, -1))
    assert same_bits(t_s, T[0, 0]) and not same_bits(p_s, P[0, 0, 0])


def test_the_translation_property():
    """a run over the rows from n0 = s0 sub on with phi0 replaced by the phase at n0 gives sub-integrations s0 .. bit for bit"""
    k = CUBE_CASE
    rows, steps, phases, delays, mask = _cube_case(seed=2)
    whole, hits = cand_ref.cube_ref(rows, steps, phases, k["nchan"], k["nbins"], k["sub"], k["nsamp"], delays, mask)
    n0 = k["sub"]
    later = [fold_ref.phase_at(st, ph, n0) for st, ph in zip(steps, phases)]
    part, part_hits = cand_ref.cube_ref(rows[n0:], steps, later, k["nchan"], k["nbins"], k["sub"], k["nsamp"] - n0, delays, mask)
    assert same_bits(part, whole[:, 1:]) and np.array_equal(part_hits, hits[:, 1:])


def test_nothing_is_read_behind_the_rows_or_in_a_masked_channel():
    k = CUBE_CASE
    rows, steps, phases, delays, mask = _cube_case(seed=3)
    need = cand_ref.rows_needed(2, k["nchan"], delays, mask, k["nsamp"])
    assert need == k["nsamp"] + int(delays[:, mask != 0].max()) and cand_ref.rows_needed(2, k["nchan"], delays, mask, 0) == 0
    want = cand_ref.cube_ref(rows, steps, phases, k["nchan"], k["nbins"], k["sub"], k["nsamp"], delays, mask)
    wide = np.full((need + 4, k["nchan"] + 4), np.nan, np.float32)
    wide[:need, :k["nchan"]] = rows[:need]
    wide[:, 3] = np.nan
    got = cand_ref.cube_ref(wide, steps, phases, k["nchan"], k["nbins"], k["sub"], k["nsamp"], delays, mask)
    assert same_bits(got[0], want[0]) and np.array_equal(got[1], want[1])
    # each channel's own last row is read: a NaN there shows
    wide[k["nsamp"] - 1 + delays[0, 0], 0] = np.nan
    assert np.isnan(cand_ref.cube_ref(wide, steps, phases, k["nchan"], k["nbins"], k["sub"], k["nsamp"], delays, mask)[0][0, -1, 0]).any()


def test_the_cube_ties_dedispersion_to_folding():
    """integer samples 0 .. 15 and every bin's total below 2^24: every sum is exact, so the cube summed over its channels
    is fold_ref over dedisp_ref's series with the same delays bit for bit, and the hits are equal"""
    nchan, nbins, sub, nsamp = 16, 12, 64, 200
    rng = np.random.default_rng(6)
    steps, phases = fold_ref.table(3, seed=6, first=7.7)
    delays = rng.integers(0, 30, (3, nchan)).astype(np.int32)
    mask = dedisp_ref.random_mask(nchan, 6)
    rows = rng.integers(0, 16, (nsamp + 29, nchan)).astype(np.float32)
    cube, hits = cand_ref.cube_ref(rows, steps, phases, nchan, nbins, sub, nsamp, delays, mask)
    series = dedisp_ref.dedisp_ref(rows, delays, mask, nsamp)                    # [3, nsamp]: trial c is candidate c's delays
    assert series.max() * nsamp < 2 ** 24
    for c in range(3):
        prof, fhits = fold_ref.fold_ref(series[c:c + 1], steps[c:c + 1], phases[c:c + 1], nbins, sub, nsamp)
        total = np.zeros((cube.shape[1], nbins), np.float32)
        for i in range(nchan):
            total = total + cube[c, :, i]
        assert same_bits(total, prof[0, 0]) and np.array_equal(hits[c], fhits[0])


# ---- the host helpers ---------------------------------------------------------------------------------------------

DM_SETS = [(64, 1, 400e6, 100e6, 1e-3, 50.3, 32, 9, -2.0, 0.5), (16, 0, 1420.4e6, 2.0e6, 1e-4, 333.25, 256, 5, -30.0, 15.0),
           (1024, 1, 408e6, 2.4e6, 2048 / 2.4e6, 17.0, 2, 3, 0.0, 0.7), (4, 0, 151e6, 2.4e6, 1e-3, 2.5, 50, 256, -12.8, 0.1)]


@pytest.mark.parametrize("args", DM_SETS)
def test_dm_shifts_against_extended_precision(cand, args):
    got = cand.dm_shifts(*args)
    want, away = cand_ref.reduced(cand_ref.dm_shift_quotients(*args), args[6])
    assert got.dtype == np.int32 and got.shape == (args[7], args[0]) and away.mean() > 0.99
    assert np.array_equal(got[away], want[away]) and got.min() >= 0 and got.max() < args[6]
    top = np.argmax(cand_ref.frequencies_mhz(*args[:4]))
    assert not got[:, top].any()                                             # the highest channel is the reference


def test_dm_shifts_signs(cand):
    """a larger DM delays the low channels: their shift grows with the offset, and a negative offset gives nbins - shift"""
    nchan, nbins = 64, 256
    a = cand.dm_shifts(nchan, 1, 400e6, 100e6, 1e-3, 500.0, nbins, 3, -1.0, 1.0)
    low = np.argmin(cand_ref.frequencies_mhz(nchan, 1, 400e6, 100e6))
    late = float(cand_ref.dm_delay_rows(nchan, 1, 400e6, 100e6, 1e-3, 1.0)[low])
    assert 0 < late < 250 and a[2, low] == round(nbins * late / 500.0) and not a[1].any()
    assert np.array_equal((a[0] + a[2]) % nbins, np.zeros(nchan, np.int32))


DRIFT_SETS = [(32, 256, 16, 9, -2.4e-4, 6.1e-5, 1, 0.0, 0.0), (256, 4096, 32, 129, -1e-5, 1.5625e-7, 3, -1e-10, 1e-10),
              (2, 16, 1024, 4, -0.01, 0.007, 2, 1e-6, -3e-6), (50, 1 << 24, 3, 64, -2e-8, 1e-9, 64, -1e-15, 1e-16)]


@pytest.mark.parametrize("args", DRIFT_SETS)
def test_drift_shifts_against_extended_precision(cand, args):
    got = cand.drift_shifts(*args)
    want, away = cand_ref.reduced(cand_ref.drift_shift_quotients(*args), args[0])
    assert got.dtype == np.int32 and got.shape == (args[3] * args[6], args[2]) and away.mean() > 0.95
    assert np.array_equal(got[away], want[away]) and got.min() >= 0 and got.max() < args[0]


def test_drift_shifts_order_and_signs(cand):
    """r runs the frequency index fastest; a fold faster than the pulsar by df reads df t turns further on, and a derivative
    adds t^2 / 2"""
    nbins, sub, nsub = 100, 1000, 4
    g = cand.drift_shifts(nbins, sub, nsub, 2, 0.0, 1e-4, 2, 0.0, 1e-7)
    t = (np.arange(nsub) + 0.5) * sub
    assert not g[0].any()
    assert np.array_equal(g[1], np.rint(nbins * 1e-4 * t).astype(np.int64) % nbins)
    assert np.array_equal(g[2], np.rint(nbins * 0.5e-7 * t * t).astype(np.int64) % nbins)
    assert np.array_equal(g[3], np.rint(nbins * (1e-4 * t + 0.5e-7 * t * t)).astype(np.int64) % nbins)
    back = cand.drift_shifts(nbins, sub, nsub, 1, -1e-4, 0.0)
    assert np.array_equal((back[0] + g[1]) % nbins, np.zeros(nsub, np.int32))


def test_helper_refusals(cand):
    L = cand.lib()
    buf = (C.c_int32 * (256 * 4096))()
    ok = (64, 1, 400e6, 100e6, 1e-3, 50.3, 32, 9, -2.0, 0.5)
    nan, inf = float("nan"), float("inf")
    for at, value, text in ((0, 3, "nchan"), (0, 6, "nchan"), (0, 4100, "nchan"), (1, 2, "shifted"), (2, nan, "frequency"), (2, 40e6, "frequency"),
                            (3, 0.0, "bandwidth_hz"), (3, inf, "bandwidth_hz"), (4, 0.0, "row_seconds"), (4, nan, "row_seconds"),
                            (5, 0.0, "period_rows"), (5, -3.0, "period_rows"), (5, inf, "period_rows"), (6, 1, "nbins"), (6, 257, "nbins"),
                            (7, 0, "ndm"), (7, 257, "ndm"), (8, nan, "DM offsets"), (9, inf, "DM offsets"), (5, 1e-9, "2^31")):
        args = list(ok)
        args[at] = value
        assert L.rtlws_cand_dm_shifts(*args, buf) == -1 and text in cand.last_error(), (at, value, cand.last_error())
        with pytest.raises(ValueError):
            cand.dm_shifts(*args)
    assert L.rtlws_cand_dm_shifts(*ok, None) == -1 and "null table" in cand.last_error()
    assert L.rtlws_cand_dm_shifts(*ok, buf) == 0 and cand.last_error() == ""
    ok = (32, 256, 16, 9, -1e-4, 2.5e-5, 2, 0.0, 1e-9)
    for at, value, text in ((0, 1, "nbins"), (0, 257, "nbins"), (1, 15, "sub"), (1, (1 << 24) + 1, "sub"), (2, 0, "nsub"), (2, 1025, "nsub"),
                            (3, 0, "nf"), (6, 0, "nf"), (3, 2049, "nf"), (4, nan, "finite"), (5, inf, "finite"), (7, nan, "finite"),
                            (8, -inf, "finite"), (4, 1e6, "2^31")):
        args = list(ok)
        args[at] = value
        assert L.rtlws_cand_drift_shifts(*args, buf) == -1 and text in cand.last_error(), (at, value, cand.last_error())
    assert L.rtlws_cand_drift_shifts(*ok, None) == -1 and "null table" in cand.last_error()
    assert L.rtlws_cand_drift_shifts(32, 256, 16, 64, 0.0, 1e-6, 64, 0.0, 1e-9, buf) == 0 and cand.last_error() == ""
    with pytest.raises(ValueError):
        cand.drift_shifts(32, 256, 16, 0, 0.0, 1e-6)


def test_chi2(cand):
    for stat, total, nbins, var in ((1234.5, 60.25, 32, 3.5), (7.0, -2.0, 2, 0.125), (1e12, 1e5, 256, 900.0)):
        assert cand.chi2(stat, total, nbins, var) == cand_ref.chi2(stat, total, nbins, var)
    assert cand.chi2(8.0, 4.0, 2, 1.0) == 0.0                                   # a flat profile
    for bad in ((1.0, 1.0, 1, 1.0), (1.0, 1.0, 0, 1.0), (1.0, 1.0, 8, 0.0), (1.0, 1.0, 8, -1.0), (1.0, 1.0, 8, float("nan"))):
        assert math.isnan(cand.chi2(*bad)) and math.isnan(cand_ref.chi2(*bad))


def planted_search(cand, fold):
    """the synthetic pulsar folded a little off in DM and in frequency by fold(rows, steps, phases, nchan, nbins, sub, nsamp,
    delays) and searched over the helpers' grids -> (stat [ndm, ntr], q_true, r_true, search_ref's arguments)"""
    p = cand_ref.PULSAR
    band = (p["nchan"], p["shifted"], p["f_centre_hz"], p["bandwidth_hz"], p["row_seconds"])
    delays = dedisp_ref.delays(*band, 1, p["dm_fold"], 0.0)
    rows, step = cand_ref.pulsar_rows(delays)
    cube = fold(rows, [step], [0], p["nchan"], p["nbins"], p["sub"], p["nsamp"], delays)
    a = cand.dm_shifts(*band, p["period"], p["nbins"], p["ndm"], p["ddm0"], p["ddm_step"])
    g = cand.drift_shifts(p["nbins"], p["sub"], cube.shape[1], p["nf"], p["df0"], p["df_step"])
    return cube, a[None], g[None]


def test_the_planted_offsets_are_the_strict_maximum(cand):
    """the helpers' sign conventions: a pulsar folded at a slightly wrong (DM, f) in the restatement comes out at the
    planted offsets' (q, r), the strict maximum of stat, and nowhere else"""
    p = cand_ref.PULSAR
    cube, a, g = planted_search(cand, lambda *args: cand_ref.cube_ref(*args)[0])
    stat, total, P, T = cand_ref.search_ref(cube, a, g)
    assert stat.shape == (1, p["ndm"], p["nf"])
    best = np.unravel_index(np.argmax(stat[0]), stat[0].shape)
    assert best == (p["q_true"], p["r_true"]) and (stat[0] == stat[0].max()).sum() == 1
    # the zero offsets (the fold's own DM and frequency) see a smeared pulse
    q0, r0 = int(round(-p["ddm0"] / p["ddm_step"])), int(round(-p["df0"] / p["df_step"]))
    assert not a[0, q0].any() and not g[0, r0].any() and stat[0, q0, r0] < 0.8 * stat[0].max()
    var = p["nchan"] * p["nsamp"] / p["nbins"]                                   # unit noise: a bin of P adds nchan * nsamp / nbins samples
    assert cand.chi2(stat[0][best], total[0][best], p["nbins"], var) > 20.0


# ---- the library without a GPU ------------------------------------------------------------------------------------

def test_exports_are_the_header(cand):
    import test_abi_cpu
    declared = test_abi_cpu._declared_functions("rtlws_cand.h")
    assert len(declared) == 15 and set(declared) == set(cand.SYMBOLS)
    assert test_abi_cpu._exported(cand.CAND_LIB) == set(declared)
    L = cand.lib()
    assert all(getattr(L, f).argtypes is not None for f in cand.SYMBOLS)


def test_the_header_is_strict_c99(tmp_path):
    src = tmp_path / "t_rtlws_cand.c"
    src.write_text('#include "rtlws_cand.h"\nint main(void) { return rtlws_cand_fold_supported(1, 4, 2, 16) ? 0 : 1; }\n')
    out = subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Wextra", "-Werror", "-I", INCLUDE, "-c", str(src), "-o", os.devnull],
                         capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    code = re.sub(r"/\*.*?\*/", "", open(os.path.join(INCLUDE, "rtlws_cand.h")).read(), flags=re.S)
    assert "hipStream_t" not in code and "hipError_t" not in code
    for name, value in (("MAX_CANDS", 64), ("MIN_NCHAN", 4), ("MAX_NCHAN", 4096), ("MAX_DELAY", 65535), ("MIN_BINS", 2), ("MAX_BINS", 256),
                        ("MIN_SUB", 16), ("MAX_SUB", 1 << 24), ("MAX_NSAMP", 1 << 30), ("MAX_NSUB", 1024), ("MAX_NDM", 256), ("MAX_NTR", 4096),
                        ("MAX_WORKSPACE", 1 << 30)):
        assert re.search(r"#define RTLWS_CAND_%s %d\b" % (name, value), code) and getattr(cand_ref, name) == value, name


# (ncand, nchan, nbins, sub) -> the refusal, None when served
FOLD_LIMITS = [
    ((0, 4, 2, 16), "ncand must be 1 .. 64"), ((1, 4, 2, 16), None), ((64, 4096, 256, 1 << 24), None), ((65, 4, 2, 16), "ncand must be 1 .. 64"),
    ((1, 0, 2, 16), "nchan must be 4 .. 4096 and a multiple of 4"), ((1, 6, 2, 16), "nchan must be 4 .. 4096 and a multiple of 4"),
    ((1, 4100, 2, 16), "nchan must be 4 .. 4096 and a multiple of 4"), ((1, 4096, 2, 16), None),
    ((1, 4, 1, 16), "nbins must be 2 .. 256"), ((1, 4, 257, 16), "nbins must be 2 .. 256"), ((1, 4, 256, 16), None),
    ((1, 4, 2, 15), "sub must be 16 .. 16777216"), ((1, 4, 2, (1 << 24) + 1), "sub must be 16 .. 16777216"), ((1, 4, 2, 17), None),
    ((0, 0, 0, 0), "ncand must be 1 .. 64"), ((1, 0, 0, 0), "nchan must be 4 .. 4096 and a multiple of 4"), ((1, 4, 0, 0), "nbins must be 2 .. 256"),
]
# (ncand, nsub, nchan, nbins, ndm, ntr)
SEARCH_LIMITS = [
    ((1, 1, 4, 2, 1, 1), None), ((64, 1024, 4096, 4, 256, 4096), None), ((0, 1, 4, 2, 1, 1), "ncand must be 1 .. 64"),
    ((65, 1, 4, 2, 1, 1), "ncand must be 1 .. 64"), ((1, 0, 4, 2, 1, 1), "nsub must be 1 .. 1024"), ((1, 1025, 4, 2, 1, 1), "nsub must be 1 .. 1024"),
    ((1, 1, 2, 2, 1, 1), "nchan must be 4 .. 4096 and a multiple of 4"), ((1, 1, 4098, 2, 1, 1), "nchan must be 4 .. 4096 and a multiple of 4"),
    ((1, 1, 4, 1, 1, 1), "nbins must be 2 .. 256"), ((1, 1, 4, 257, 1, 1), "nbins must be 2 .. 256"),
    ((1, 1, 4, 2, 0, 1), "ndm must be 1 .. 256"), ((1, 1, 4, 2, 257, 1), "ndm must be 1 .. 256"),
    ((1, 1, 4, 2, 1, 0), "ntr must be 1 .. 4096"), ((1, 1, 4, 2, 1, 4097), "ntr must be 1 .. 4096"),
    ((64, 1024, 4, 65, 256, 1), "a workspace above 2^30 bytes"), ((16, 1024, 4, 256, 256, 1), "a workspace above 2^30 bytes"),
    ((4, 1024, 4, 256, 256, 1), None), ((0, 0, 0, 0, 0, 0), "ncand must be 1 .. 64"),
]


def test_the_rules_at_every_limit(cand):
    for args, why in FOLD_LIMITS:
        assert bool(cand.fold_supported(*args)) == (why is None), args
        assert cand.last_error() == ("" if why is None else "rtlws_cand_fold: " + why), (args, cand.last_error())
        got = cand.fold_geometry(*args, nsamp=100)
        assert (got[0] == 0) == (why is None), args
        if why is None:
            assert got[1:] == cand_ref.fold_plan(*args, 100), args
        else:
            assert cand.last_error() == "rtlws_cand_fold_geometry: " + why
    for args, why in SEARCH_LIMITS:
        assert bool(cand.search_supported(*args)) == (why is None), args
        assert cand.last_error() == ("" if why is None else "rtlws_cand_search: " + why), (args, cand.last_error())
        got = cand.search_geometry(*args)
        assert (got[0] == 0) == (why is None), args
        if why is None:
            assert got[1:] == cand_ref.search_plan(*args), args
    assert cand.lib().rtlws_cand_fold_geometry(1, 4, 2, 16, 100, None, None, None, None, None) == 0
    assert cand.lib().rtlws_cand_search_geometry(1, 1, 4, 2, 1, 1, None, None, None, None, None, None) == 0


def test_geometry_is_the_stated_rule(cand):
    """the channel groups and wavefronts per workgroup across the bin counts' steps, nsamp at its ends, the grid's limit"""
    for nbins, wpb in ((2, 4), (64, 4), (65, 2), (128, 2), (129, 1), (256, 1)):
        for nchan in (4, 64, 68, 132, 256, 260, 4096):
            rc, blocks, threads, lds, waves, nsub = cand.fold_geometry(3, nchan, nbins, 100, 1030)
            assert (rc, threads, lds, waves, nsub) == (0, 64 * wpb, wpb * nbins * 256, wpb, 11) and lds <= 65536
            assert blocks == 3 * 11 * -(-nchan // (64 * wpb)) == cand_ref.fold_plan(3, nchan, nbins, 100, 1030)[0]
    assert cand.fold_geometry(1, 4, 2, 16, 0)[1:] == (0, 256, 2048, 4, 0)
    assert cand.fold_geometry(1, 4, 2, 100, 99)[5] == 1 and cand.fold_geometry(1, 4, 2, 100, 101)[5] == 2
    for nsamp in (-1, (1 << 30) + 1):
        assert cand.fold_geometry(1, 4, 2, 16, nsamp)[0] == -1 and cand.last_error() == "rtlws_cand_fold_geometry: nsamp must be 0 .. 2^30"
    # 2^26 sub-integrations of 64 candidates over 64 channel groups: 2^38 workgroups
    assert cand.fold_geometry(64, 4096, 256, 16, 1 << 30)[0] == -1 and "more workgroups than one grid holds" in cand.last_error()
    assert cand.fold_geometry(1, 64, 256, 16, 1 << 30)[:2] == (0, 1 << 26)
    assert cand.fold_geometry(32, 64, 256, 16, 1 << 30)[0] == -1 and cand.fold_geometry(31, 64, 256, 16, 1 << 30)[:2] == (0, 31 << 26)
    for nbins in (2, 64, 65, 256):
        rc, b1, b2, threads, lds1, lds2, work = cand.search_geometry(3, 17, 68, nbins, 33, 65)
        assert (rc, b1, b2, threads, lds1, lds2, work) == (0, 3 * 17 * 5, 3 * 33 * 9, 512, 128 * nbins, 160 * nbins, 3 * 33 * 17 * nbins * 4)


def test_open_without_an_engine(cand):
    steps, phases = np.array([5], np.uint64), np.array([0], np.uint64)
    with pytest.raises(RuntimeError, match="rtlws_cand_fold_open: null engine"):
        cand.CandFoldPlan(None, steps, phases, 4, 2, 16)
    for kwargs, text in ((dict(nchan=6), "nchan must be 4 .. 4096"), (dict(nbins=1), "nbins must be 2 .. 256"), (dict(sub=8), "sub must be 16"),
                         (dict(ncand=0), "ncand must be 1 .. 64"), (dict(steps=None, ncand=1), "null steps"), (dict(phases=None), "null phases"),
                         (dict(delays=[0, 1, 65536, 2]), "a delay outside 0 .. 65535"), (dict(delays=[0, -1, 3, 2]), "a delay outside 0 .. 65535"),
                         (dict(delays=[0, 65536, 3, 2], mask=[1, 0, 1, 1]), "a delay outside 0 .. 65535")):
        args = dict(steps=steps, phases=phases, nchan=4, nbins=2, sub=16)
        args.update(kwargs)
        with pytest.raises(RuntimeError, match="rtlws_cand_fold_open: " + text):                  # the arguments come before the engine
            cand.CandFoldPlan(None, **args)
    a, g = np.zeros((1, 1, 4), np.int32), np.zeros((1, 1, 3), np.int32)
    with pytest.raises(RuntimeError, match="rtlws_cand_search_open: null engine"):
        cand.CandSearchPlan(None, 1, 3, 4, 2, a, g)
    for kwargs, text in ((dict(nsub=0), "nsub must be 1 .. 1024"), (dict(a=None, ndm=1), "null a"), (dict(g=None, ntr=1), "null g"),
                         (dict(a=[[[0, 2, 0, 0]]]), "an entry of a outside 0 .. nbins - 1"), (dict(a=[[[0, -1, 0, 0]]]), "an entry of a outside"),
                         (dict(g=[[[0, 0, 2]]]), "an entry of g outside 0 .. nbins - 1"), (dict(a=np.zeros((1, 300, 4), np.int32)), "ndm must be 1 .. 256")):
        args = dict(ncand=1, nsub=3, nchan=4, nbins=2, a=a, g=g)
        args.update(kwargs)
        with pytest.raises(RuntimeError, match="rtlws_cand_search_open: " + text):
            cand.CandSearchPlan(None, **args)
    L = cand.lib()
    assert L.rtlws_cand_fold_rows_needed(None, 1) == -1 and "null plan" in cand.last_error()
    assert L.rtlws_cand_fold_rows_needed(None, -1) == -1 and "nsamp must be 0 .. 2^30" in cand.last_error()
    L.rtlws_cand_fold_close(None)
    L.rtlws_cand_search_close(None)
    # a run's refusals that need no plan come before the null plan's, in the header's order: (d_rows, in_stride, nsamp, d_cube, d_hits)
    run = lambda *args: L.rtlws_cand_fold_run(None, *args, None)
    for args, text in (((64, 4, -1, 64, None), "nsamp must be 0 .. 2^30"), ((64, 4, (1 << 30) + 1, 64, None), "nsamp must be 0 .. 2^30"),
                       ((64, 0, 1, 64, None), "in_stride must be >= 4 and a multiple of 4"), ((64, 6, 1, 64, None), "in_stride must be >= 4"),
                       ((None, 4, 1, 64, None), "null pointer"), ((64, 4, 1, None, None), "null pointer"),
                       ((72, 4, 1, 64, None), "d_rows must be 16-byte aligned"), ((64, 4, 1, 66, None), "d_cube must be 4-byte aligned"),
                       ((64, 4, 1, 64, 66), "d_hits must be 4-byte aligned"), ((64, 4, 1, 68, 68), "null plan"), ((64, 4, 0, 64, None), "null plan")):
        assert run(*args) == -1 and text in cand.last_error(), (args, cand.last_error())
    # (d_cube, d_stat, d_total, d_prof, d_tphase)
    run = lambda *args: L.rtlws_cand_search_run(None, *args, None)
    for args, text in (((None, 64, 64, None, None), "null pointer"), ((64, None, 64, None, None), "null pointer"), ((64, 64, None, None, None), "null pointer"),
                       ((66, 64, 64, None, None), "d_cube must be 4-byte aligned"), ((64, 68, 64, None, None), "d_stat must be 8-byte aligned"),
                       ((64, 64, 68, None, None), "d_total must be 8-byte aligned"), ((64, 64, 64, 66, None), "d_prof must be 4-byte aligned"),
                       ((64, 64, 64, 68, 66), "d_tphase must be 4-byte aligned"), ((68, 64, 64, 68, 68), "null plan")):
        assert run(*args) == -1 and text in cand.last_error(), (args, cand.last_error())


def test_the_pinned_surface_holds_with_the_submodule(built, cand):
    """tests/test_python_api_cpu.py's snapshot with rtlws.cand imported: no new public name, no new Engine method, the
    plans no _Plan subclasses"""
    import test_python_api_cpu as api
    rec, now = api._recorded(), api.snapshot(built)
    assert built.cand is cand
    for part in ("names", "functions", "methods"):
        assert now[part] == rec[part], part
    for plan in (cand.CandFoldPlan, cand.CandSearchPlan):
        assert not issubclass(plan, built._Plan) and issubclass(plan, built._PlanBase)
    assert "cand" not in api.SATELLITES
    assert "librtlws_cand.so (include/rtlws_cand.h)" in cand.lib.__doc__
    assert {"fold_supported", "fold_geometry", "search_supported", "search_geometry", "dm_shifts", "drift_shifts", "chi2", "fold", "search",
            "CandFoldPlan", "CandSearchPlan", "GUARD"} <= set(vars(cand))


def test_the_new_sources_carry_no_conditionals():
    for path in NEW_SOURCES:
        lines = [ln.strip() for ln in open(path) if re.match(r"\s*#", ln)]
        other = [ln for ln in lines if not re.match(r"#\s*(include|pragma|define)\b", ln)]
        guards = [ln for ln in other if re.match(r"#\s*(ifndef RTLWS_\w+_H|endif\b|ifdef __cplusplus)", ln)]
        assert other == guards, (path, [ln for ln in other if ln not in guards])
        assert sum(ln.startswith("#ifndef") for ln in lines) == (0 if path.endswith(".hip") else 1), path


def test_no_kernel_of_the_library_spills(built, cand):
    """the code object's metadata: three kernels of the cube (one per wavefronts-per-workgroup) and eight of the stages
    (bins per lane 1 .. 4, with and without the sums); no spill, no scratch, no static LDS: what geometry reports is all
    the LDS a workgroup has, and it stays within 64 KiB"""
    from rtlws import codeobj
    mine = codeobj.kernels(cand.CAND_LIB)
    assert len([k for k in mine if "cand_fold_kernel" in k["name"]]) == 3 and len([k for k in mine if "cand_stage_kernel" in k["name"]]) == 8
    assert len(mine) == 11
    for k in mine:
        assert not k["vgpr_spill_count"] and not k.get("sgpr_spill_count", 0) and not k["private_segment_fixed_size"], k["name"]
        assert k["vgpr_count"] <= 128 and k.get("agpr_count", 0) == 0, k["name"]
        assert k["group_segment_fixed_size"] == 0, k["name"]
    assert max(cand.fold_geometry(1, 4, nbins, 16)[3] for nbins in range(2, 257)) == 65536
    assert max(cand.search_geometry(1, 1, 4, nbins, 1, 1)[5] for nbins in range(2, 257)) == 40960


def test_the_makefile_builds_it():
    txt = open(os.path.join(ROOT, "rtl-ws_amd", "Makefile")).read()
    assert re.search(r"^SATELLITES := .*\bcand\b", txt, flags=re.M)
    assert re.search(r"^\$\(eval \$\(call SATELLITE,cand,cand cand_shim,", txt, flags=re.M)
    out = subprocess.run(["nm", "-D", "--undefined-only", os.path.join(ROOT, "rtl-ws_amd", "lib", "librtlws_cand.so")],
                         capture_output=True, text=True, check=True).stdout
    assert "rtlws_engine_device" in out and "rtlws_engine_stream" in out          # the engine is librtlws_hip.so's

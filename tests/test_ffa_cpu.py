"""CPU suite of include/rtlws_ffa.h: the restatement's own properties (tests/ffa_ref.py: the passes against the one-go
transform, where a delta lands, row 0, the peaks against the header's loop), and what the library does without a GPU:
its exports, the rules and the geometry at every limit, the host helpers, the binding's place beside the pinned surface,
the new sources' preprocessor lines and the kernels' registers."""
import math
import os
import re
import subprocess

import numpy as np
import pytest

import ffa_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "rtl-ws_amd", "csrc")
NEW_SOURCES = [os.path.join(CSRC, f) for f in ("ffa.h", "ffa.hip", "ffa_shim.hip", "search_plan.h")] + [os.path.join(ROOT, "include", "rtlws_ffa.h")]


@pytest.fixture(scope="module")
def ffa(built):
    import rtlws.ffa
    return rtlws.ffa


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


# ---- the restatement ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("p", [16, 17, 23])
def test_the_passes_are_the_transform(p):
    """every split of L = 1 .. 6 into passes, done as the pass kernel does them, gives the one-go transform's bits"""
    for L in range(1, 7):
        x = ffa_ref.signed_series(2, (p << L) + 3, seed=10 * p + L)
        whole = ffa_ref.ffa(x, p, L)
        assert whole.shape == (2, 1 << L, p)
        splits = ffa_ref.splits_of(L)
        assert len(splits) == 1 << (L - 1)
        for stages in splits:
            assert np.array_equal(_bits(ffa_ref.ffa_passes(x, p, L, stages)), _bits(whole)), (p, L, stages)


def test_where_a_delta_lands():
    """a delta in row r, column c0 reaches row s of the output once, at column c0 - sigma(r, s); the last row's shift is
    s itself, so that row s folds at p + s / (m - 1)"""
    L, p, c0 = 4, 17, 3
    m = 1 << L
    for r in range(m):
        x = np.zeros((1, m * p), np.float32)
        x[0, r * p + c0] = 1.0
        out = ffa_ref.ffa(x, p, L)[0]
        for s in range(m):
            assert np.argwhere(out[s])[:, 0].tolist() == [(c0 - ffa_ref.sigma(r, s, L)) % p], (r, s)
    for L in range(1, 13):
        assert all(ffa_ref.sigma((1 << L) - 1, s, L) == s for s in range(1 << L))
        assert all(ffa_ref.sigma(0, s, L) == 0 for s in range(1 << L))


def test_row_zero_is_the_balanced_column_sum():
    p, L = 19, 5
    x = ffa_ref.signed_series(1, p << L, seed=5)
    rows = ffa_ref.rows_of(x, p, 1 << L)[0]
    while rows.shape[0] > 1:                                     # neighbours first: stage 1 adds rows 2k and 2k + 1
        rows = rows[0::2] + rows[1::2]
    assert np.array_equal(_bits(ffa_ref.ffa(x, p, L)[0, 0]), _bits(rows[0]))
    sequential = np.zeros(p, np.float32)
    for r in ffa_ref.rows_of(x, p, 1 << L)[0]:
        sequential = sequential + r
    assert not np.array_equal(_bits(sequential), _bits(rows[0]))          # the order is part of the definition


def test_the_peaks_are_the_headers_loop():
    rng = np.random.default_rng(3)
    b = ffa_ref.signed_series(1, 16 * 21, seed=4).reshape(16, 21)
    b[2, 3], b[9, 0] = np.nan, np.nan
    b[4, 5] = b[5, 1] = np.float32(1.0e6)                        # a tie across rows: the first wins
    b[12:14] = np.nan                                            # a segment of NaN only
    b[14:16] = -np.inf
    b[rng.integers(0, 12, 20), rng.integers(0, 21, 20)] = 0.0
    for seg in (1, 2, 4, 16):
        peak, at = ffa_ref.peaks(b[None], seg)
        want_peak, want_at = ffa_ref.peaks_by_the_letter(b, seg)
        assert np.array_equal(at[0], want_at) and np.array_equal(_bits(peak[0]), _bits(want_peak)), seg
    peak, at = ffa_ref.peaks(b[None], 2)
    assert at[0, 2] == 4 * 21 + 5 and at[0, 6] == -1 and at[0, 7] == -1 and peak[0, 6] == -np.inf


def test_the_circular_boxcar():
    """B_w of a row: rtlws_pulse.h's combination over the row repeated, so the same bits as the linear one there"""
    import pulse_ref
    p = 37
    row = ffa_ref.signed_series(1, p, seed=8)
    twice = np.concatenate([row, row], axis=1)
    for w in (1, 2, 3, 5, 8, 13, 31, 32, 37):
        assert np.array_equal(_bits(ffa_ref.boxcar(row, w)), _bits(pulse_ref.boxcar(twice, w)[:, :p])), w


# ---- the library without a GPU ------------------------------------------------------------------------------------

def test_exports_are_the_header(ffa):
    import test_abi_cpu
    declared = test_abi_cpu._declared_functions("rtlws_ffa.h")
    assert len(declared) == 10 and set(declared) == set(ffa.SYMBOLS)
    assert test_abi_cpu._exported(ffa.FFA_LIB) == set(declared)
    L = ffa.lib()
    assert all(getattr(L, f).argtypes is not None for f in ffa.SYMBOLS)


LADDER16 = (1, 2, 3, 4, 6, 8, 12, 16, 24, 32, 48, 64, 96, 128, 255, 256)
# (p0, nper, L, widths, seg) -> served
LIMITS = [
    ((16, 1, 1, (1,), 1), True), ((15, 1, 1, (1,), 1), False),
    ((16, 0, 1, (1,), 1), False),
    ((1024, 1, 12, (1,), 1), True), ((1025, 1, 2, (1,), 1), False), ((1000, 25, 2, (1,), 1), True), ((1000, 26, 2, (1,), 1), False),
    ((16, 1, 0, (1,), 1), False), ((16, 1, 12, (1,), 1), True), ((16, 1, 13, (1,), 1), False),
    # m * p_max = 2^22 is the two limits met at once: above it lies only p_max = 1025 or L = 13
    ((1024, 1, 12, (1,), 4096), True), ((512, 513, 12, (1,), 1), True), ((1024, 2, 12, (1,), 1), False), ((512, 514, 12, (1,), 1), False),
    ((1024, 1, 13, (1,), 1), False),
    ((16, 1, 1, (16,), 1), True), ((16, 1, 1, (17,), 1), False), ((300, 1, 1, (256,), 1), True), ((300, 1, 1, (257,), 1), False),
    ((16, 1, 1, (0,), 1), False), ((16, 1, 1, (), 1), False), ((16, 1, 1, None, 1), False),
    ((300, 1, 1, LADDER16, 1), True), ((300, 1, 1, LADDER16[:-1] + (255,), 1), False), ((300, 1, 1, (1,) + LADDER16, 1), False),
    ((16, 1, 1, (2, 1), 1), False), ((16, 1, 1, (2, 2), 1), False),
    ((16, 1, 4, (1,), 16), True), ((16, 1, 4, (1,), 32), False), ((16, 1, 4, (1,), 3), False), ((16, 1, 4, (1,), 0), False),
    ((16, 1, 4, (1,), -4), False),
]


def test_the_rules_at_every_limit(ffa):
    for args, served in LIMITS:
        assert bool(ffa.supported(*args)) == served, args
        assert bool(ffa.last_error()) == (not served), args
        assert ffa_ref.supported(*args) == served, args
        got = ffa.geometry(*args, max_trials=2)
        assert (got[0] == 0) == served, args
        if served:
            assert got[1:] == ffa_ref.plan(*args, max_trials=2), args
    assert ffa.geometry(16, 1, 1, (1,), 1, max_trials=0)[0] == -1 and "max_trials" in ffa.last_error()
    assert ffa.supported(15, 1, 1, (1,), 1) == 0 and ffa.last_error() == "rtlws_ffa: p0 must be >= 16"


def test_the_geometry_of_every_plan(ffa):
    """every L at the pitches where the tile changes: the stages add to L and are dealt evenly over as few passes as fit,
    the LDS stays inside 160 KiB, the workspace inside its cap, and the pairs in flight are what the cap holds"""
    seen = set()
    for p_max in (16, 17, 79, 80, 159, 160, 319, 320, 639, 640, 1024):
        for L in range(1, 13):
            if (p_max << L) > ffa_ref.MAX_CELLS:
                continue
            for widths, seg in (((1,), 1), ((1, min(256, p_max)), 1 << L), (LADDER16[:10], 1 << (L // 2))):
                if max(widths) > p_max:
                    continue
                rc, passes, stages, blocks, threads, lds, merge, ws, pairs = ffa.geometry(p_max, 1, L, widths, seg, max_trials=70000)
                assert rc == 0 and (passes, stages, blocks, threads, lds, merge, ws, pairs) == ffa_ref.plan(p_max, 1, L, widths, seg, 70000)
                assert sum(stages) == L and all(n >= 1 for n in stages[:passes]) and not any(stages[passes:])
                assert passes == -(-L // ffa_ref.max_stages(p_max)) and max(stages) - min(stages[:passes]) <= 1
                assert all(0 < b <= 160 * 1024 for b in lds[:passes]) and threads == 512
                assert blocks[:passes] == tuple((1 << L) >> n for n in stages[:passes])
                assert merge == int(seg > (1 << stages[passes - 1]))
                assert 1 <= pairs <= 65535 and ws <= ffa.WORKSPACE_CAP and (ws == 0) == (passes == 1 and not merge)
                seen.add(passes)
    assert seen == {1, 2, 3}
    assert ffa_ref.max_stages(1024) == 4 and ffa_ref.max_stages(16) == 7
    # the pairs in flight: what the caller expects, else what the cap holds
    assert ffa.geometry(1024, 1, 12, (1,), 1, max_trials=3)[-1] == 3
    rc, *_, ws, pairs = ffa.geometry(1024, 1, 12, (1,), 1, max_trials=1000)
    assert pairs == ffa.WORKSPACE_CAP // (2 << 24) == 32 and ws == 1 << 30


def test_open_without_an_engine(ffa):
    with pytest.raises(RuntimeError, match="rtlws_ffa_open: null engine"):
        ffa.FfaPlan(None, 16, 2, 3, (1, 3), 1)
    with pytest.raises(RuntimeError, match="rtlws_ffa_open: p0 must be >= 16"):       # the arguments come first
        ffa.FfaPlan(None, 15, 2, 3, (1, 3), 1)
    L = ffa.lib()
    assert L.rtlws_ffa_samples_needed(None) == -1 and "null plan" in ffa.last_error()
    assert L.rtlws_ffa_workspace_bytes(None) == 0
    L.rtlws_ffa_close(None)
    # a run's refusals that need no plan come before the null plan's, in the header's order
    run = lambda *a: L.rtlws_ffa_run(None, *a, None)
    for args, text in (((64, 8, 0, 64, 64, None, 0), "ntrials"), ((64, 8, 65537, 64, 64, None, 0), "ntrials"),
                       ((64, 6, 1, 64, 64, None, 0), "in_stride must be a multiple of 4"), ((None, 8, 1, 64, 64, None, 0), "null pointer"),
                       ((64, 8, 1, None, 64, None, 0), "null pointer"), ((64, 8, 1, 64, None, None, 0), "null pointer"),
                       ((72, 8, 1, 64, 64, None, 0), "d_in must be 16-byte aligned"), ((64, 8, 1, 66, 64, None, 0), "d_peak must be 4-byte aligned"),
                       ((64, 8, 1, 64, 65, None, 0), "d_at must be 4-byte aligned"), ((64, 8, 1, 64, 64, 67, 0), "d_prof must be 4-byte aligned"),
                       ((64, 8, 1, 64, 64, 64, 0), "null plan")):
        assert run(*args) == -1 and text in ffa.last_error(), (args, ffa.last_error())


def _ulps(a, b):
    if a == b:
        return 0.0
    return abs(a - b) / math.ulp(max(abs(a), abs(b)))


def test_the_host_helpers(ffa):
    """rtlws_ffa_period and rtlws_ffa_snr against the same expressions in Python doubles: division and square root are
    correctly rounded on both sides, so 2 ulp covers a contracted multiply-add and nothing else"""
    for p, s, L in ((16, 0, 1), (16, 1, 1), (250, 77, 7), (1024, 4095, 12), (1000, 1, 12), (33, 6, 3)):
        want = float(p) + float(s) / float((1 << L) - 1)
        assert _ulps(ffa.period(p, s, L), want) <= 2 and _ulps(ffa_ref.period(p, s, L), want) == 0, (p, s, L)
    assert ffa.period(250, 127, 7) == 251.0 and ffa.period(16, 0, 5) == 16.0
    for args in ((0, 0, 3), (16, -1, 3), (16, 8, 3), (16, 0, 0), (16, 0, 13)):
        assert math.isnan(ffa.period(*args)), args
    rng = np.random.default_rng(9)
    for _ in range(200):
        peak, width, rows = float(rng.normal(50.0, 30.0)), int(rng.integers(1, 257)), int(1 << rng.integers(0, 13))
        count = int(rng.integers(2, 1 << 22))
        mean, sd = float(rng.normal(0.0, 3.0)), float(rng.uniform(0.1, 5.0))
        sum1, sum2 = mean * count, (sd * sd + mean * mean) * count
        m = sum1 / float(count)
        var = sum2 / float(count) - m * m
        n = float(width) * float(rows)
        want = (peak - n * m) / math.sqrt(n * var)
        got = ffa.snr(peak, width, rows, sum1, sum2, count)
        assert var > 0 and _ulps(got, want) <= 2, (peak, width, rows, got, want)
        assert _ulps(ffa_ref.snr(peak, width, rows, sum1, sum2, count), want) <= 2
    for args in ((1.0, 1, 1, 0.0, 1.0, 1), (1.0, 0, 1, 0.0, 4.0, 4), (1.0, 1, 0, 0.0, 4.0, 4), (1.0, 1, 1, 8.0, 16.0, 4), (1.0, 1, 1, 8.0, 15.0, 4)):
        assert math.isnan(ffa.snr(*args)) and np.isnan(ffa_ref.snr(*args)), args
    assert ffa.snr(10.0, 1, 1, 0.0, 4.0, 4) == 10.0 and ffa.snr(20.0, 2, 2, 0.0, 4.0, 4) == 10.0


def test_the_pinned_surface_holds_with_the_submodule(built, ffa):
    """tests/test_python_api_cpu.py's snapshot with rtlws.ffa imported: no new public name, no new Engine method, FfaPlan
    no _Plan subclass"""
    import test_python_api_cpu as api
    rec, now = api._recorded(), api.snapshot(built)
    assert built.ffa is ffa
    for part in ("names", "functions", "methods"):
        assert now[part] == rec[part], part
    assert not issubclass(ffa.FfaPlan, built._Plan) and issubclass(ffa.FfaPlan, built._PlanBase) and issubclass(built._Plan, built._PlanBase)
    assert "ffa" not in api.SATELLITES and len(now["methods"]["Engine"]) == 37
    assert "librtlws_ffa.so (include/rtlws_ffa.h)" in ffa.lib.__doc__
    assert {"supported", "geometry", "period", "snr", "search", "FfaPlan"} <= set(vars(ffa))


def test_the_new_sources_carry_no_conditionals():
    for path in NEW_SOURCES:
        lines = [ln.strip() for ln in open(path) if re.match(r"\s*#", ln)]
        other = [ln for ln in lines if not re.match(r"#\s*(include|pragma|define)\b", ln)]
        guards = [ln for ln in other if re.match(r"#\s*(ifndef RTLWS_\w+_H|endif\b|ifdef __cplusplus)", ln)]
        assert other == guards, (path, [ln for ln in other if ln not in guards])
        assert sum(ln.startswith("#ifndef") for ln in lines) == (0 if path.endswith(".hip") else 1), path


def test_no_kernel_of_the_library_spills(built, ffa):
    """the code object's metadata, as tests/test_abi_cpu.py reads librtlws_hip.so's: the two pass kernels and the merge,
    no spill, no scratch, and the pass kernels inside the 128 registers of their 512 threads"""
    from rtlws import codeobj
    ks = [k for k in codeobj.kernels(ffa.FFA_LIB)]
    mine = [k for k in ks if "ffa_" in k["name"]]
    assert len(mine) == 3 and sum("ffa_pass" in k["name"] for k in mine) == 2
    for k in mine:
        assert not k["vgpr_spill_count"] and not k.get("sgpr_spill_count", 0) and not k["private_segment_fixed_size"], k["name"]
        assert k["vgpr_count"] <= 128, k["name"]


def test_the_makefile_builds_it():
    txt = open(os.path.join(ROOT, "rtl-ws_amd", "Makefile")).read()
    assert re.search(r"^SATELLITES := .*\bffa\b", txt, flags=re.M)
    out = subprocess.run(["nm", "-D", "--undefined-only", os.path.join(ROOT, "rtl-ws_amd", "lib", "librtlws_ffa.so")],
                         capture_output=True, text=True, check=True).stdout
    assert "rtlws_engine_device" in out and "rtlws_engine_stream" in out          # the engine is librtlws_hip.so's

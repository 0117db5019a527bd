"""CPU suite of include/rtlws_cutout.h: the restatement's own properties (tests/cutout_ref.py against an independent f64
sum within the bound of one rounding an addition, its two ties to the dedispersion, the window at its borders), and what
the library does without a GPU: its exports and prototypes, the header as strict C99, every refusal in its order, the
geometry against the stated rule, rtlws_cutout_window against the restatement, the binding's place beside the pinned
surface, the Makefile's entries, the kernels' registers and LDS."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import cutout_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "rtl-ws_amd", "csrc")
INCLUDE = os.path.join(ROOT, "include")
NEW_SOURCES = [os.path.join(CSRC, f) for f in ("cutout.h", "cutout.hip", "cutout_shim.hip")] + [os.path.join(INCLUDE, "rtlws_cutout.h")]
LIMITS = ("MIN_NCHAN", "MAX_NCHAN", "MAX_TRIALS", "MAX_DELAY", "MAX_WIDTHS", "MAX_WIDTH", "MAX_BIN", "MIN_NX", "MAX_NX", "MAX_NF", "MAX_RQ", "MAX_DQ",
          "MAX_NSAMP", "MAX_CAND", "CAND_WORDS", "INFO_WORDS")
W3, B3 = np.array([1, 2, 5], np.int32), np.array([1, 3, 16], np.int32)


@pytest.fixture(scope="module")
def co(built):
    import rtlws.cutout
    return rtlws.cutout


# ---- the restatement ----------------------------------------------------------------------------------------------

def _case(nchan, ntrials, nsamp, seed, dmax=9):
    rng = np.random.default_rng(seed)
    delays = rng.integers(0, dmax + 1, (ntrials, nchan)).astype(np.int32)
    rows = ref.waterfall(nsamp + dmax, nchan, seed + 100)
    mask = np.ones(nchan, np.uint8)
    mask[rng.integers(0, nchan)] = 0
    return rows, delays, mask


def test_the_restatement_is_the_sum_within_one_rounding_an_addition():
    """every F and G against the sum of the same terms in f64: |F - exact| <= (cpb + b) 2^-24 sum|terms| (cpb + b - 2
    additions of relative error 2^-24 each, to first order, with room for the second), G within b 2^-24 sum|terms|"""
    for nchan, nf, nx, seed in ((12, 3, 8, 1), (64, 1, 12, 2), (20, 20, 4, 3)):
        rows, delays, mask = _case(nchan, 5, 90, seed)
        series = ref.dedisp(rows, delays, mask, 90)
        cand = ref.list_of([(2, 0, 40), (4, 1, 3), (0, 2, 88), (1, 2, 45)])
        F, G, info = ref.cutout_ref(rows, series, cand, [4, 0], delays, mask, W3, B3, nx, nf, 2, 1, 90, 4)
        cpb = nchan // nf
        for i in range(4):
            t, k, at = (int(v) for v in cand[i, [0, 2, 3]])
            b, (n0, inside) = int(B3[k]), ref.window(at, int(W3[k]), int(B3[k]), nx, 90)
            assert info[i].tolist() == [n0, b, 1, inside]
            n = n0 + np.arange(nx * b)
            ok = (n >= 0) & (n < 90)
            assert ok.sum() == inside
            for f in range(nf):
                ch = [c for c in range(f * cpb, (f + 1) * cpb) if mask[c]]
                terms = np.zeros((len(ch), nx * b))
                for a, c in enumerate(ch):
                    terms[a, ok] = rows[n[ok] + delays[t, c], c].astype(np.float64)
                exact, size = terms.reshape(len(ch), nx, b).sum(axis=(0, 2)), np.abs(terms).reshape(len(ch), nx, b).sum(axis=(0, 2))
                assert np.all(np.abs(F[i, f] - exact) <= (cpb + b) * 2.0 ** -24 * size), (nchan, i, f)
            for r in range(5):
                q = t + r - 2
                terms = np.zeros(nx * b)
                if 0 <= q < 5:
                    terms[ok] = series[q, n[ok]].astype(np.float64)
                exact, size = terms.reshape(nx, b).sum(axis=1), np.abs(terms).reshape(nx, b).sum(axis=1)
                assert np.all(np.abs(G[i, r] - exact) <= b * 2.0 ** -24 * size), (nchan, i, r)
                assert (0 <= q < 5) or not G[i, r].any()


def test_the_two_ties_to_the_dedispersion_hold_in_the_restatement():
    """nf = 1, b = 1: F[i][0][x] is D[t][n0 + x] bit for bit inside the series; b = 1: G[i][rq][x] is it with -0.0 as +0.0"""
    rows, delays, mask = _case(16, 3, 70, 7)
    rows[30 + delays[1], np.arange(16)] = np.float32(-0.0)        # a sample of the series that is -0.0
    series = ref.dedisp(rows, delays, mask, 70)
    assert series[1, 30] == 0.0 and not np.signbit(series[1, 30])  # the dedispersion never gives -0.0 either
    series[1, 31] = np.float32(-0.0)                              # but a caller's series may hold one
    cand = ref.list_of([(1, 0, 30), (2, 0, 2), (0, 0, 69)])
    F, G, info = ref.cutout_ref(rows, series, cand, [3, 0], delays, mask, [1], [1], 12, 1, 1, 1, 70, 3)
    for i, (t, at) in enumerate(((1, 30), (2, 2), (0, 69))):
        n = at - 6 + np.arange(12)
        ok = (n >= 0) & (n < 70)
        want = ref.dedisp(rows, delays, mask, 70)[t, n[ok]]
        assert np.array_equal(F[i, 0, ok].view(np.uint32), want.view(np.uint32)) and not F[i, 0, ~ok].view(np.uint32).any()
        assert np.array_equal(G[i, 1, ok].view(np.uint32), (series[t, n[ok]] + np.float32(0.0)).view(np.uint32))
    assert G[0, 1, 7] == 0.0 and not np.signbit(G[0, 1, 7]) and np.signbit(series[1, 31])


def test_an_invalid_candidate_is_all_zeros_in_the_restatement():
    rows, delays, mask = _case(8, 3, 40, 9)
    series = ref.dedisp(rows, delays, mask, 40)
    cand = ref.list_of([(-1, 0, 5), (3, 0, 5), (0, -1, 5), (0, 3, 5), (0, 0, -1), (0, 0, 40), (0, 0, 39)])
    F, G, info = ref.cutout_ref(rows, series, cand, [7, 0], delays, mask, W3, B3, 4, 2, 1, 1, 40, 7)
    assert not F[:6].view(np.uint32).any() and not G[:6].view(np.uint32).any() and not info[:6].any()
    assert info[6].tolist() == [37, 1, 1, 3] and F[6].any()


# ---- the library without a GPU ------------------------------------------------------------------------------------

def test_exports_are_the_header(co):
    import test_abi_cpu
    declared = test_abi_cpu._declared_functions("rtlws_cutout.h")
    assert len(declared) == 8 and set(declared) == set(co.SYMBOLS)
    assert test_abi_cpu._exported(co.CUTOUT_LIB) == set(declared)
    mapped = open(os.path.join(ROOT, "rtl-ws_amd", "exports", "cutout.map")).read()
    assert re.findall(r"global:\s*([^;]+);", mapped) == ["rtlws_cutout_*"] and all(n.startswith("rtlws_cutout_") for n in declared)
    L = co.lib()
    assert all(getattr(L, f).argtypes is not None for f in co.SYMBOLS)


def test_the_header_is_strict_c99(tmp_path):
    src = tmp_path / "t_rtlws_cutout.c"
    src.write_text('#include "rtlws_cutout.h"\nint main(void) { int32_t w = 1; long n0; return rtlws_cutout_supported(4, 1, 1, &w, &w, 4, 1, 0, 1) && '
                   '!rtlws_cutout_window(0, 1, 1, 4, 1, &n0, 0) ? 0 : 1; }\n')
    out = subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Wextra", "-Werror", "-I", INCLUDE, "-c", str(src), "-o", os.devnull],
                         capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    code = re.sub(r"/\*.*?\*/", "", open(os.path.join(INCLUDE, "rtlws_cutout.h")).read(), flags=re.S)
    assert "hipStream_t" not in code and "hipError_t" not in code
    for name in LIMITS:
        assert re.search(r"#define RTLWS_CUTOUT_%s %d\b" % (name, getattr(ref, name)), code), name


def test_the_pinned_surface_holds_with_the_submodule(built, co):
    """tests/test_python_api_cpu.py's snapshot with rtlws.cutout imported: no new public name, no new Engine method, the
    plan no _Plan subclass"""
    import test_python_api_cpu as api
    rec, now = api._recorded(), api.snapshot(built)
    assert built.cutout is co
    for part in ("names", "functions", "methods"):
        assert now[part] == rec[part], part
    assert not issubclass(co.CutoutPlan, built._Plan) and issubclass(co.CutoutPlan, built._PlanBase)
    assert "cutout" not in api.SATELLITES
    assert "librtlws_cutout.so (include/rtlws_cutout.h)" in co.lib.__doc__
    assert {"supported", "geometry", "window", "cutout", "CutoutPlan", "GUARD", "SYMBOLS", "last_error", "lib"} <= set(vars(co))
    for name in LIMITS:
        assert getattr(co, name) == getattr(ref, name), name


NCHAN_TEXT, TRIALS_TEXT = "nchan must be 4 .. 4096 and a multiple of 4", "ntrials must be 1 .. 4096"
NWIDTHS_TEXT, WIDTH_TEXT, ASCEND_TEXT = "nwidths must be 1 .. 16", "every width must be 1 .. 1024", "the widths must be strictly ascending"
BIN_TEXT, NX_TEXT, NF_TEXT = "every bin must be 1 .. 1024", "nx must be 4 .. 256 and a multiple of 4", "nf must be 1 .. nchan and divide nchan"
RQ_TEXT, DQ_TEXT, DELAY_TEXT = "rq must be 0 .. 64", "dq must be 1 .. 64", "every delay must be 0 .. 65535"
NSAMP_TEXT, CAND_TEXT = "nsamp must be 1 .. 2^30", "max_cand must be 1 .. 4096"
# (nchan, ntrials, widths, bins, nx, nf, rq, dq) -> the refusal, None when served; every line breaks the rules behind the
# one that speaks as well
SHAPE_LIMITS = [((4, 1, [1], [1], 4, 1, 0, 1), None), ((4096, 4096, list(range(1, 17)), [1024] * 16, 256, 4096, 64, 64), None), ((12, 5, [1024], [1], 8, 3, 1, 1), None),
                ((1028, 7, [1, 2], [1, 1024], 36, 1, 0, 64), None), ((260, 2, [3], [2], 4, 65, 64, 1), None),
                ((0, 0, [], [], 0, 0, -1, 0), NCHAN_TEXT), ((6, 0, [], [], 0, 0, -1, 0), NCHAN_TEXT), ((4100, 0, [], [], 0, 0, -1, 0), NCHAN_TEXT),
                ((4, 0, [], [], 0, 0, -1, 0), TRIALS_TEXT), ((4, 4097, [], [], 0, 0, -1, 0), TRIALS_TEXT),
                ((4, 1, [], [], 0, 0, -1, 0), NWIDTHS_TEXT), ((4, 1, list(range(1, 18)), [1] * 17, 0, 0, -1, 0), NWIDTHS_TEXT),
                ((4, 1, [0], [0], 0, 0, -1, 0), WIDTH_TEXT), ((4, 1, [1025], [0], 0, 0, -1, 0), WIDTH_TEXT), ((4, 1, [2, 2], [0, 0], 0, 0, -1, 0), ASCEND_TEXT),
                ((4, 1, [1, 2], [1, 0], 0, 0, -1, 0), BIN_TEXT), ((4, 1, [1], [1025], 0, 0, -1, 0), BIN_TEXT),
                ((4, 1, [1], [1], 0, 0, -1, 0), NX_TEXT), ((4, 1, [1], [1], 6, 0, -1, 0), NX_TEXT), ((4, 1, [1], [1], 260, 0, -1, 0), NX_TEXT),
                ((4, 1, [1], [1], 4, 0, -1, 0), NF_TEXT), ((4, 1, [1], [1], 4, 3, -1, 0), NF_TEXT), ((4096, 1, [1], [1], 4, 8192, -1, 0), NF_TEXT), ((8, 1, [1], [1], 4, 16, -1, 0), NF_TEXT),
                ((4, 1, [1], [1], 4, 2, -1, 0), RQ_TEXT), ((4, 1, [1], [1], 4, 2, 65, 0), RQ_TEXT), ((4, 1, [1], [1], 4, 2, 0, 0), DQ_TEXT), ((4, 1, [1], [1], 4, 2, 64, 65), DQ_TEXT)]


def test_the_shape_rules_at_every_limit(co):
    for args, why in SHAPE_LIMITS:
        assert bool(co.supported(*args)) == (why is None), args
        assert co.last_error() == ("" if why is None else "rtlws_cutout: " + why), (args, co.last_error())
    w = np.array([1], np.int32)
    assert co.lib().rtlws_cutout_supported(4, 1, 1, None, None, 4, 1, 0, 1) == 0 and co.last_error() == "rtlws_cutout: null widths"
    assert co.lib().rtlws_cutout_supported(4, 1, 1, w.ctypes.data_as(C.c_void_p), None, 4, 1, 0, 1) == 0 and co.last_error() == "rtlws_cutout: null bins"


def test_geometry_is_the_stated_rule(co):
    """band-time: max_cand * ceil(nx / 32) * ceil(nf / per) workgroups of 256 threads, per = 256 / cpb subbands where cpb <=
    256, else 1, and the tile's 32 x 257 f32 of LDS; DM-time: max_cand * ndm workgroups of nx threads in whole wavefronts;
    max_delay over the kept positions; and every refusal of geometry in its order"""
    for nchan, nf, nx, rq, room in ((4, 4, 4, 0, 1), (12, 4, 36, 2, 3), (64, 64, 32, 64, 4096), (256, 1, 256, 1, 7), (260, 4, 64, 3, 64), (260, 1, 68, 0, 2),
                                    (1028, 1, 4, 16, 5), (4096, 256, 256, 64, 4096), (4096, 16, 128, 8, 100), (1024, 64, 64, 16, 1024)):
        cpb = nchan // nf
        per = 256 // cpb if cpb <= 256 else 1
        delays = (np.arange(3 * nchan, dtype=np.int32).reshape(3, nchan) * 5) % 1001
        mask = np.ones(nchan, np.uint8)
        mask[int(np.argmax(delays.max(axis=0)))] = 0
        want = (0, (room * -(-nx // 32) * -(-nf // per), room * (2 * rq + 1)), (256, -(-nx // 64) * 64), (32 * 257 * 4, 0), 2 * rq + 1)
        assert co.geometry(delays, None, W3, B3, nx, nf, rq, 1, room) == want + (int(delays.max()),), (nchan, nf, nx)
        assert co.geometry(delays, mask, W3, B3, nx, nf, rq, 1, room) == want + (int(delays[:, mask != 0].max()),), (nchan, nf, nx)
    assert co.geometry(np.zeros((2, 8), np.int32), np.zeros(8, np.uint8), W3, B3, 4, 2, 0, 1)[-1] == 0
    d = np.zeros((2, 8), np.int32)
    bad = d.copy()
    bad[1, 7] = 65536
    neg = d.copy()
    neg[0, 0] = -1
    cases = [((d, None, [0], [0], 0, 0, -1, 0, 0), WIDTH_TEXT), ((d, None, W3, [1, 1, 0], 0, 0, -1, 0, 0), BIN_TEXT), ((d, None, W3, B3, 5, 0, -1, 0, 0), NX_TEXT),
             ((d, None, W3, B3, 4, 3, -1, 0, 0), NF_TEXT), ((d, None, W3, B3, 4, 2, 65, 0, 0), RQ_TEXT), ((d, None, W3, B3, 4, 2, 1, 0, 0), DQ_TEXT),
             ((bad, None, W3, B3, 4, 2, 1, 1, 0), DELAY_TEXT), ((neg, None, W3, B3, 4, 2, 1, 1, 0), DELAY_TEXT), ((d, None, W3, B3, 4, 2, 1, 1, 0), CAND_TEXT),
             ((d, None, W3, B3, 4, 2, 1, 1, 4097), CAND_TEXT)]
    for args, text in cases:
        assert co.geometry(*args)[0] == -1 and co.last_error() == "rtlws_cutout_geometry: " + text, (args[2:], co.last_error())
    bad[1, 7], bad[0, 3] = 0, 65535
    assert co.geometry(bad, None, W3, B3, 4, 2, 1, 1)[-1] == 65535                # the limit itself is served
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    L = co.lib()
    assert L.rtlws_cutout_geometry(8, 2, None, None, 3, p(W3), p(B3), 4, 2, 1, 1, 1, None, None, None, None, None) == -1 and co.last_error().endswith(": null delays")
    assert L.rtlws_cutout_geometry(8, 2, p(d), None, 3, p(W3), p(B3), 4, 2, 1, 1, 1, None, None, None, None, None) == 0 and co.last_error() == ""


def test_the_window_s_rule_at_its_borders(co):
    """rtlws_cutout_window against the restatement: at = 0, at = nsamp - 1, a window longer than nsamp, odd widths, and its
    refusals"""
    seen = set()
    for at, width, b, nx, nsamp in ((0, 1, 1, 4, 100), (99, 1, 1, 4, 100), (0, 1024, 1024, 256, 100), (50, 3, 1, 8, 100), (50, 5, 3, 36, 100), (50, 7, 16, 4, 100),
                                    (0, 1, 1, 4, 1), (10, 1023, 1, 256, 11), (5, 2, 1, 4, 6), ((1 << 30) - 1, 1024, 1024, 256, 1 << 30), (50, 1, 1, 4, 100)):
        n0, inside = ref.window(at, width, b, nx, nsamp)
        assert co.window(at, width, b, nx, nsamp) == (0, n0, inside), (at, width, b, nx, nsamp)
        assert n0 == at + width // 2 - (nx // 2) * b and inside == len([n for n in range(max(n0, 0), min(n0 + nx * b, nsamp))])
        seen.add((n0 < 0, n0 + nx * b > nsamp, width % 2))
    assert {(True, True, 0), (True, False, 1), (False, True, 1), (False, False, 1), (True, True, 1)} <= seen
    assert co.window(10, 1023, 1, 256, 11) == (0, 393, 0)         # a wide boxcar near the end: the whole window lies behind the series
    for args, text in (((0, 0, 0, 0, 0), NSAMP_TEXT), ((0, 0, 0, 0, (1 << 30) + 1), NSAMP_TEXT), ((-1, 0, 0, 0, 10), "at must be 0 .. nsamp - 1"),
                       ((10, 0, 0, 0, 10), "at must be 0 .. nsamp - 1"), ((9, 0, 0, 0, 10), WIDTH_TEXT), ((9, 1025, 0, 0, 10), WIDTH_TEXT), ((9, 1, 0, 0, 10), BIN_TEXT),
                       ((9, 1, 1025, 0, 10), BIN_TEXT), ((9, 1, 1, 2, 10), NX_TEXT), ((9, 1, 1, 258, 10), NX_TEXT)):
        assert co.window(*args)[0] == -1 and co.last_error() == "rtlws_cutout_window: " + text, (args, co.last_error())
    assert co.lib().rtlws_cutout_window(5, 3, 2, 8, 20, None, None) == 0 and co.last_error() == ""


def test_open_and_rows_needed_without_an_engine(co):
    d = np.zeros((2, 8), np.int32)
    with pytest.raises(RuntimeError, match="rtlws_cutout_open: null engine"):
        co.CutoutPlan(None, d, None, W3, B3, 4, 2, 1, 1)
    for kw, text in ((dict(dq=0), DQ_TEXT), (dict(nf=3, rq=70), NF_TEXT), (dict(bins=[1, 1, 2000], nx=5), BIN_TEXT), (dict(widths=[2, 1, 3]), ASCEND_TEXT)):
        args = dict(delays=d, mask=None, widths=W3, bins=B3, nx=4, nf=2, rq=1, dq=1)
        args.update(kw)
        with pytest.raises(RuntimeError, match="rtlws_cutout_open: " + text):                       # the arguments come before the engine
            co.CutoutPlan(None, **args)
    bad = d.copy()
    bad[1, 1] = 70000
    with pytest.raises(RuntimeError, match="rtlws_cutout_open: " + DELAY_TEXT):
        co.CutoutPlan(None, bad, None, W3, B3, 4, 2, 1, 1)
    L = co.lib()
    for nsamp, text in ((0, NSAMP_TEXT), ((1 << 30) + 1, NSAMP_TEXT), (1, "null plan")):
        assert L.rtlws_cutout_rows_needed(None, nsamp) == -1 and co.last_error().startswith("rtlws_cutout_rows_needed: " + text), (nsamp, co.last_error())
    L.rtlws_cutout_close(None)


def test_every_refusal_of_a_run_in_its_order(co):
    """the refusals that need no plan come before the null plan's, in the header's order; every line breaks the rules behind
    it as well: (d_rows, in_stride, d_series, series_stride, nsamp, d_cand, d_count, max_cand, d_ft, d_dmt, d_info)"""
    run = lambda *args: co.lib().rtlws_cutout_run(None, *args, None)
    R, S, L, N, F, G, I = 4096, 8192, 12288, 16384, 20480, 24576, 28672       # aligned stand-ins: nothing is dereferenced before the plan
    for args, text in (((None, 0, None, 0, 0, None, None, 0, None, None, None), NSAMP_TEXT), ((None, 0, None, 0, (1 << 30) + 1, None, None, 0, None, None, None), NSAMP_TEXT),
                       ((None, 0, None, 0, 10, None, None, 0, None, None, None), CAND_TEXT), ((None, 0, None, 0, 10, None, None, 4097, None, None, None), CAND_TEXT),
                       ((None, 0, None, 0, 10, None, None, 1, None, None, None), "in_stride must be >= 4 and a multiple of 4"),
                       ((None, 6, None, 0, 10, None, None, 1, None, None, None), "in_stride must be >= 4 and a multiple of 4"),
                       ((None, 4, None, 9, 10, None, None, 1, None, None, None), "series_stride must be >= nsamp"),
                       ((None, 4, None, 10, 10, None, None, 1, None, None, None), "d_ft and d_dmt must not both be NULL"),
                       ((R + 2, 4, S + 2, 10, 10, None, N + 2, 1, F + 2, G + 2, I + 2), "null pointer"), ((R + 2, 4, S + 2, 10, 10, L + 8, None, 1, F + 2, G + 2, I + 2), "null pointer"),
                       ((R + 2, 4, S + 2, 10, 10, L + 8, N + 2, 1, F + 2, G + 2, None), "null pointer"), ((None, 4, S + 2, 10, 10, L + 8, N + 2, 1, F + 2, G + 2, I + 2), "null pointer"),
                       ((R + 2, 4, None, 10, 10, L + 8, N + 2, 1, F + 2, G + 2, I + 2), "null pointer"),
                       ((R + 8, 4, S + 2, 10, 10, L + 8, N + 2, 1, F + 2, G + 2, I + 2), "d_rows must be 16-byte aligned"),
                       ((R, 4, S + 2, 10, 10, L + 8, N + 2, 1, F + 2, G + 2, I + 2), "d_cand must be 16-byte aligned"),
                       ((R, 4, S + 2, 10, 10, L, N + 2, 1, F + 2, G + 2, I + 2), "d_series must be 4-byte aligned"),
                       ((R, 4, S + 4, 10, 10, L, N + 2, 1, F + 2, G + 2, I + 2), "d_count must be 4-byte aligned"),
                       ((R, 4, S + 4, 10, 10, L, N + 4, 1, F + 2, G + 2, I + 2), "d_ft must be 4-byte aligned"),
                       ((R, 4, S + 4, 10, 10, L, N + 4, 1, F + 4, G + 2, I + 2), "d_dmt must be 4-byte aligned"),
                       ((R, 4, S + 4, 10, 10, L, N + 4, 1, F + 4, G + 4, I + 2), "d_info must be 4-byte aligned"),
                       ((R, 4, S + 4, 10, 10, L, N + 4, 1, F + 4, G + 4, I + 4), "null plan"),
                       ((None, 4, S, 10, 10, L, N, 1, None, G, I), "null plan"), ((R, 4, None, 1 << 30, 1 << 30, L, N, 4096, F, None, I), "null plan")):
        assert run(*args) == -1 and co.last_error().startswith("rtlws_cutout_run: " + text), (args, co.last_error())


def test_the_new_sources_carry_no_conditionals():
    for path in NEW_SOURCES:
        lines = [ln.strip() for ln in open(path) if re.match(r"\s*#", ln)]
        other = [ln for ln in lines if not re.match(r"#\s*(include|pragma|define)\b", ln)]
        guards = [ln for ln in other if re.match(r"#\s*(ifndef RTLWS_\w+_H|endif\b|ifdef __cplusplus)", ln)]
        assert other == guards, (path, [ln for ln in other if ln not in guards])
        assert sum(ln.startswith("#ifndef") for ln in lines) == (0 if path.endswith(".hip") else 1), path


def test_the_shim_takes_the_family_s_text():
    """the plan, its open and close, the answer of supported and the shared rules are csrc/search_plan.h's, the table's texts
    the dedispersion's, not restated; the limits are held to the shared ones; no atomic operation and no wait on memory in
    the kernels"""
    shim = open(os.path.join(CSRC, "cutout_shim.hip")).read()
    for name in ("struct rtlws_cutout_plan : rtlws::search::Plan", "sp::open_plan<rtlws_cutout_plan>", "sp::close_plan(p,", "supported(\"rtlws_cutout\"", "sp::why_not_nchan(",
                 "sp::why_not_widths(", "sp::why_not_grid(", "sp::why_not_stride_of_rows(", "sp::why_not_row_stride(", "sp::ceil_div(", "sp::misaligned(", "sp::use_device(",
                 "static_assert(", "NULL_PLAN", "prepare_cutout()", "dd::WHY_NTRIALS", "dd::WHY_NULL_DELAYS", "dd::WHY_DELAY", "MAX_NCHAN == sp::MAX_NCHAN",
                 "MAX_WIDTHS == sp::MAX_WIDTHS", "MAX_NSAMP == sp::MAX_NSAMP"):
        assert name in shim, name
    for text in ("nchan must be", "ntrials must be", "nwidths must be", "strictly ascending", "more workgroups than", "null plan", "null delays", "every delay must",
                 "hipFree", "hipMalloc", "hipMemcpy"):
        assert text not in shim, text
    head = open(os.path.join(CSRC, "search_plan.h")).read().split("#ifndef")[0]
    assert "cutout_shim.hip" in head
    kernels = open(os.path.join(CSRC, "cutout.hip")).read()
    assert "atomic" not in kernels.lower() and "volatile" not in kernels and "while" not in kernels and '#include "cutout.h"' in kernels
    assert "load_kernel(kernel)" in kernels and kernels.count("__global__") == 2


def test_no_kernel_of_the_library_spills(co):
    """the code object's metadata of the three kernels: no spill, no scratch, at most 256 threads, the LDS what geometry
    reports"""
    from rtlws import codeobj
    co.lib()
    found = {}
    for k in codeobj.kernels(co.CUTOUT_LIB):
        m = re.search(r"rtlws::cutout::cutout_(band_kernel<\w+>|dmt_kernel)\(", k.get("demangled", k["name"]))
        assert m, k
        found[m.group(1)] = k
    assert set(found) == {"band_kernel<false>", "band_kernel<true>", "dmt_kernel"}
    lds = co.geometry(np.zeros((2, 8), np.int32), None, W3, B3, 4, 2, 1, 1)[3]
    for name, k in found.items():
        assert k["vgpr_spill_count"] == 0 and k["private_segment_fixed_size"] == 0 and not k.get("sgpr_spill_count", 0), name
        assert k["vgpr_count"] + (k.get("agpr_count") or 0) <= 128 and k["max_flat_workgroup_size"] == 256, name
        assert k["group_segment_fixed_size"] == lds[name == "dmt_kernel"], name
        print(name, "vgpr", k["vgpr_count"], "sgpr", k["sgpr_count"], "lds", k["group_segment_fixed_size"])


def test_the_makefile_builds_it(co):
    txt = open(os.path.join(ROOT, "rtl-ws_amd", "Makefile")).read()
    assert re.search(r"^SATELLITES := .*\bcutout\b", txt, flags=re.M)
    assert re.search(r"^\$\(eval \$\(call SATELLITE,cutout,cutout cutout_shim,.*csrc/search_plan\.h", txt, flags=re.M)
    assert re.search(r"^\$\(BUILD\)/cutout\.o: csrc/cutout\.hip .*\n\t\$\(HIPCC\) \$\(HIPFLAGS\) -ffp-contract=off ", txt, flags=re.M)
    out = subprocess.run(["nm", "-D", "--undefined-only", co.CUTOUT_LIB], capture_output=True, text=True, check=True).stdout
    assert "rtlws_engine_device" in out and "rtlws_engine_stream" in out          # the engine is librtlws_hip.so's
    assert "rtlws_sift_" not in out and "rtlws_dedisp_" not in out and "rtlws_pulse_" not in out      # and nothing of the libraries it follows

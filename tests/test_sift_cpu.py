"""CPU suite of include/rtlws_sift.h: the restatement's own properties (tests/sift_ref.py: the vectorised stages against
the definition event by event, rt = rs = 0, a threshold of +Inf, the order, stage 1 against rtlws_pulse_snr bit for bit),
and what the library does without a GPU: its exports and prototypes, the header as strict C99, every refusal in its order,
the geometry against the stated rule, the shape rules at every limit, the binding's place beside the pinned surface, the
Makefile's entries, the kernels' registers and LDS."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import sift_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "rtl-ws_amd", "csrc")
INCLUDE = os.path.join(ROOT, "include")
NEW_SOURCES = [os.path.join(CSRC, f) for f in ("sift.h", "sift.hip", "sift_shim.hip")] + [os.path.join(INCLUDE, "rtlws_sift.h")]
W3 = np.array([1, 2, 4], np.int32)


@pytest.fixture(scope="module")
def sf(built):
    import rtlws.sift
    return rtlws.sift


# ---- the restatement ----------------------------------------------------------------------------------------------

# (T, K, S, seed, tail, step, threshold, rt, rs): the random cases of this file and of tests/test_sift_gpu.py; every one is
# held to ref.richness below
RANDOM_CASES = [(5, 3, 7, 1, None, None, 1.0, 1, 0), (40, 16, 33, 2, 17, None, 2.0, 4, 2), (9, 2, 12, 3, 2, 0.5, 1.0, 1, 1),
                (12, 4, 10, 4, None, 0.25, 0.5, 1, 1)]


def test_the_random_cases_are_not_vacuous():
    """at least 8 candidates, a suppressed event above the threshold and a box of three members or more, by the
    restatement alone"""
    for T, K, S, seed, tail, step, thr, rt, rs in RANDOM_CASES:
        got = ref.richness(*ref.random_case(T, K, S, seed, tail=tail, step=step), thr, rt, rs)
        print((T, K, S, seed), "candidates %d, suppressed %d, most members %d" % got)
        assert got[0] >= 8 and got[1] >= 1 and got[2] >= 3, ((T, K, S, seed), got)


def test_the_vectorised_stages_are_the_definition_event_by_event():
    for T, K, S, seed, tail, step, thr, rt, rs in RANDOM_CASES:
        peak, at, mom, widths, seg, nout = ref.random_case(T, K, S, seed, tail=tail, step=step)
        for radii in ((rt, rs), (0, 0), (32, 8), (0, 3), (2, 0)):
            cand, count, score, k = ref.sift_ref(peak, at, mom, widths, seg, nout, thr, *radii)
            slow = ref.sift_slow(score, thr, *radii)
            assert [(int(c[0]), int(c[1]), int(c[6]), int(c[7] & 0xFFFF), int(c[7] >> 16)) for c in cand] == slow, (seed, radii)
            assert count[0] == len(slow) and count[1] == int((score >= np.float32(thr)).sum())
    # equal scores are there for the tie rule to decide
    peak, at, mom, widths, seg, nout = ref.random_case(9, 2, 12, 3, tail=2, step=0.5)
    score, _ = ref.plane(peak, mom, widths, seg, nout)
    assert len(np.unique(score[:, :-1])) < score[:, :-1].size // 2


def test_zero_radii_keep_every_event_at_or_above_the_threshold():
    peak, at, mom, widths, seg, nout = ref.random_case(12, 4, 10, 4, step=0.25)
    for thr in (0.5, -np.inf, 0.0):
        cand, count, score, k = ref.sift_ref(peak, at, mom, widths, seg, nout, thr, 0, 0)
        assert count[0] == count[1] == int((score >= np.float32(thr)).sum()) and count[0] > 0
        assert np.all(cand[:, 6] == 1) and np.array_equal(cand[:, 7], (cand[:, 0] << 16) | cand[:, 0])
    assert ref.sift_ref(peak, at, mom, widths, seg, nout, -np.inf, 0, 0)[1][0] == 120


def test_a_threshold_of_plus_infinity_gives_none():
    peak, at, mom, widths, seg, nout = ref.random_case(5, 3, 7, 1)
    cand, count, _, _ = ref.sift_ref(peak, at, mom, widths, seg, nout, np.inf, 1, 1)
    assert cand.shape == (0, 8) and count.tolist() == [0, 0]
    peak[2, 1, 3] = np.inf                                        # but an infinite score is at or above it
    cand, count, score, _ = ref.sift_ref(peak, at, mom, widths, seg, nout, np.inf, 1, 1)
    assert count.tolist() == [1, 1] and cand[0, :3].tolist() == [2, 3, 1] and score[2, 3] == np.inf


def test_the_list_ascends_strictly_in_s_then_t():
    for T, K, S, seed, tail, step, thr, rt, rs in RANDOM_CASES:
        cand = ref.sift_ref(*ref.random_case(T, K, S, seed, tail=tail, step=step), thr, rt, rs)[0]
        key = cand[:, 1].astype(np.int64) * T + cand[:, 0]
        assert np.all(np.diff(key) > 0), seed


def test_among_equal_scores_of_a_box_exactly_one_survives():
    mom = ref.flat_moments(6, 64, 64 * 9)
    peak = np.full((6, 1, 9), 10.0, np.float32)
    at = np.zeros((6, 1, 9), np.int32)
    cand, count, score, _ = ref.sift_ref(peak, at, mom, [2], 64, 64 * 9, 0.0, 32, 8)
    assert len(np.unique(score)) == 1 and count.tolist() == [1, 54] and cand[0, [0, 1, 6, 7]].tolist() == [0, 0, 54, 5 << 16]
    # an event is beaten by an equal neighbour before it whether that neighbour survives or not: one candidate at any radius
    cand, count, _, _ = ref.sift_ref(peak, at, mom, [2], 64, 64 * 9, 0.0, 1, 1)
    assert count.tolist() == [1, 54] and cand[0, [0, 1, 6, 7]].tolist() == [0, 0, 4, 1 << 16]
    cand, count, _, _ = ref.sift_ref(peak, at, mom, [2], 64, 64 * 9, 0.0, 0, 1)
    assert [tuple(int(v) for v in c[:2]) for c in cand] == [(t, 0) for t in range(6)] and np.all(cand[:, 6] == 2)


def test_stage_one_is_rtlws_pulse_snr_rounded_to_float(built):
    """(float) rtlws_pulse_snr(peak, w, q1, q2, len) bit for bit wherever it is a number and the peak is one above -Inf,
    -Inf elsewhere: on random moments, a segment of constant samples, a last segment of one output, peaks of -Inf and NaN"""
    peak, at, mom, widths, seg, nout = ref.random_case(6, 5, 9, 11, tail=1)
    mom[1, 2] = (64 * 2.5, 64 * 6.25)                            # constant samples: the variance is exactly 0
    mom[2, 3] = (64 * 0.1, 64 * 0.1 * 0.1)                       # and where rounding makes it what it will
    peak[0, 1, 0], peak[0, 2, 1], peak[3, 0, 4] = -np.inf, np.nan, np.inf
    seen = set()
    for k, w in enumerate(widths):
        got = ref.score_of_width(peak[:, k, :], w, mom, seg, nout)
        for t in range(6):
            for s in range(9):
                ln = int(ref.lengths(seg, nout)[s])
                snr = built.pulse_snr(float(peak[t, k, s]), int(w), mom[t, s, 0], mom[t, s, 1], ln)
                with np.errstate(all="ignore"):
                    want = np.float32(snr)
                if np.isnan(want) or np.isnan(peak[t, k, s]) or peak[t, k, s] == -np.inf:
                    want = ref.NEG_INF
                    seen.add("refused")
                assert got[t, s].view(np.uint32) == want.view(np.uint32), (t, k, s, got[t, s], want)
                seen.add("number" if np.isfinite(want) else "infinite")
    assert seen == {"refused", "number", "infinite"}
    score, k_of = ref.plane(peak, mom, widths, seg, nout)
    assert np.all(score[:, 8] == ref.NEG_INF) and np.all(k_of[:, 8] == 0) and score[1, 2] == ref.NEG_INF and score[3, 4] == np.inf and k_of[3, 4] == 0


# ---- the library without a GPU ------------------------------------------------------------------------------------

def test_exports_are_the_header(sf):
    import test_abi_cpu
    declared = test_abi_cpu._declared_functions("rtlws_sift.h")
    assert len(declared) == 7 and set(declared) == set(sf.SYMBOLS)
    assert test_abi_cpu._exported(sf.SIFT_LIB) == set(declared)
    L = sf.lib()
    assert all(getattr(L, f).argtypes is not None for f in sf.SYMBOLS)


def test_the_header_is_strict_c99(tmp_path):
    src = tmp_path / "t_rtlws_sift.c"
    src.write_text('#include "rtlws_sift.h"\nint main(void) { int32_t w = 1; return rtlws_sift_supported(1, &w, 64, 0, 0) ? 0 : 1; }\n')
    out = subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Wextra", "-Werror", "-I", INCLUDE, "-c", str(src), "-o", os.devnull],
                         capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    code = re.sub(r"/\*.*?\*/", "", open(os.path.join(INCLUDE, "rtlws_sift.h")).read(), flags=re.S)
    assert "hipStream_t" not in code and "hipError_t" not in code
    for name in ("MAX_WIDTHS", "MAX_WIDTH", "MIN_SEG", "MAX_SEG", "MAX_TRIALS", "MAX_NOUT", "MAX_RT", "MAX_RS", "MAX_CAND", "CAND_WORDS"):
        assert re.search(r"#define RTLWS_SIFT_%s %d\b" % (name, getattr(ref, name)), code), name


def test_the_pinned_surface_holds_with_the_submodule(built, sf):
    """tests/test_python_api_cpu.py's snapshot with rtlws.sift imported: no new public name, no new Engine method, the plan
    no _Plan subclass"""
    import test_python_api_cpu as api
    rec, now = api._recorded(), api.snapshot(built)
    assert built.sift is sf
    for part in ("names", "functions", "methods"):
        assert now[part] == rec[part], part
    assert not issubclass(sf.SiftPlan, built._Plan) and issubclass(sf.SiftPlan, built._PlanBase)
    assert "sift" not in api.SATELLITES
    assert "librtlws_sift.so (include/rtlws_sift.h)" in sf.lib.__doc__
    assert {"supported", "geometry", "sift", "SiftPlan", "GUARD", "SYMBOLS", "CAND_WORDS", "last_error", "lib"} <= set(vars(sf))
    for name in ("MAX_WIDTHS", "MAX_WIDTH", "MIN_SEG", "MAX_SEG", "MAX_TRIALS", "MAX_NOUT", "MAX_RT", "MAX_RS", "MAX_CAND", "CAND_WORDS"):
        assert getattr(sf, name) == getattr(ref, name), name


NWIDTHS_TEXT, WIDTH_TEXT, ASCEND_TEXT = "nwidths must be 1 .. 16", "every width must be 1 .. 1024", "the widths must be strictly ascending"
SEG_TEXT, RT_TEXT, RS_TEXT = "seg must be 64 .. 1048576 and a multiple of 4", "rt must be 0 .. 32", "rs must be 0 .. 8"
TRIALS_TEXT, NOUT_TEXT = "ntrials must be 1 .. 65536", "nout must be 1 .. 2^30 (0: there is no event to sift)"
EVENTS_TEXT = "more than 2^31 - 1 events"
# (widths, seg, rt, rs) -> the refusal, None when served; where two rules refuse, the earlier one speaks
PLAN_LIMITS = [(([1], 64, 0, 0), None), ((list(range(1, 17)), 1048576, 32, 8), None), (([1024], 68, 32, 0), None), (([1, 1024], 64, 0, 8), None),
               (([], 0, -1, -1), NWIDTHS_TEXT), ((list(range(1, 18)), 64, 0, 0), NWIDTHS_TEXT),
               (([0], 0, -1, -1), WIDTH_TEXT), (([1025], 64, 0, 0), WIDTH_TEXT), (([2, 2], 0, 0, 0), ASCEND_TEXT), (([3, 2], 64, 0, 0), ASCEND_TEXT),
               (([1], 60, 33, 9), SEG_TEXT), (([1], 66, 0, 0), SEG_TEXT), (([1], 1048580, 0, 0), SEG_TEXT), (([1], 0, 0, 0), SEG_TEXT),
               (([1], 64, -1, 9), RT_TEXT), (([1], 64, 33, 0), RT_TEXT), (([1], 64, 0, -1), RS_TEXT), (([1], 64, 32, 9), RS_TEXT)]


def test_the_shape_rules_at_every_limit(sf):
    for args, why in PLAN_LIMITS:
        assert bool(sf.supported(*args)) == (why is None), args
        assert sf.last_error() == ("" if why is None else "rtlws_sift: " + why), (args, sf.last_error())
    assert sf.lib().rtlws_sift_supported(1, None, 64, 0, 0) == 0 and sf.last_error() == "rtlws_sift: null widths"


def test_geometry_is_the_stated_rule(sf):
    """scoring: one thread an event; the box and the list: one workgroup a tile of 64 x 64 events; the LDS of the code
    objects; and every refusal of geometry in its order"""
    for T, nout, seg in ((1, 1, 64), (5, 7 * 64, 64), (63, 64 * 65, 64), (64, 64 * 64, 64), (65, 64 * 63 + 1, 64), (4096, 1024 * 256, 256), (65536, 1 << 30, 1048576),
                         (1, 1 << 30, 64), (127, (1 << 30) - 63, 64)):
        S = -(-nout // seg)
        tiles = -(-T // 64) * -(-S // 64)
        got = sf.geometry(W3, seg, 3, 1, T, nout)
        assert got == (0, (-(-T * S // 256), tiles, tiles), (256, 256, 256), (0, 42016, 3376), 64, 64, S), ((T, nout, seg), got)
    assert sf.geometry(W3, 64, 32, 8, 4096, 1024 * 64)[3] == sf.geometry(W3, 64, 0, 0, 1, 1)[3]       # the LDS is static
    cases = [(([0], 60, 40, 9, 0, 0), WIDTH_TEXT), ((W3, 60, 40, 9, 0, 0), SEG_TEXT), ((W3, 64, 40, 9, 0, 0), RT_TEXT), ((W3, 64, 4, 9, 0, 0), RS_TEXT),
             ((W3, 64, 4, 1, 0, 0), TRIALS_TEXT), ((W3, 64, 4, 1, 65537, 0), TRIALS_TEXT), ((W3, 64, 4, 1, 1, 0), NOUT_TEXT), ((W3, 64, 4, 1, 1, -5), NOUT_TEXT),
             ((W3, 64, 4, 1, 1, (1 << 30) + 1), NOUT_TEXT), ((W3, 64, 4, 1, 128, 1 << 30), EVENTS_TEXT), ((W3, 64, 4, 1, 65536, 1 << 30), EVENTS_TEXT),
             ((W3, 64, 4, 1, 128, (1 << 30) - 63), EVENTS_TEXT)]
    for args, text in cases:
        assert sf.geometry(*args)[0] == -1 and sf.last_error() == "rtlws_sift_geometry: " + text, (args, sf.last_error())
    w = np.ascontiguousarray(W3)
    assert sf.lib().rtlws_sift_geometry(3, w.ctypes.data_as(C.c_void_p), 64, 1, 1, 5, 448, None, None, None, None, None, None) == 0 and sf.last_error() == ""


def test_open_and_run_without_an_engine(sf):
    with pytest.raises(RuntimeError, match="rtlws_sift_open: null engine"):
        sf.SiftPlan(None, W3, 64, 1, 1)
    with pytest.raises(RuntimeError, match="rtlws_sift_open: rt must be 0 .. 32"):                   # the arguments come before the engine
        sf.SiftPlan(None, W3, 64, 33, 1)
    with pytest.raises(RuntimeError, match="rtlws_sift_open: the widths must be strictly ascending"):
        sf.SiftPlan(None, [2, 1], 64, 1, 1)
    L = sf.lib()
    for args, text in (((0, 0), TRIALS_TEXT), ((1, 0), NOUT_TEXT), ((1, 1), "null plan")):
        assert L.rtlws_sift_work_bytes(None, *args) == -1 and sf.last_error().startswith("rtlws_sift_work_bytes: " + text), (args, sf.last_error())
    L.rtlws_sift_close(None)


def test_every_refusal_of_a_run_in_its_order(sf):
    """the refusals that need no plan come before the null plan's, in the header's order; every line breaks the rules behind
    it as well: (d_peak, d_at, d_mom, ntrials, nout, threshold, max_cand, d_work, d_cand, d_count, d_score, d_k)"""
    nan = float("nan")
    run = lambda *args: sf.lib().rtlws_sift_run(None, *args, None)
    P, A, M, W, D, N = 4096, 8192, 12288, 16384, 20480, 24576       # aligned stand-ins: nothing is dereferenced before the plan
    for args, text in (((None, None, None, 0, 0, nan, 0, None, None, None, 2, 2), TRIALS_TEXT), ((None, None, None, 65537, 0, nan, 0, None, None, None, 2, 2), TRIALS_TEXT),
                       ((None, None, None, 1, 0, nan, 0, None, None, None, 2, 2), NOUT_TEXT), ((None, None, None, 1, (1 << 30) + 1, nan, 0, None, None, None, 2, 2), NOUT_TEXT),
                       ((None, None, None, 1, 64, nan, 0, None, None, None, 2, 2), "threshold must not be NaN"),
                       ((None, None, None, 1, 64, 1.0, 0, None, None, None, 2, 2), "max_cand must be 1 .. 16777216"),
                       ((None, None, None, 1, 64, 1.0, (1 << 24) + 1, None, None, None, 2, 2), "max_cand must be 1 .. 16777216"),
                       ((None, A + 2, M + 4, 1, 64, 1.0, 1, W + 8, D + 8, N + 2, 2, 2), "null pointer"), ((P + 2, None, M + 4, 1, 64, 1.0, 1, W + 8, D + 8, N + 2, 2, 2), "null pointer"),
                       ((P + 2, A + 2, None, 1, 64, 1.0, 1, W + 8, D + 8, N + 2, 2, 2), "null pointer"), ((P + 2, A + 2, M + 4, 1, 64, 1.0, 1, None, D + 8, N + 2, 2, 2), "null pointer"),
                       ((P + 2, A + 2, M + 4, 1, 64, 1.0, 1, W + 8, None, N + 2, 2, 2), "null pointer"), ((P + 2, A + 2, M + 4, 1, 64, 1.0, 1, W + 8, D + 8, None, 2, 2), "null pointer"),
                       ((P + 2, A + 2, M + 4, 1, 64, 1.0, 1, W + 8, D + 8, N + 2, 2, 2), "d_peak must be 4-byte aligned"),
                       ((P, A + 2, M + 4, 1, 64, 1.0, 1, W + 8, D + 8, N + 2, 2, 2), "d_at must be 4-byte aligned"),
                       ((P, A, M + 4, 1, 64, 1.0, 1, W + 8, D + 8, N + 2, 2, 2), "d_mom must be 8-byte aligned"),
                       ((P, A, M + 8, 1, 64, 1.0, 1, W + 8, D + 8, N + 2, 2, 2), "d_work must be 16-byte aligned"),
                       ((P, A, M + 8, 1, 64, 1.0, 1, W, D + 8, N + 2, 2, 2), "d_cand must be 16-byte aligned"),
                       ((P, A, M + 8, 1, 64, 1.0, 1, W, D, N + 2, 2, 2), "d_count must be 4-byte aligned"),
                       ((P, A, M + 8, 1, 64, 1.0, 1, W, D, N + 4, 2, 2), "d_score must be 4-byte aligned"),
                       ((P, A, M + 8, 1, 64, 1.0, 1, W, D, N + 4, 4, 2), "d_k must be 4-byte aligned"),
                       ((P, A, M + 8, 1, 64, 1.0, 1, W, D, N + 4, 4, 4), "null plan"), ((P, A, M + 8, 65536, 1 << 30, float("-inf"), 1 << 24, W, D, N, None, None), "null plan")):
        assert run(*args) == -1 and sf.last_error().startswith("rtlws_sift_run: " + text), (args, sf.last_error())


def test_the_new_sources_carry_no_conditionals():
    for path in NEW_SOURCES:
        lines = [ln.strip() for ln in open(path) if re.match(r"\s*#", ln)]
        other = [ln for ln in lines if not re.match(r"#\s*(include|pragma|define)\b", ln)]
        guards = [ln for ln in other if re.match(r"#\s*(ifndef RTLWS_\w+_H|endif\b|ifdef __cplusplus)", ln)]
        assert other == guards, (path, [ln for ln in other if ln not in guards])
        assert sum(ln.startswith("#ifndef") for ln in lines) == (0 if path.endswith(".hip") else 1), path


def test_the_shim_takes_the_family_s_text():
    """the plan, its open and close, the answer of supported and the shared rules are csrc/search_plan.h's, not restated; no
    atomic operation and no wait on memory in the kernels"""
    shim = open(os.path.join(CSRC, "sift_shim.hip")).read()
    for name in ("struct rtlws_sift_plan : rtlws::search::Plan", "sp::open_plan<rtlws_sift_plan>", "sp::close_plan(p,", "supported(\"rtlws_sift\"", "sp::why_not_ntrials(",
                 "sp::why_not_widths(", "sp::why_not_grid(", "sp::ceil_div(", "sp::misaligned(", "sp::use_device(", "static_assert(", "NULL_PLAN", "prepare_sift()"):
        assert name in shim, name
    for text in ("ntrials must be", "nwidths must be", "strictly ascending", "more workgroups than", "null plan", "hipFree", "hipMalloc", "hipMemcpy"):
        assert text not in shim, text
    kernels = open(os.path.join(CSRC, "sift.hip")).read()
    assert "atomic" not in kernels.lower() and "volatile" not in kernels and "while" not in kernels and '#include "sift.h"' in kernels
    assert "load_kernel(kernel)" in kernels and kernels.count("__global__") == 3


def test_no_kernel_of_the_library_spills(sf):
    """the code object's metadata of the three kernels: no spill, no scratch, 256 threads, the LDS what geometry reports"""
    from rtlws import codeobj
    sf.lib()
    found = {}
    for k in codeobj.kernels(sf.SIFT_LIB):
        m = re.search(r"rtlws::sift::sift_(score|box|list)_kernel\(", k.get("demangled", k["name"]))
        assert m, k
        found[m.group(1)] = k
    assert set(found) == {"score", "box", "list"}
    lds = sf.geometry(W3, 64, 1, 1, 5, 448)[3]
    for which, name in enumerate(("score", "box", "list")):
        k = found[name]
        assert k["vgpr_spill_count"] == 0 and k["private_segment_fixed_size"] == 0 and not k.get("sgpr_spill_count", 0), name
        assert k["vgpr_count"] + (k.get("agpr_count") or 0) <= 128 and k["max_flat_workgroup_size"] == 256, name
        assert k["group_segment_fixed_size"] == lds[which], name
        print(name, "vgpr", k["vgpr_count"], "sgpr", k["sgpr_count"], "lds", k["group_segment_fixed_size"])


def test_the_makefile_builds_it(sf):
    txt = open(os.path.join(ROOT, "rtl-ws_amd", "Makefile")).read()
    assert re.search(r"^SATELLITES := .*\bsift\b", txt, flags=re.M)
    assert re.search(r"^\$\(eval \$\(call SATELLITE,sift,sift sift_shim,.*csrc/search_plan\.h", txt, flags=re.M)
    assert re.search(r"^\$\(BUILD\)/sift\.o: csrc/sift\.hip .*\n\t\$\(HIPCC\) \$\(HIPFLAGS\) -ffp-contract=off ", txt, flags=re.M)
    out = subprocess.run(["nm", "-D", "--undefined-only", sf.SIFT_LIB], capture_output=True, text=True, check=True).stdout
    assert "rtlws_engine_device" in out and "rtlws_engine_stream" in out          # the engine is librtlws_hip.so's
    assert "rtlws_pulse_" not in out                                              # and nothing of librtlws_pulse.so's

"""CPU suite of include/rtlws_subdedisp.h: the restatement's own identities (tests/subdedisp_ref.py against
tests/dedisp_ref.py, the later-row property), and what the library does without a GPU: its exports and prototypes, the
header as strict C99, every refusal of supported, delays and geometry in their order, the sweep's tables against numpy
entry for entry, the smear bound against rtlws_dedisp_delays, the plan's rule at every listed table
(tests/subdedisp_form_cases.py), the binding's place beside the pinned surface, the kernels' registers and LDS."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import dedisp_form_cases as forms1
import dedisp_ref
import subdedisp_form_cases as forms
import subdedisp_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "rtl-ws_amd", "csrc")
INCLUDE = os.path.join(ROOT, "include")
NEW_SOURCES = [os.path.join(CSRC, f) for f in ("subdedisp.h", "subdedisp.hip", "subdedisp_shim.hip", "dedisp_form.h")] + [os.path.join(INCLUDE, "rtlws_subdedisp.h")]


@pytest.fixture(scope="module")
def sd(built):
    import rtlws.subdedisp
    return rtlws.subdedisp


def same_bits(x, y):
    return x.shape == y.shape and x.dtype == y.dtype == np.float32 and np.array_equal(np.ascontiguousarray(x).view(np.uint32), np.ascontiguousarray(y).view(np.uint32))


# ---- the restatement ----------------------------------------------------------------------------------------------

def test_one_subband_and_a_nominal_per_trial_is_the_dedispersion():
    """B = 1, d2 = 0, A = T: D is dedisp_ref of d1 bit for bit, and P is D"""
    for M, T, maxd, seed in ((16, 5, 7, 1), (36, 9, 300, 2), (4, 1, 0, 3)):
        d1 = dedisp_ref.random_table(T, M, maxd, seed)
        rows = dedisp_ref.signed_rows(100 + maxd, M, seed)
        D, P = ref.subdedisp_ref(rows, np.arange(T + 1), d1, np.zeros((T, 1), np.int32), want_subbands=True)
        want = dedisp_ref.dedisp_ref(rows, d1)
        assert same_bits(D, want) and same_bits(P[:, 0, :], want), (M, T)
        mask = dedisp_ref.random_mask(M, seed)
        assert same_bits(ref.subdedisp_ref(rows, np.arange(T + 1), d1, np.zeros((T, 1), np.int32), mask), dedisp_ref.dedisp_ref(rows, d1, mask))


def integer_rows(nrows, width, seed):
    """integer-valued float32, 0 .. 255: any sum of up to 2^16 of them is below 2^24 and exact in any order"""
    return dedisp_ref.hashed_ints(nrows * width, 255, seed).astype(np.float32).reshape(nrows, width)


def test_exact_sums_do_not_see_the_subbands():
    """A = T, d2 = 0, integer-valued rows whose sums stay below 2^24: D is dedisp_ref of d1 bit for bit for any B"""
    for M, B, T, seed in ((16, 4, 3, 1), (48, 4, 5, 2), (72, 2, 4, 3), (72, 18, 2, 4)):
        d1 = dedisp_ref.random_table(T, M, 40, seed)
        rows = integer_rows(120, M, seed)
        assert M * 255 < 1 << 24
        got = ref.subdedisp_ref(rows, np.arange(T + 1), d1, np.zeros((T, B), np.int32))
        assert same_bits(got, dedisp_ref.dedisp_ref(rows, d1)), (M, B)
    # and the order is not idle: hashed floats differ from the single sum somewhere
    rows = dedisp_ref.hashed_rows(120, 48, 5)
    d1 = dedisp_ref.random_table(3, 48, 40, 6)
    assert not same_bits(ref.subdedisp_ref(rows, np.arange(4), d1, np.zeros((3, 4), np.int32)), dedisp_ref.dedisp_ref(rows, d1))


def test_a_run_from_a_later_row():
    M, B, seed = 48, 4, 9
    first = np.array([0, 2, 5], np.int32)
    d1, d2 = ref.random_tables(first, M, B, 30, 20, seed)
    rows = dedisp_ref.signed_rows(200, M, seed)
    whole, P = ref.subdedisp_ref(rows, first, d1, d2, want_subbands=True)
    assert whole.shape == (5, 150) and P.shape == (2, 4, 170)
    for j0 in (1, 7, 64):
        part, Pp = ref.subdedisp_ref(rows[j0:], first, d1, d2, want_subbands=True)
        assert same_bits(part, whole[:, j0:]) and same_bits(Pp, P[:, :, j0:])


def test_a_masked_subband_is_positive_zero():
    M, B = 48, 4
    first = np.array([0, 3], np.int32)
    d1, d2 = ref.random_tables(first, M, B, 9, 9, 4)
    rows = -np.abs(dedisp_ref.signed_rows(80, M, 4))
    mask = np.ones(M, np.uint8)
    mask[12:24] = 0
    d2[:, 1] = 60000                                              # a subband that keeps nothing does not count in max_d2
    D, P = ref.subdedisp_ref(rows, first, d1, d2, mask, want_subbands=True)
    assert ref.maxima(d1, d2, mask) == (9, 9) and D.shape == (3, 62)
    assert not P[:, 1].any() and not np.signbit(P[:, 1]).any()
    zeros = np.zeros(M, np.uint8)
    D0 = ref.subdedisp_ref(rows, first, d1, d2, zeros, nout=10)
    assert D0.shape == (3, 10) and not D0.any() and not np.signbit(D0).any() and ref.rows_needed(d1, d2, zeros, 10) == 10


def test_the_bound_holds_for_the_restatement():
    M, B = 72, 2
    first = ref.even_first(7, 3)
    d1, d2 = ref.random_tables(first, M, B, 50, 30, 8)
    rows = dedisp_ref.signed_rows(200, M, 8)
    D, P, D64 = ref.subdedisp_both(rows, first, d1, d2)
    ratio = (np.abs(D.astype(np.float64) - D64) / ref.bound(rows, first, d1, d2)).max()
    print("largest share of the bound %.3f" % ratio)
    assert 0.0 < ratio <= 1.0 and ref.gamma(M, B) > (36 + 2 - 2) * 2.0 ** -24


def test_a_dispersed_pulse_through_the_sweep_s_tables():
    """the restatement alone: the maximum of D lies at the trial the pulse was swept at and within 1 row of the injection;
    neighbouring trials' tables differ"""
    k = ref.PULSE
    rows, t0, row0 = ref.pulse_waterfall()
    first, d1, d2, smear = ref.tables(*ref.pulse_sweep())
    assert k["per_nominal"] % 2 == 1 and first[k["nominal"]] + k["per_nominal"] // 2 == t0
    assert all(not np.array_equal(d2[t], d2[t + 1]) for t in range(k["ntrials"] - 1)) and all(not np.array_equal(d1[a], d1[a + 1]) for a in range(len(first) - 2))
    D = ref.subdedisp_ref(rows, first, d1, d2)
    t, n = np.unravel_index(int(np.argmax(D)), D.shape)
    print("smear_rows %.2f, maximum %.0f of %d at trial %d, row %d; the next best trial %.0f" % (smear, D[t, n], k["nchan"], t, n, np.delete(D, t, axis=0).max()))
    assert t == t0 and abs(int(n) - (row0 + 1)) <= 1 and D[t, n] > 1.2 * np.delete(D, t, axis=0).max()


# ---- the library without a GPU ------------------------------------------------------------------------------------

def test_exports_are_the_header(sd):
    import test_abi_cpu
    declared = test_abi_cpu._declared_functions("rtlws_subdedisp.h")
    assert len(declared) == 10 and set(declared) == set(sd.SYMBOLS)
    assert test_abi_cpu._exported(sd.SUBDEDISP_LIB) == set(declared)
    L = sd.lib()
    assert all(getattr(L, f).argtypes is not None for f in sd.SYMBOLS)


def test_the_header_is_strict_c99(tmp_path):
    src = tmp_path / "t_rtlws_subdedisp.c"
    src.write_text('#include "rtlws_subdedisp.h"\nint main(void) { return rtlws_subdedisp_supported(4, 1, 1, 1) ? 0 : 1; }\n')
    out = subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Wextra", "-Werror", "-I", INCLUDE, "-c", str(src), "-o", os.devnull],
                         capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    code = re.sub(r"/\*.*?\*/", "", open(os.path.join(INCLUDE, "rtlws_subdedisp.h")).read(), flags=re.S)
    assert "hipStream_t" not in code and "hipError_t" not in code
    for name in ("MIN_NCHAN", "MAX_NCHAN", "MIN_PER_SUB", "MAX_NOMINALS", "MAX_TRIALS", "MAX_DELAY"):
        assert re.search(r"#define RTLWS_SUBDEDISP_%s %d\b" % (name, getattr(ref, name)), code), name


def test_the_pinned_surface_holds_with_the_submodule(built, sd):
    """tests/test_python_api_cpu.py's snapshot (the one tests/test_ffa_cpu.py holds) with rtlws.subdedisp imported: no new
    public name, no new Engine method, the plan no _Plan subclass"""
    import test_python_api_cpu as api
    rec, now = api._recorded(), api.snapshot(built)
    assert built.subdedisp is sd
    for part in ("names", "functions", "methods"):
        assert now[part] == rec[part], part
    assert not issubclass(sd.SubdedispPlan, built._Plan) and issubclass(sd.SubdedispPlan, built._PlanBase)
    assert "subdedisp" not in api.SATELLITES
    assert "librtlws_subdedisp.so (include/rtlws_subdedisp.h)" in sd.lib.__doc__
    assert {"supported", "delays", "geometry", "dedisperse", "SubdedispPlan", "GUARD", "SYMBOLS", "last_error", "lib"} <= set(vars(sd))


NCHAN_TEXT = "nchan must be 4 .. 4096 and a multiple of 4"
NSUB_TEXT = "nsub must be 1 .. nchan / 4 and divide nchan into subbands of a multiple of 4 positions"
NOMINAL_TEXT, TRIALS_TEXT, MORE_TEXT = "nnominal must be 1 .. 4096", "ntrials must be 1 .. 4096", "nnominal must be <= ntrials"
# (nchan, nsub, nnominal, ntrials) -> the refusal, None when served; where two rules refuse, the earlier one speaks
SHAPE_LIMITS = [((4, 1, 1, 1), None), ((4096, 1024, 4096, 4096), None), ((4096, 1, 1, 4096), None), ((48, 4, 2, 2), None), ((48, 12, 1, 1), None),
                ((0, 1, 1, 1), NCHAN_TEXT), ((6, 1, 1, 1), NCHAN_TEXT), ((4100, 1, 1, 1), NCHAN_TEXT), ((-4, 0, 0, 0), NCHAN_TEXT),
                ((4, 0, 1, 1), NSUB_TEXT), ((4, 2, 1, 1), NSUB_TEXT), ((48, 5, 1, 1), NSUB_TEXT), ((48, 8, 1, 1), NSUB_TEXT), ((48, 24, 1, 1), NSUB_TEXT),
                ((48, -1, 0, 0), NSUB_TEXT), ((4096, 2048, 1, 1), NSUB_TEXT),
                ((4, 1, 0, 1), NOMINAL_TEXT), ((4, 1, 4097, 4097), NOMINAL_TEXT), ((4, 1, 0, 0), NOMINAL_TEXT),
                ((4, 1, 1, 0), TRIALS_TEXT), ((4, 1, 1, 4097), TRIALS_TEXT), ((4, 1, 2, 1), MORE_TEXT), ((4, 1, 4096, 4095), MORE_TEXT)]


def test_the_shape_rules_at_every_limit(sd):
    for args, why in SHAPE_LIMITS:
        assert bool(sd.supported(*args)) == (why is None), args
        assert sd.last_error() == ("" if why is None else "rtlws_subdedisp: " + why), (args, sd.last_error())


def _geometry(sd, nchan, nsub, nnominal, ntrials, first, d1, d2, mask, nout):
    """rtlws_subdedisp_geometry with every argument as given (None: a NULL pointer) -> its return code"""
    p = lambda a: None if a is None else np.ascontiguousarray(a).ctypes.data_as(C.c_void_p)
    keep = [np.ascontiguousarray(a) for a in (first, d1, d2, mask) if a is not None]
    rc = sd.lib().rtlws_subdedisp_geometry(nchan, nsub, nnominal, ntrials, p(first), p(d1), p(d2), p(mask), nout, None, None, None, None, None, None, None, None)
    del keep
    return rc


def test_every_refusal_of_geometry_in_its_order(sd):
    i32 = lambda *v: np.array(v, np.int32)
    first, d1, d2 = i32(0, 1, 3), np.zeros((2, 8), np.int32), np.zeros((3, 2), np.int32)
    bad1, bad2, neg2 = d1.copy(), d2.copy(), d2.copy()
    bad1[1, 7], bad2[2, 1], neg2[0, 0] = 65536, 65536, -1
    ok = (8, 2, 2, 3, first, d1, d2, None, 10)
    assert _geometry(sd, *ok) == 0 and sd.last_error() == ""
    cases = [((6, 0, 0, 0, None, None, None, None, -1), NCHAN_TEXT), ((8, 3, 0, 0, None, None, None, None, -1), NSUB_TEXT),
             ((8, 2, 0, 0, None, None, None, None, -1), NOMINAL_TEXT), ((8, 2, 2, 0, None, None, None, None, -1), TRIALS_TEXT),
             ((8, 2, 3, 2, None, None, None, None, -1), MORE_TEXT), ((8, 2, 2, 3, None, None, None, None, -1), "null first"),
             ((8, 2, 2, 3, i32(0, 1, 1), None, None, None, -1), "first must ascend strictly from 0 to ntrials"),
             ((8, 2, 2, 3, i32(0, 3, 2), None, None, None, -1), "first must ascend strictly from 0 to ntrials"),
             ((8, 2, 2, 3, i32(1, 2, 3), None, None, None, -1), "first must ascend strictly from 0 to ntrials"),
             ((8, 2, 2, 3, i32(0, 1, 2), None, None, None, -1), "first must ascend strictly from 0 to ntrials"),
             ((8, 2, 2, 3, i32(0, 1, 4), None, None, None, -1), "first must ascend strictly from 0 to ntrials"),
             ((8, 2, 2, 3, first, None, d2, None, -1), "null delays"), ((8, 2, 2, 3, first, d1, None, None, -1), "null delays"),
             ((8, 2, 2, 3, first, bad1, bad2, None, -1), "every delay must be 0 .. 65535"), ((8, 2, 2, 3, first, d1, bad2, None, -1), "every delay must be 0 .. 65535"),
             ((8, 2, 2, 3, first, d1, neg2, None, -1), "every delay must be 0 .. 65535"),
             # a delay out of range is refused under the mask too
             ((8, 2, 2, 3, first, bad1, d2, np.zeros(8, np.uint8), -1), "every delay must be 0 .. 65535"),
             ((8, 2, 2, 3, first, d1, d2, None, -1), "nout must be >= 0")]
    for args, text in cases:
        assert _geometry(sd, *args) == -1 and sd.last_error() == "rtlws_subdedisp_geometry: " + text, (args, sd.last_error())
    # the grids: stage 1's first.  4096 nominals of one trial, one nominal a workgroup where neighbours spread 65535
    A = 4096
    wide1 = np.zeros((A, 4), np.int32)
    wide1[1::2] = 65535
    f = np.arange(A + 1, dtype=np.int32)
    assert sd.geometry(f, wide1, np.zeros((A, 1), np.int32), None, 0)[5] == 1
    most = (2 ** 31 - 1) // A * 256
    assert _geometry(sd, 4, 1, A, A, f, wide1, np.zeros((A, 1), np.int32), None, most + 1) == -1
    assert sd.last_error() == "rtlws_subdedisp_geometry: more workgroups than one grid holds"
    assert _geometry(sd, 4, 1, A, A, f, wide1, np.zeros((A, 1), np.int32), None, most - 65535) == 0
    # ... and stage 2's alone: eight nominals a workgroup in stage 1, one trial a workgroup in stage 2
    assert _geometry(sd, 4, 1, A, A, f, np.zeros((A, 4), np.int32), np.zeros((A, 1), np.int32), None, most + 1) == -1
    assert _geometry(sd, 4, 1, A, A, f, np.zeros((A, 4), np.int32), np.zeros((A, 1), np.int32), None, most) == 0


DELAYS_OK = (16, 4, 0, 1420.4e6, 2.0e6, 1e-4, 7, 10.0, 25.0, 3)


def _delays(sd, args, first=True, d1=True, d2=True, smear=True):
    """rtlws_subdedisp_delays with generous tables (False: a NULL pointer) -> its return code"""
    bufs = [(C.c_int32 * 70000)() if want else None for want in (first, d1, d2)]
    return sd.lib().rtlws_subdedisp_delays(*args, *bufs, C.byref(C.c_double()) if smear else None)


def test_every_refusal_of_delays_in_its_order(sd):
    nan, inf = float("nan"), float("inf")                       # 0 * inf is NaN: an infinite step fails at trial 0

    def args(**kw):
        names = ("nchan", "nsub", "shifted", "f", "bw", "row", "ntrials", "dm0", "step", "per")
        a = dict(zip(names, DELAYS_OK))
        a.update(kw)
        return tuple(a[n] for n in names)

    assert _delays(sd, DELAYS_OK) == 0 and sd.last_error() == "" and _delays(sd, DELAYS_OK, smear=False) == 0
    # each line breaks every rule behind it as well: the earliest speaks
    broken = dict(nchan=6, nsub=3, ntrials=0, shifted=2, per=0, f=-1.0, bw=0.0, row=nan, dm0=-1.0)
    order = [("nchan", NCHAN_TEXT), ("nsub", NSUB_TEXT), ("ntrials", TRIALS_TEXT), ("shifted", "shifted must be 0 or 1"), ("per", "per_nominal must be >= 1")]
    for k, (name, text) in enumerate(order):
        kw = {n: broken[n] for n, _ in order[k:]}
        kw.update(f=-1.0, bw=0.0, row=nan, dm0=-1.0)
        if "nchan" not in kw and "nsub" in kw:
            kw["nsub"] = 3
        assert _delays(sd, args(**kw), first=False) == -1 and sd.last_error() == "rtlws_subdedisp_delays: " + text, (name, sd.last_error())
    for which in ("first", "d1", "d2"):
        assert _delays(sd, args(f=-1.0, dm0=-1.0), **{which: False}) == -1 and sd.last_error() == "rtlws_subdedisp_delays: null table", which
    for kw, text in ((dict(bw=0.0, row=0.0, f=-1.0, dm0=-1.0), "bandwidth_hz must be finite and > 0"), (dict(bw=inf), "bandwidth_hz must be finite and > 0"),
                     (dict(row=0.0, f=-1.0, dm0=-1.0), "row_seconds must be finite and > 0"), (dict(row=nan), "row_seconds must be finite and > 0"),
                     (dict(f=0.9e6, dm0=-1.0), "every channel's frequency must be finite and > 0"), (dict(f=nan), "every channel's frequency must be finite and > 0"),
                     (dict(dm0=-1.0), "trial 0: the dispersion measure must be finite and >= 0"), (dict(step=-5.0), "trial 3: the dispersion measure must be finite and >= 0"),
                     (dict(dm0=nan), "trial 0: the dispersion measure must be finite and >= 0"), (dict(step=inf), "trial 0: the dispersion measure must be finite and >= 0"),
                     # d2 of trial 1 passes 65535 while d1 of its nominal stays below; then, in one wide subband, d1 of nominal 1 does
                     (dict(f=100e6, bw=8e6, row=1e-6, dm0=0.0, step=2.0, nsub=4, per=1), "trial 1: a delay above 65535 rows"),
                     (dict(f=100e6, bw=8e6, row=1e-6, dm0=0.0, step=2.0, nsub=1, per=1), "nominal 1: a delay above 65535 rows")):
        assert _delays(sd, args(**kw)) == -1 and sd.last_error() == "rtlws_subdedisp_delays: " + text, (kw, sd.last_error())
    with pytest.raises(RuntimeError, match="rtlws_subdedisp_delays failed .*per_nominal must be >= 1"):
        sd.delays(*args(per=0))


def test_the_sweep_against_numpy(sd, built):
    """every entry of first, d1 and d2 and smear_rows against the float64 restatement, on five sweeps: both `shifted`, one
    subband, a ragged last nominal, one trial a nominal; no argument of rint within 1e-9 of a half-integer; and the smear
    bound against rtlws_dedisp_delays: |d1[a(t)][i] + d2[t][s(i)] - full[t][i]| <= floor(smear_rows + 1.5), the real
    arguments differing by at most smear_rows and three roundings adding at most 0.5 each"""
    seen = set()
    for args in ref.DELAY_SETS:
        nchan, nsub, shifted, ntrials, per = args[0], args[1], args[2], args[6], args[9]
        want_first, q1, q2, want_smear = ref.sweep(*args)
        for q in (q1, q2):
            assert np.abs(np.abs(q - np.floor(q)) - 0.5).min() > 1e-9, args
        first, d1, d2, smear = sd.delays(*args)
        A = -(-ntrials // per)
        assert first.dtype == d1.dtype == d2.dtype == np.int32 and first.shape == (A + 1,) and d1.shape == (A, nchan) and d2.shape == (ntrials, nsub)
        assert np.array_equal(first, want_first) and np.array_equal(d1, np.rint(q1)) and np.array_equal(d2, np.rint(q2)), args
        assert smear == want_smear, (args, smear, want_smear)
        # the reference position of a subband is not delayed inside it, and what a subband's highest frequency is does not depend on `shifted`
        assert (d1.reshape(A, nsub, -1).min(axis=2) == 0).all()
        full = built.dedisp_delays(nchan, *args[2:9])
        both = d1[ref.nominal_of(first)] + d2[:, np.arange(nchan) // (nchan // nsub)]
        off = int(np.abs(both - full).max())
        assert off <= int(np.floor(smear + 1.5)), (args, off, smear)
        if per == 1:
            assert smear == 0.0 and off <= 1
        print("%s: smear_rows %.3f, largest difference from the full table %d rows, largest d1 %d, d2 %d" % (args, smear, off, d1.max(), d2.max()))
        seen |= {("shifted", shifted), ("one subband", nsub == 1), ("ragged", ntrials % per != 0), ("per 1", per == 1)}
    assert {("shifted", 0), ("shifted", 1), ("one subband", True), ("ragged", True), ("per 1", True)} <= seen
    # the same positions either way the rows were written: shifted rows are the unshifted ones rotated by half the band
    a = list(ref.DELAY_SETS[2])
    a[1] = 2                                                      # subbands that do not straddle the rotation
    s1 = sd.delays(*a)
    a[2] = 0
    s0 = sd.delays(*a)
    assert np.array_equal(np.roll(s0[1], 32, axis=1), s1[1]) and np.array_equal(s0[2][:, ::-1], s1[2]) and s0[3] == s1[3]


def test_the_cases_reach_every_form_on_both_sides_of_every_border():
    # stage 1: the dedispersion's list, held to its conditions by tests/test_dedisp_forms_cpu.py; here, that it is whole
    reached1 = {(c.plan_per, forms1.form(c.plan_spread, c.plan_per)[:2]) for c in forms.STAGE1_CASES}
    assert reached1 == {(per, (32, lds)) for per in (8, 4, 2, 1) for lds in (forms.SMALL_LDS, forms.BIG_LDS)} | \
        {(1, (chunk, lds)) for chunk in (16, 8, 4) for lds in (forms.SMALL_LDS, forms.BIG_LDS)} | {(1, ("lone", forms.SMALL_LDS))}
    for (_, last, beyond) in forms1.BORDERS[:-1]:
        assert {last, beyond} <= {c.plan_spread for c in forms.STAGE1_CASES}
    # stage 2: the rule's borders are where the words run out
    for lds, last, beyond in forms.BORDERS2:
        assert forms.form2(last, 8) == (lds, 256 + last) and forms.form2(beyond, 8) != (lds, 256 + beyond)
        assert forms.CHUNK * (256 + last) + 256 <= lds // 4 < forms.CHUNK * (256 + beyond) + 256
    assert forms.form2(249, 2) is None and forms.form2(0, 1) == (forms.SMALL_LDS, 256)
    reached2 = {(c.plan_per, forms.form2(c.plan_spread, c.plan_per)[0]) for c in forms.STAGE2_CASES}
    assert reached2 == {(per, lds) for per in (8, 4, 2) for lds in (forms.SMALL_LDS, forms.BIG_LDS)} | {(1, forms.SMALL_LDS)}
    for per in (8, 4, 2):
        assert {0, 1, 24, 25, 248, 249} <= {c.spread for c in forms.STAGE2_CASES if c.per == per}
    assert {(c.plan_per, forms.form2(c.plan_spread, c.plan_per)[0]) for c in forms.STAGE2_FORMS} == \
        {(8, forms.SMALL_LDS), (8, forms.BIG_LDS), (4, forms.BIG_LDS), (2, forms.SMALL_LDS), (1, forms.SMALL_LDS)}


def test_geometry_is_the_stated_rule(sd):
    """rtlws_subdedisp_geometry against the restated rule on every listed table: stage 1's cases with any d2, stage 2's with
    any d1, with and without masks, and the sweeps"""
    for case in forms.STAGE1_CASES:
        first, d1, d2 = forms.stage1_case_tables(case)
        got = sd.geometry(first, d1, d2, None, forms.NOUT)
        assert got == (0,) + forms.geometry(first, d1, d2, None, forms.NOUT), (forms1.case_id(case), got)
        assert (got[5], got[3][0]) == (case.plan_per, forms1.form(case.plan_spread, case.plan_per)[1]), forms1.case_id(case)
        assert got[6] == 2 and got[3][1] == forms.SMALL_LDS                   # two trials a nominal, d2 to 5
    for case in forms.STAGE1_FORMS:
        first, d1, d2 = forms.stage1_case_tables(case)
        for name, mask in forms1.masks(case, forms.NCHAN1):
            assert sd.geometry(first, d1, d2, mask, forms.NOUT) == (0,) + forms.geometry(first, d1, d2, mask, forms.NOUT), (forms1.case_id(case), name)
    for case in forms.STAGE2_CASES:
        first, d1, d2 = forms.stage2_case_tables(case)
        got = sd.geometry(first, d1, d2, None, forms.NOUT)
        assert got == (0,) + forms.geometry(first, d1, d2, None, forms.NOUT), (forms.case2_id(case), got)
        assert (got[6], got[3][1]) == (case.plan_per, forms.form2(case.plan_spread, case.plan_per)[0]), forms.case2_id(case)
        # the delayed subband masked out: nothing spreads, and the cap alone decides
        mask = np.ones(forms.NCHAN2, np.uint8)
        s = forms.delayed_subband(case)
        mask[4 * s:4 * s + 4] = 0
        got = sd.geometry(first, d1, d2, mask, forms.NOUT)
        assert got == (0,) + forms.geometry(first, d1, d2, mask, forms.NOUT), (forms.case2_id(case), "masked")
        if case.kind == "border":
            assert (got[6], got[3][1]) == (case.per, forms.SMALL_LDS), forms.case2_id(case)
        # all but one position of it masked: it spreads as before
        mask[4 * s + 1] = 1
        assert sd.geometry(first, d1, d2, mask, forms.NOUT)[6] == case.plan_per
    for args in ref.DELAY_SETS:
        first, d1, d2, _ = ref.tables(*args)
        for nout in (0, 1, 256, 1000):
            assert sd.geometry(first, d1, d2, None, nout) == (0,) + forms.geometry(first, d1, d2, None, nout), (args, nout)
    # one trial a nominal: every table within the limits is served, whatever d2
    first = np.arange(5, dtype=np.int32)
    d2 = np.array([[0, 65535], [65535, 0]] * 2, np.int32)
    got = sd.geometry(first, np.zeros((4, 8), np.int32), d2, None, 1)
    assert got[0] == 0 and got[6] == 1 and got[8] == 65535 and got[1] == (256, 4)
    # two trials of one nominal 65535 apart: one trial a workgroup
    got = sd.geometry(np.array([0, 4], np.int32), np.zeros((1, 8), np.int32), d2, None, 1)
    assert got[0] == 0 and got[6] == 1 and got[5] == 1 and got[1] == (256, 4)
    # the cap: two trials a nominal take groups of two, three of four, five of eight
    for most, per in ((1, 1), (2, 2), (3, 4), (4, 4), (5, 8), (17, 8)):
        first = np.array([0, most], np.int32)
        assert sd.geometry(first, np.zeros((1, 8), np.int32), np.zeros((most, 2), np.int32), None, 1)[6] == per, most


def test_open_and_run_without_an_engine(sd):
    first, d1, d2 = np.array([0, 1, 3], np.int32), np.zeros((2, 8), np.int32), np.zeros((3, 2), np.int32)
    with pytest.raises(RuntimeError, match="rtlws_subdedisp_open: null engine"):
        sd.SubdedispPlan(None, first, d1, d2)
    with pytest.raises(RuntimeError, match="rtlws_subdedisp_open: first must ascend"):                # the arguments come before the engine
        sd.SubdedispPlan(None, np.array([0, 2, 2], np.int32), d1, d2)
    with pytest.raises(RuntimeError, match="rtlws_subdedisp_open: every delay must be 0 .. 65535"):
        sd.SubdedispPlan(None, first, d1 - 1, d2)
    L = sd.lib()
    for fn in (L.rtlws_subdedisp_rows_needed, L.rtlws_subdedisp_mid_stride, L.rtlws_subdedisp_work_floats):
        assert fn(None, 10) == -1 and "null plan" in sd.last_error()
        assert fn(None, -1) == -1 and "nout must be >= 0" in sd.last_error()
    L.rtlws_subdedisp_close(None)
    # a run's refusals that need no plan come before the null plan's, in the header's order:
    # (d_rows, in_stride, nout, d_work, d_out, out_stride)
    run = lambda *args: L.rtlws_subdedisp_run(None, *args, None)
    for args, text in (((64, 0, -1, 0, 0, -2), "nout must be >= 0"), ((64, 0, 8, 0, 0, 4), "in_stride must be >= nchan"), ((72, 6, 8, 0, 0, 4), "in_stride must be a multiple of 4"),
                       ((72, 8, 8, 0, 0, 7), "out_stride must be >= nout"), ((None, 8, 8, 66, 130, 8), "null pointer"), ((72, 8, 8, None, 130, 8), "null pointer"),
                       ((72, 8, 8, 66, None, 8), "null pointer"), ((72, 8, 8, 66, 130, 8), "d_rows must be 16-byte aligned"),
                       ((64, 8, 8, 66, 130, 8), "d_work must be 4-byte aligned"), ((64, 8, 8, 68, 130, 8), "d_out must be 4-byte aligned"),
                       ((64, 8, 8, 68, 132, 8), "null plan"), ((None, 8, 0, None, None, 0), "null plan")):
        assert run(*args) == -1 and sd.last_error().startswith("rtlws_subdedisp_run: " + text), (args, sd.last_error())


def test_the_new_sources_carry_no_conditionals():
    for path in NEW_SOURCES:
        lines = [ln.strip() for ln in open(path) if re.match(r"\s*#", ln)]
        other = [ln for ln in lines if not re.match(r"#\s*(include|pragma|define)\b", ln)]
        guards = [ln for ln in other if re.match(r"#\s*(ifndef RTLWS_\w+_H|endif\b|ifdef __cplusplus)", ln)]
        assert other == guards, (path, [ln for ln in other if ln not in guards])
        assert sum(ln.startswith("#ifndef") for ln in lines) == (0 if path.endswith(".hip") else 1), path


def test_one_text_for_what_both_shims_state():
    """the rule that turns a table into a form lives in csrc/dedisp_form.h, which both shims include and neither restates;
    the band's formula and the shared rules are csrc/search_plan.h's"""
    shim, other = open(os.path.join(CSRC, "subdedisp_shim.hip")).read(), open(os.path.join(CSRC, "dedisp_shim.hip")).read()
    for text in (shim, other):
        assert '#include "dedisp_form.h"' in text and '#include "search_plan.h"' in text
        for name in ("unit_range", "widest_spread", "choose_layout", "build_tables"):
            assert not re.search(r"^\w[\w:<>\* ]*\b%s\(" % name, text, flags=re.M), name
        assert "4.148808e3" not in text and "must be 4 .. 4096" not in text and "0 .. 65535" not in text
    for name in ("struct rtlws_subdedisp_plan : rtlws::search::Plan", "sp::open_plan<rtlws_subdedisp_plan>", "sp::close_plan(p,", "supported(\"rtlws_subdedisp\"",
                 "sp::DISPERSION", "sp::why_not_band(", "sp::excess(", "sp::why_not_nchan(", "sp::why_not_row_stride(", "sp::why_not_stride(", "sp::why_not_grid(",
                 "sp::ceil_div(", "sp::misaligned(", "static_assert(", "dd::choose_layout(", "dd::build_tables("):
        assert name in shim, name
    kernels = open(os.path.join(CSRC, "subdedisp.hip")).read()
    assert "atomic" not in kernels.lower() and '#include "subdedisp.h"' in kernels
    assert "fit_stride" in open(os.path.join(CSRC, "dedisp_form.h")).read() and "struct Layout" not in open(os.path.join(CSRC, "subdedisp.h")).read()


def _kernels(sd):
    from rtlws import codeobj
    sd.lib()
    stage1, stage2 = {}, {}
    for k in codeobj.kernels(sd.SUBDEDISP_LIB):
        d = k.get("demangled", k["name"])
        m1 = re.search(r"rtlws::subdedisp::subdedisp_subband_kernel<(\d+), (false|true), (false|true)>", d)
        m2 = re.search(r"rtlws::subdedisp::subdedisp_trial_kernel<(\d+), (false|true)>", d)
        assert m1 or m2, d
        if m1:
            stage1[(int(m1.group(1)), m1.group(2) == "true", m1.group(3) == "true")] = k
        else:
            stage2[(int(m2.group(1)), m2.group(2) == "true")] = k
    return stage1, stage2


def test_no_kernel_of_the_library_spills(sd):
    """the code object's metadata of all 16 instantiations, exactly those the launch tables reach: no spill, no scratch, 256
    threads, the LDS what geometry reports for the form, no more registers than the workgroups that LDS admits can have"""
    stage1, stage2 = _kernels(sd)
    assert set(stage1) == {(t, False, big) for t in (8, 4, 2, 1) for big in (False, True)} | {(1, True, False)}
    assert set(stage2) == {(t, big) for t in (8, 4, 2) for big in (False, True)} | {(1, False)}
    for key, k in list(stage1.items()) + list(stage2.items()):
        assert k["vgpr_spill_count"] == 0 and k["private_segment_fixed_size"] == 0 and not k.get("sgpr_spill_count", 0), key
        assert k["vgpr_count"] + (k.get("agpr_count") or 0) <= (256 if key[-1] else 128), key
        assert k["max_flat_workgroup_size"] == 256
        assert k["group_segment_fixed_size"] == (forms.BIG_LDS if key[-1] else forms.SMALL_LDS), key
        print(key, "vgpr", k["vgpr_count"], "sgpr", k["sgpr_count"])
    # ... which is what geometry reports for a table of that form
    for case in forms.STAGE1_FORMS:
        got = sd.geometry(*forms.stage1_case_tables(case), None, forms.NOUT)
        f = forms1.form(case.plan_spread, case.plan_per)
        assert stage1[(case.plan_per, f[0] == "lone", got[3][0] == forms.BIG_LDS)]["group_segment_fixed_size"] == got[3][0] == f[1]
    for case in forms.STAGE2_FORMS:
        got = sd.geometry(*forms.stage2_case_tables(case), None, forms.NOUT)
        assert stage2[(case.plan_per, got[3][1] == forms.BIG_LDS)]["group_segment_fixed_size"] == got[3][1]


def test_the_makefile_builds_it(sd):
    txt = open(os.path.join(ROOT, "rtl-ws_amd", "Makefile")).read()
    assert re.search(r"^SATELLITES := .*\bsubdedisp\b", txt, flags=re.M)
    assert re.search(r"^\$\(eval \$\(call SATELLITE,subdedisp,subdedisp subdedisp_shim,", txt, flags=re.M)
    assert re.search(r"^\$\(BUILD\)/subdedisp_shim\.o: csrc/dedisp_form\.h$", txt, flags=re.M) and re.search(r"^\$\(BUILD\)/dedisp_shim\.o: csrc/dedisp_form\.h$", txt, flags=re.M)
    out = subprocess.run(["nm", "-D", "--undefined-only", sd.SUBDEDISP_LIB], capture_output=True, text=True, check=True).stdout
    assert "rtlws_engine_device" in out and "rtlws_engine_stream" in out          # the engine is librtlws_hip.so's
    assert "rtlws_dedisp_" not in out                                             # and nothing of librtlws_dedisp.so's

"""CPU suite of include/rtlws_fold.h (librtlws_fold.so): the ABI, the kernels' resources from the code-object metadata,
the block shape a bin count gets, the refusals and their order, rtlws_fold_step against fractions.Fraction,
rtlws_fold_phase_at, rtlws_fold_chi2 -- and the numpy restatement's own properties (tests/fold_ref.py), which hold the
yardstick of tests/test_fold_gpu.py rather than the code under test.  No GPU is used."""
import math
import os
import re
import subprocess
from fractions import Fraction

import numpy as np
import pytest

import fold_ref
from test_abi_cpu import INCLUDE, _declared_functions, _exported


def _u64(values):
    return np.ascontiguousarray(values, dtype=np.uint64)


def test_fold_library_exports_its_header_and_nothing_else(built):
    built.fold_lib()
    declared = _declared_functions("rtlws_fold.h")
    assert len(declared) == 10
    assert _exported(built.FOLD_LIB) == set(declared) == set(built.FOLD_SYMBOLS)
    dyn = subprocess.run(["readelf", "-d", built.FOLD_LIB], capture_output=True, text=True, check=True).stdout
    assert "librtlws_hip.so" in dyn and "$ORIGIN" in dyn
    txt = open(os.path.join(INCLUDE, "rtlws_fold.h")).read()
    for name, value in (("MAX_PERIODS", 4096), ("MIN_BINS", 2), ("MAX_BINS", 256), ("MIN_SUB", 64), ("MAX_SUB", 1 << 24),
                        ("MAX_TRIALS", 65536), ("MAX_NSAMP", 1 << 30)):
        assert re.search(r"#define RTLWS_FOLD_%s %d\b" % (name, value), txt) and getattr(built, "FOLD_" + name) == value
        assert getattr(fold_ref, name) == value


def test_fold_header_is_strict_c99(built, tmp_path):
    src = tmp_path / "uses_fold.c"
    src.write_text('#include "rtlws_fold.h"\nint main(void) { return rtlws_fold_supported(0, 0, 0, 0, 0); }\n')
    subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Wextra", "-Werror", "-I", INCLUDE, "-fsyntax-only", str(src)], check=True)


def _kernels(built):
    """{wavefronts per workgroup: metadata} of every kernel of the library"""
    from rtlws import codeobj
    built.fold_lib()
    names = {}
    for k in codeobj.kernels(built.FOLD_LIB):
        d = k.get("demangled", k["name"])
        m = re.search(r"rtlws::fold::fold_kernel<(\d+), rtlws::fold::RowReads>", d)
        assert m, d
        names[int(m.group(1))] = k
    return names


def test_fold_kernels_do_not_spill(built):
    """Every kernel of the library: no scratch, no spilled register, 64 threads per wavefront of its name, no static LDS
    (a workgroup's LDS is the launch's: waves_per_block * nbins * 256 bytes), and no more registers than eight
    wavefronts per SIMD have (64): the registers never limit the workgroups a compute unit holds, the LDS does"""
    names = _kernels(built)
    assert set(names) == {4, 2, 1}
    for wpb, k in names.items():
        assert k["vgpr_spill_count"] == 0 and k["private_segment_fixed_size"] == 0, wpb
        assert not k.get("sgpr_spill_count", 0), wpb
        assert k["max_flat_workgroup_size"] == 64 * wpb
        assert k["group_segment_fixed_size"] == 0
        assert k["vgpr_count"] + (k.get("agpr_count") or 0) <= 64, (wpb, k["vgpr_count"], k.get("agpr_count"))


def test_geometry_is_the_rule_and_the_code_objects(built):
    """rtlws_fold_geometry at every border of the bin count and of the period count: the header's rule, the kernel of
    that block shape, never more than 64 KiB"""
    names = _kernels(built)
    sub, ntrials, nsamp = 64, 3, 1000
    shapes = set()
    for nbins in (2, 64, 65, 128, 129, 256):
        for nperiods in (1, 64, 65, 4096):
            rc, blocks, threads, lds, tile, wpb, nsub = built.fold_geometry(nperiods, nbins, sub, ntrials, nsamp)
            assert rc == 0 and built.fold_last_error() == "", (nbins, nperiods)
            assert (blocks, threads, lds, tile, wpb, nsub) == fold_ref.plan(nperiods, nbins, sub, ntrials, nsamp), (nbins, nperiods)
            assert wpb == (4 if nbins <= 64 else 2 if nbins <= 128 else 1) and lds == wpb * nbins * 256 <= 65536 and tile == 64
            assert threads == names[wpb]["max_flat_workgroup_size"] == 64 * wpb
            assert blocks == ntrials * -(-nperiods // (64 * wpb)) * 16 and nsub == 16
            shapes.add((wpb, lds))
    assert {w for w, _ in shapes} == {4, 2, 1} and max(l for _, l in shapes) == 65536 and (4, 2048) in shapes
    # nsub = ceil(nsamp / sub); the grid
    for sub in (64, 68, 1 << 24):
        for nsamp in (0, 1, sub - 1, sub, sub + 1, 5 * sub + 3, 1 << 30):
            for ntrials, nperiods in ((1, 1), (3, 65), (65536, 4096)):
                rc, blocks, _, _, _, _, nsub = built.fold_geometry(nperiods, 16, sub, ntrials, nsamp)
                want = ntrials * -(-nperiods // 256) * -(-nsamp // sub)
                if -(-nsamp // sub) > (2 ** 31 - 1) // (ntrials * -(-nperiods // 256)):
                    assert rc == -1 and "more workgroups than one grid holds" in built.fold_last_error()
                else:
                    assert (rc, nsub, blocks) == (0, -(-nsamp // sub), want), (sub, nsamp, ntrials)
    # any pointer behind nsamp may be null
    assert built.fold_lib().rtlws_fold_geometry(3, 16, 64, 1, 10, None, None, None, None, None, None) == 0


def test_fold_refusals_need_no_gpu(built):
    L = built.fold_lib()
    err = built.fold_last_error
    st, ph = _u64([1 << 60, 0, (1 << 64) - 1]), _u64([0, 5, 1 << 63])
    for nbins in (2, 3, 255, 256):
        for sub in (64, 68, 1 << 24):
            assert built.fold_supported(st, ph, nbins, sub) == 1 and err() == ""

    def each(nperiods=3, steps=st.ctypes.data, phases=ph.ctypes.data, nbins=16, sub=64):
        yield "rtlws_fold_open", not L.rtlws_fold_open(None, nperiods, steps, phases, nbins, sub), err()
        yield "rtlws_fold", L.rtlws_fold_supported(nperiods, steps, phases, nbins, sub) == 0, err()

    for kw, word in (({"nperiods": 0}, "nperiods must be 1 .. 4096"), ({"nperiods": 4097}, "nperiods must be"), ({"nperiods": -1}, "nperiods"),
                     ({"steps": None}, "null steps"), ({"phases": None}, "null phases"), ({"nbins": 1}, "nbins must be 2 .. 256"),
                     ({"nbins": 257}, "nbins must be"), ({"nbins": 0}, "nbins"), ({"sub": 63}, "sub must be 64 .. 16777216 and a multiple of 4"),
                     ({"sub": 60}, "sub must be"), ({"sub": 66}, "sub must be"), ({"sub": (1 << 24) + 4}, "sub must be"), ({"sub": 0}, "sub")):
        for fn, refused, why in each(**kw):
            assert refused and word in why and why.startswith(fn + ": "), (kw, fn, why)
    # the tables' rules in order: nperiods, the steps, the phases, nbins, sub
    chain = (({"nperiods": 0}, "nperiods"), ({"steps": None}, "null steps"), ({"phases": None}, "null phases"), ({"nbins": 1}, "nbins"),
             ({"sub": 0}, "sub must be"))
    for i, (_, word) in enumerate(chain):
        kw = {}
        for later, _ in reversed(chain[i:]):
            kw.update(later)
        for fn, refused, why in each(**kw):
            assert refused and word in why, (i, fn, why)
    # geometry: nperiods, nbins, sub, ntrials, nsamp, the grid, in that order
    def geo(**kw):
        return (L.rtlws_fold_geometry(kw.get("nperiods", 3), kw.get("nbins", 16), kw.get("sub", 64), kw.get("ntrials", 1), kw.get("nsamp", 5),
                                      None, None, None, None, None, None), err())
    assert geo() == (0, "")
    gchain = (({"nperiods": 0}, "nperiods must be"), ({"nbins": 300}, "nbins must be"), ({"sub": 62}, "sub must be"), ({"ntrials": 0}, "ntrials must be 1 .. 65536"),
              ({"nsamp": -1}, "nsamp must be 0 .. 2^30"))
    for i, (_, word) in enumerate(gchain):
        kw = {}
        for later, _ in reversed(gchain[i:]):
            kw.update(later)
        rc, why = geo(**kw)
        assert rc == -1 and word in why and why.startswith("rtlws_fold_geometry: "), (i, why)
    for kw, word in (({"ntrials": 65537}, "ntrials must be"), ({"nsamp": (1 << 30) + 1}, "nsamp must be"),
                     ({"ntrials": 65536, "nperiods": 4096, "nsamp": 1 << 30}, "more workgroups than one grid holds"),
                     ({"ntrials": 65536, "nperiods": 4096, "nsamp": (1 << 30) + 1}, "nsamp must be")):
        rc, why = geo(**kw)
        assert rc == -1 and word in why, (kw, why)
    h = L.rtlws_fold_open(None, 3, st.ctypes.data, ph.ctypes.data, 16, 64)
    assert not h and err() == "rtlws_fold_open: null engine (no usable HIP device: there is no CPU path)"
    with pytest.raises(RuntimeError):
        built.FoldPlan(None, st, ph, 16, 64)
    L.rtlws_fold_close(None)
    assert L.rtlws_fold_subints(None, 5) == -1 and "null plan" in err()
    assert L.rtlws_fold_subints(None, -1) == -1 and "nsamp must be 0 .. 2^30" in err()
    assert L.rtlws_fold_subints(None, (1 << 30) + 1) == -1 and "nsamp must be" in err()

    A, B, Cc = 1 << 20, 2 << 20, 3 << 20                      # stand-ins for device pointers: never dereferenced
    base = (("plan", None), ("din", A), ("istride", 104), ("ntrials", 2), ("nsamp", 100), ("prof", B), ("hits", Cc), ("st", None))

    def run(**kw):
        assert set(kw) <= {k for k, _ in base}
        return L.rtlws_fold_run(*[kw.get(k, v) for k, v in base]), err()

    for kw, word in (({"ntrials": 0}, "ntrials must be 1 .. 65536"), ({"ntrials": 65537}, "ntrials must be"), ({"nsamp": -1}, "nsamp must be 0 .. 2^30"),
                     ({"nsamp": (1 << 30) + 4, "istride": 1 << 31}, "nsamp must be"), ({"istride": 96}, "in_stride must be >= nsamp"),
                     ({"istride": 0}, "in_stride must be >="), ({"istride": 102}, "in_stride must be a multiple of 4"),
                     ({"din": None}, "null pointer"), ({"prof": None}, "null pointer"),
                     ({"din": A + 4}, "d_in must be 16-byte aligned"), ({"din": A + 8}, "d_in must be 16-byte"),
                     ({"prof": B + 2}, "d_prof must be 4-byte aligned"), ({"hits": Cc + 1}, "d_hits must be 4-byte aligned"),
                     ({}, "null plan"), ({"hits": None}, "null plan"),
                     ({"nsamp": 0, "din": None, "prof": None, "hits": None, "istride": 0}, "null plan"), ({"istride": 1 << 40}, "null plan")):
        rc, why = run(**kw)
        assert rc == -1 and word in why and why.startswith("rtlws_fold_run: "), (kw, why)
    # the order: a call that breaks rule i and every later rule it still can is refused for rule i
    chain = (({"ntrials": 0}, "ntrials"), ({"nsamp": -1}, "nsamp must be"), ({"istride": 2}, "in_stride must be >="), ({"istride": 102}, "multiple of 4"),
             ({"prof": None}, "null pointer"), ({"din": A + 4}, "d_in"), ({"prof": B + 2}, "d_prof"), ({"hits": Cc + 2}, "d_hits"), ({}, "null plan"))
    for i, (_, word) in enumerate(chain):
        kw = {}
        for later, _ in reversed(chain[i:]):
            kw.update(later)
        rc, why = run(**kw)
        assert rc == -1 and word in why, (i, kw, why)
    # the header's wording of the order names the same things in the same order
    txt = re.sub(r"\s+\*\s+", " ", open(os.path.join(INCLUDE, "rtlws_fold.h")).read())
    order = re.search(r"in this order: (.*?)0; -1 bad argument", txt, re.S).group(1)
    places = [order.index(word) for word in ("ntrials", "nsamp", "in_stride at least", "multiple of 4", "null pointers", "alignments", "null plan", "the grid")]
    assert places == sorted(places)
    # a refusal here leaves a sibling's error slot empty
    assert built.pulse_supported((1, 2), 64) == 1
    assert run(nsamp=-1)[0] == -1 and err() != "" and built.pulse_last_error() == ""


def test_step_is_the_fraction(built):
    """rtlws_fold_step equals round-half-up(2^64 / P) of the double's exact value"""
    rng = np.random.default_rng(17)
    periods = [2.0, 2.0 ** 32, 3.0, 37.3, 1e6 + 1.0 / 3.0, float(np.nextafter(2.0, 3.0)), float(np.nextafter(2.0 ** 32, 0.0)), 4.0, 2.5, 6.0,
               2.0 ** 32 / 3.0]
    periods += list(np.exp2(rng.uniform(1.0, 32.0, 1000)))
    for period in periods:
        assert 2.0 <= period <= 2.0 ** 32
        got, want = built.fold_step(period), fold_ref.step_of(period)
        assert got == want and built.fold_last_error() == "", (period, got, want)
        exact = Fraction(1 << 64) / Fraction(period)
        assert abs(Fraction(got) - exact) <= Fraction(1, 2)
    assert built.fold_step(2.0) == 1 << 63 and built.fold_step(2.0 ** 32) == 1 << 32 and built.fold_step(4.0) == 1 << 62
    for period in (1.999999, 0.0, -3.0, float(np.nextafter(2.0, 0.0)), float(np.nextafter(2.0 ** 32, np.inf)), 1e300, float("inf"), float("nan")):
        assert built.fold_step(period) == 0 and "the period must be 2 .. 2^32 samples" in built.fold_last_error(), period


def test_phase_at_wraps(built):
    M = 1 << 64
    rng = np.random.default_rng(3)
    cases = [(0, 0, 0), (1, M - 1, 1), (M - 1, M - 1, 1 << 30), (1 << 63, 1, 3), (1 << 63, 1, 4), (M - 1, 0, 2), (12345, 1 << 63, 1 << 30)]
    cases += [(int(a), int(b), int(n)) for a, b, n in zip(rng.integers(0, M, 200, dtype=np.uint64), rng.integers(0, M, 200, dtype=np.uint64),
                                                           rng.integers(0, 1 << 30, 200))]
    for step, phi0, n0 in cases:
        assert built.fold_phase_at(step, phi0, n0) == (phi0 + n0 * step) % M == fold_ref.phase_at(step, phi0, n0), (step, phi0, n0)
    assert built.fold_phase_at(1, M - 1, 1) == 0 and built.fold_phase_at(1 << 63, 0, 2) == 0


def test_chi2_is_the_expression(built):
    """rtlws_fold_chi2 against the same expression in numpy f64 to 1e-12 relative (as rtlws_pulse_snr's test); its NaNs"""
    rng = np.random.default_rng(5)
    worst = 0.0
    for trial in range(200):
        nbins = int(rng.integers(2, 257))
        hits = rng.integers(1, 2000, nbins).astype(np.uint32)
        count = int(hits.sum())
        mean = rng.uniform(0.5, 50.0) * rng.choice([-1.0, 1.0])
        sigma = abs(mean) * rng.uniform(0.5, 2.0)
        sum1, sum2 = mean * count, (sigma * sigma + mean * mean) * count
        prof = (hits * mean + rng.standard_normal(nbins) * sigma * np.sqrt(hits) * rng.uniform(1.0, 5.0)).astype(np.float32)
        got, want = built.fold_chi2(prof, hits, sum1, sum2, count), float(fold_ref.chi2(prof, hits, sum1, sum2, count))
        assert math.isfinite(want) and want > 0 and abs(got - want) <= 1e-12 * abs(want), (trial, got, want)
        worst = max(worst, abs(got - want) / abs(want))
    print("rtlws_fold_chi2: at most %.3g relative from the numpy expression" % worst)
    # mean 1, var 2: ((5 - 4)^2 + (2 - 4)^2) / (4 * 2)
    assert built.fold_chi2([5.0, 2.0], [4, 4], 8.0, 24.0, 8) == (1.0 + 4.0) / 8.0
    nan = float("nan")
    for args in (([5.0, 2.0], [4, 4], 8.0, 24.0, 1), ([5.0, 2.0], [4, 4], 8.0, 24.0, 0), ([5.0, 2.0], [4, 4], 8.0, 8.0, 8), ([5.0, 2.0], [4, 4], 8.0, 7.0, 8),
                 ([5.0, 2.0], [4, 0], 8.0, 24.0, 8), ([5.0, 2.0], [0, 4], 8.0, 24.0, 8), ([5.0, 2.0], [4, 4], nan, 24.0, 8), ([5.0, 2.0], [4, 4], 8.0, nan, 8)):
        assert math.isnan(built.fold_chi2(*args)) and math.isnan(fold_ref.chi2(*args)), args
    assert math.isnan(built.fold_chi2([nan, 2.0], [4, 4], 8.0, 24.0, 8)) and math.isnan(built.fold_chi2([], [], 8.0, 24.0, 8))
    assert math.isnan(built.fold_lib().rtlws_fold_chi2(None, None, 2, 8.0, 24.0, 8))


# ---- the yardstick's own properties ---------------------------------------------------------------------------

def _case(nsamp=3000, nbins=16, seed=1):
    x = fold_ref.signed_series(1, nsamp, seed)
    return x, fold_ref.step_of(37.3), 0x9E3779B97F4A7C15, nbins


def test_restatement_is_the_plain_loop():
    x, step, phi0, nbins = _case()
    expo = np.frexp(x)[1]
    assert x.dtype == np.float32 and expo.max() - expo.min() == 12                     # 2^-6 .. 2^6
    for sub, nsamp in ((3000, 3000), (64, 517), (68, 1), (1 << 24, 700)):
        prof, hits = fold_ref.fold_ref(x, [step], [phi0], nbins, sub, nsamp)
        assert prof.shape == (1, 1, -(-nsamp // sub), nbins) and hits.shape == prof.shape[1:] and hits.dtype == np.uint32
        for s in range(prof.shape[2]):
            n0, n1 = s * sub, min((s + 1) * sub, nsamp)
            acc, count = fold_ref.fold_by_the_letter(x[0, n0:n1], step, fold_ref.phase_at(step, phi0, n0), nbins)
            assert np.array_equal(prof[0, 0, s].view(np.uint32), acc.view(np.uint32)) and np.array_equal(hits[0, s], count), (sub, s)
            assert hits[0, s].sum() == n1 - n0
    # several trials and periods at once: each its own loop
    x3 = fold_ref.signed_series(3, 517, seed=2)
    steps, phases = fold_ref.table(5, seed=3)
    prof, hits = fold_ref.fold_ref(x3, steps, phases, 7, 100, 517)
    for t in range(3):
        for p in range(5):
            for s in range(6):
                n0, n1 = s * 100, min((s + 1) * 100, 517)
                acc, count = fold_ref.fold_by_the_letter(x3[t, n0:n1], steps[p], fold_ref.phase_at(steps[p], phases[p], n0), 7)
                assert np.array_equal(prof[t, p, s].view(np.uint32), acc.view(np.uint32)) and np.array_equal(hits[p, s], count)
    # the bins: integers only, 0 .. nbins - 1, and wrap-around is silent and exact
    b = fold_ref.bins_of((1 << 64) - 1, 5, 256, 0, 10)
    assert list(b) == [0, 0, 0, 0, 0, 0, 255, 255, 255, 255]
    assert list(fold_ref.bins_of(1 << 63, 1 << 62, 4, 0, 4)) == [1, 3, 1, 3] and list(fold_ref.bins_of(0, (1 << 64) - 1, 5, 7, 9)) == [4, 4]


def test_the_order_is_not_idle():
    """on signed data with exponents over 2^-6 .. 2^6 the reversed order and the sum of 64-sample partial profiles change the
    bits of most bins: a kernel that reorders is caught"""
    x, step, phi0, nbins = _case()
    want, _ = fold_ref.fold_by_the_letter(x[0], step, phi0, nbins)
    rev, _ = fold_ref.fold_by_the_letter(x[0], step, phi0, nbins, order=range(2999, -1, -1))
    part = fold_ref.fold_partials(x[0], step, phi0, nbins, 64)
    differ_rev = int((want.view(np.uint32) != rev.view(np.uint32)).sum())
    differ_part = int((want.view(np.uint32) != part.view(np.uint32)).sum())
    print("3000 samples into 16 bins: reversed differs in %d bins, 64-sample partials in %d" % (differ_rev, differ_part))
    assert differ_rev >= 8 and differ_part >= 8
    assert np.allclose(want, rev, rtol=0, atol=1e-2) and np.allclose(want, part, rtol=0, atol=1e-2)      # the same sums, other roundings


def test_translation():
    """a run over the samples from s0 sub on with phi0 replaced by phase(s0 sub): the whole run's sub-integrations s0 .."""
    x = fold_ref.signed_series(2, 1000, seed=4)
    steps, phases = fold_ref.table(9, seed=5)
    steps[3], steps[4], steps[5] = 0, 1 << 63, (1 << 64) - 1
    for sub in (64, 68, 300):
        whole = fold_ref.fold_ref(x, steps, phases, 13, sub, 1000)
        for s0 in (1, 2, 3):
            later = [fold_ref.phase_at(st, ph, s0 * sub) for st, ph in zip(steps, phases)]
            tail = fold_ref.fold_ref(x[:, s0 * sub:], steps, later, 13, sub, 1000 - s0 * sub)
            assert np.array_equal(tail[0].view(np.uint32), whole[0][:, :, s0:].view(np.uint32)) and np.array_equal(tail[1], whole[1][:, s0:])


def test_fold_ref_reads_nothing_behind_nsamp():
    x = np.full((2, 160), np.nan, np.float32)
    x[:, :150] = fold_ref.signed_series(2, 150, seed=6)
    steps, phases = fold_ref.table(3, seed=7)
    prof, hits = fold_ref.fold_ref(x, steps, phases, 5, 64, 150)
    assert prof.shape == (2, 3, 3, 5) and np.isfinite(prof).all() and np.all(hits.sum(axis=2) == np.array([64, 64, 22])[None, :])
    # one NaN and one +Inf sample each reach one bin per period and no other
    x[0, 70], x[1, 10] = np.nan, np.inf
    prof, _ = fold_ref.fold_ref(x, steps, phases, 5, 64, 150)
    assert np.all(np.isnan(prof[0]).sum(axis=2) == np.array([0, 1, 0])[None, :]) and np.all(np.isinf(prof[1]).sum(axis=2) == np.array([1, 0, 0])[None, :])
    assert not np.isnan(prof[1]).any() and not np.isinf(prof[0]).any()

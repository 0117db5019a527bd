"""CPU suite of include/rtlws_cdd.h: the restatement's overlap-save convention (tests/cdd_ref.py against a direct linear
convolution), and what the library does without a GPU: the chirp and the overlap helpers, its exports, the rules at
every limit and the order of a run's refusals, the binding's place beside the pinned surface, the new sources'
preprocessor lines and the kernels' registers and LDS."""
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np
import pytest

import cdd_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "rtl-ws_amd", "csrc")
NEW_SOURCES = [os.path.join(CSRC, f) for f in ("cdd.h", "cdd.hip", "cdd_shim.hip", "search_plan.h")] + [os.path.join(ROOT, "include", "rtlws_cdd.h")]


@pytest.fixture(scope="module")
def cdd(built):
    import rtlws.cdd
    return rtlws.cdd


# ---- the restatement ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("lead,trail", [(5, 11), (0, 0)])
def test_overlap_save_is_the_linear_convolution(lead, trail):
    """H the transform of a short FIR h[d], d = -trail .. lead (h[d] at point d mod N): output i of the restatement is
    sum_d h[d] x[i + lead - d], the linear convolution, at every output of three segments"""
    n, nseg = 512, 3
    rng = np.random.default_rng(100 + lead)
    hop = n - lead - trail
    taps = rng.standard_normal(lead + trail + 1) + 1j * rng.standard_normal(lead + trail + 1)      # taps[d + trail]
    imp = np.zeros(n, np.complex128)
    for d in range(-trail, lead + 1):
        imp[d % n] = taps[d + trail]
    need = cdd_ref.samples_needed(n, lead, trail, nseg)
    x = rng.standard_normal((2, need)) + 1j * rng.standard_normal((2, need))
    got = cdd_ref.cdd(x, np.stack([np.fft.fft(imp)] * 2), lead, trail, nseg)
    assert got.shape == (2, nseg * hop)
    want = np.zeros_like(got)
    for d in range(-trail, lead + 1):
        want += taps[d + trail] * x[:, lead - d:lead - d + nseg * hop]
    assert np.abs(got - want).max() <= 1e-12


def test_the_power_rows_are_the_headers_order():
    v = (np.arange(24, dtype=np.float32).reshape(2, 12) * np.float32(1.1) + 1j * np.float32(0.7)).astype(np.complex64)
    p = (v.real * v.real + v.imag * v.imag).astype(np.float32)
    want = (np.float32(0.0) + p[:, 0::3]) + p[:, 1::3]
    want = want + p[:, 2::3]
    assert np.array_equal(cdd_ref.power_rows(v, 3).view(np.uint32), want.view(np.uint32))
    assert np.array_equal(cdd_ref.power_rows(v, 1).view(np.uint32), p.view(np.uint32))


def test_the_bound_is_the_derivation():
    """B = (1 + b)^2 (1 + sqrt 2 gamma_3) - 1 with b = t eta / (1 - t eta): about (2 t 6.66 + 4.24) u"""
    for t in range(9, 15):
        eta = cdd_ref.U + 4 * cdd_ref.U / (1 - 4 * cdd_ref.U) * (math.sqrt(2.0) + cdd_ref.U)
        b = t * eta / (1 - t * eta)
        assert cdd_ref.bound(t) == (1 + b) ** 2 * (1 + math.sqrt(2.0) * cdd_ref.gamma(3)) - 1
        assert abs(cdd_ref.bound(t) / cdd_ref.U - (2 * t * 6.657 + 4.243)) < 0.05


# ---- the host helpers ---------------------------------------------------------------------------------------------

CHIRPS = [(9, 1400.0, 1.0, 50.0), (12, 400.0, 2.0, 26.7), (14, 327.0, -0.5, 10.0), (10, 1400.0, 8.0, 300.0)]


@pytest.mark.parametrize("log2n,f0,rate,dm", CHIRPS)
def test_chirp_against_extended_precision(cdd, log2n, f0, rate, dm):
    got = cdd.chirp(log2n, f0, rate, dm)
    re, im = cdd_ref.chirp(log2n, f0, rate, dm)
    assert got.dtype == np.complex64 and got.shape == (1 << log2n,)
    assert np.abs(got.real.astype(np.longdouble) - re).max() <= 2.0 ** -24
    assert np.abs(got.imag.astype(np.longdouble) - im).max() <= 2.0 ** -24
    flat = cdd.chirp(log2n, f0, rate, 0.0)
    assert np.all(flat.real == 1.0) and np.all(flat.imag == 0.0)


@pytest.mark.parametrize("rate", [1.0, -1.0])
def test_chirp_group_delay(cdd, rate):
    """the dispersion the table undoes is e^(+i theta), theta = -arg H: its group delay -(1 / 2 pi) d theta / d f is
    D DM ((f0 + f)^-2 - f0^-2) microseconds, by central differences of the unwrapped phase in mid-band"""
    log2n, f0, dm = 12, 400.0, 5.0
    n = 1 << log2n
    h = cdd.chirp(log2n, f0, rate, dm).astype(np.complex128)
    order = np.argsort(np.where(np.arange(n) < n // 2, np.arange(n), np.arange(n) - n) * rate, kind="stable")
    f = (np.where(np.arange(n) < n // 2, np.arange(n), np.arange(n) - n) * rate / n)[order]
    theta = np.unwrap(-np.angle(h[order]))
    mid = slice(n // 4, 3 * n // 4)
    delay = -(theta[2:] - theta[:-2]) / (f[2:] - f[:-2]) / (2.0 * np.pi)
    want = cdd_ref.DISPERSION * dm * ((f0 + f[1:-1]) ** -2.0 - f0 ** -2.0)
    # the delay crosses zero at f = 0, so "relative" is to the largest delay of the span (162 us at f = +-0.25 MHz).  What
    # the test must leave room for: the table's f32 rounding moves a phase by up to 2^-24 rad, a difference over 2 / N MHz
    # by 2^-24 N / (4 pi) = 1.9e-5 us, and the central difference itself errs by (rate / N)^2 K / f0^4 = 5e-8 us
    assert np.abs(want[mid]).max() > 150.0
    assert np.abs(delay[mid] - want[mid]).max() <= 1e-6 * np.abs(want[mid]).max()


def test_chirp_undoes_dispersion_of_an_impulse(cdd):
    log2n, f0, rate, dm = 12, 400.0, 2.0, 26.7
    n = 1 << log2n
    k = np.arange(n)
    f = np.where(k < n // 2, k, k - n) * rate / n
    theta = 2.0 * np.pi * cdd_ref.DISPERSION * dm * f * f / (f0 * f0 * (f0 + f))
    x = np.zeros(n, np.complex128)
    x[100] = 1.0
    dispersed = np.fft.ifft(np.fft.fft(x) * np.exp(1j * theta))
    assert np.abs(dispersed).max() < 0.5                                     # it was smeared
    back = np.fft.ifft(np.fft.fft(dispersed) * cdd.chirp(log2n, f0, rate, dm).astype(np.complex128))
    assert np.abs(back - x).max() <= 1e-6


def test_chirp_refusals(cdd):
    L = cdd.lib()
    buf = (C.c_float * (2 << 14))()
    for args, text in (((8, 400.0, 1.0, 1.0), "log2_nfft"), ((15, 400.0, 1.0, 1.0), "log2_nfft"), ((9, float("nan"), 1.0, 1.0), "finite"),
                       ((9, 400.0, float("inf"), 1.0), "finite"), ((9, 400.0, 1.0, float("nan")), "finite"), ((9, 400.0, 0.0, 1.0), "rate_mhz"),
                       ((9, 0.5, 1.0, 1.0), "lower edge"), ((9, 0.5, -1.0, 1.0), "lower edge"), ((9, -400.0, 1.0, 1.0), "lower edge"),
                       ((9, 400.0, 1.0, -1.0), "dm must be >= 0")):
        assert L.rtlws_cdd_chirp(*args, buf) == -1 and text in cdd.last_error(), (args, cdd.last_error())
        with pytest.raises(ValueError):
            cdd.chirp(*args)
    assert L.rtlws_cdd_chirp(9, 400.0, 1.0, 1.0, None) == -1 and "null table" in cdd.last_error()
    assert L.rtlws_cdd_chirp(9, 400.0, 1.0, 1.0, buf) == 0 and cdd.last_error() == ""


def test_overlap(cdd):
    """against the expression in Python doubles; no tau of these within 1e-9 of an integer"""
    for f0, rate, dm in ((1400.0, 1.0, 50.0), (400.0, 2.0, 26.7), (327.0, -0.5, 10.0), (1400.0, 8.0, 300.0), (150.0, 0.2, 3.0)):
        half = abs(rate) / 2
        late, early = cdd_ref.delay_samples(f0, rate, dm, -half), -cdd_ref.delay_samples(f0, rate, dm, half)
        assert late > early > 0 and all(abs(v - round(v)) > 1e-9 for v in (late, early))
        assert cdd.overlap(f0, rate, dm) == (math.ceil(early), math.ceil(late)) == cdd_ref.overlap(f0, rate, dm)
    assert cdd.overlap(400.0, 1.0, 0.0) == (0, 0)
    L = cdd.lib()
    a, b = C.c_int(), C.c_int()
    assert L.rtlws_cdd_overlap(400.0, 1.0, 1.0, None, C.byref(b)) == -1 and "null pointer" in cdd.last_error()
    assert L.rtlws_cdd_overlap(0.5, 1.0, 1.0, C.byref(a), C.byref(b)) == -1 and "lower edge" in cdd.last_error()
    assert L.rtlws_cdd_overlap(1.0, 1.0, 1e9, C.byref(a), C.byref(b)) == -1 and "2^30" in cdd.last_error()
    with pytest.raises(ValueError):
        cdd.overlap(400.0, 1.0, -1.0)


# ---- the library without a GPU ------------------------------------------------------------------------------------

def test_exports_are_the_header(cdd):
    import test_abi_cpu
    declared = test_abi_cpu._declared_functions("rtlws_cdd.h")
    assert len(declared) == 9 and set(declared) == set(cdd.SYMBOLS)
    assert test_abi_cpu._exported(cdd.CDD_LIB) == set(declared)
    L = cdd.lib()
    assert all(getattr(L, f).argtypes is not None for f in cdd.SYMBOLS)


# (log2_nfft, lead, trail, nchan, ksum) -> served
LIMITS = [
    ((8, 0, 0, 1, 0), False), ((9, 0, 0, 1, 0), True), ((14, 0, 0, 1, 0), True), ((15, 0, 0, 1, 0), False),
    ((9, -1, 0, 1, 0), False), ((9, 0, -1, 1, 0), False),
    ((9, 500, 12, 1, 0), False), ((9, 500, 11, 1, 0), True), ((9, 0, 512, 1, 0), False), ((9, 0, 511, 1, 1), True), ((14, 16383, 0, 1, 1), True),
    ((14, 8192, 8192, 1, 0), False), ((9, 1 << 30, 1 << 30, 1, 0), False),
    ((9, 5, 11, 0, 0), False), ((9, 5, 11, 1, 0), True), ((9, 5, 11, 1024, 0), True), ((9, 5, 11, 1025, 0), False),
    ((9, 5, 11, 1, -1), False), ((9, 5, 11, 1, 496), True), ((9, 5, 11, 1, 497), False), ((9, 5, 11, 1, 16), True), ((9, 5, 11, 1, 3), False),
    ((9, 5, 12, 1, 3), True), ((9, 5, 12, 1, 165), True), ((9, 5, 12, 1, 2), False),
]


def test_the_rules_at_every_limit(cdd):
    for args, served in LIMITS:
        assert bool(cdd.supported(*args)) == served, args
        why = cdd_ref.why_not(*args)
        assert (why is None) == served and cdd.last_error() == ("" if served else "rtlws_cdd: " + why), (args, cdd.last_error())
        got = cdd.geometry(*args, nseg=3)
        assert (got[0] == 0) == served, args
        if served:
            log2n = args[0]
            assert got[1:] == (3 * args[3], max(64, (1 << log2n) // 16), 8 * ((1 << log2n) + (1 << log2n) // 16)), args
    assert cdd.geometry(9, 5, 11, 1024, 0, nseg=1 << 20)[:2] == (0, 1 << 30)
    assert cdd.geometry(9, 5, 11, 1, 0, nseg=0)[:2] == (0, 0)
    for nseg in (-1, (1 << 20) + 1):
        assert cdd.geometry(9, 5, 11, 1, 0, nseg=nseg)[0] == -1 and cdd.last_error() == "rtlws_cdd_geometry: nseg must be 0 .. 1048576"
    assert cdd.geometry(14, 0, 0, 1, 0)[1:] == (1, 1024, 136 * 1024)
    assert cdd.lib().rtlws_cdd_geometry(9, 5, 11, 1, 0, 1, None, None, None) == 0


def test_open_without_an_engine(cdd):
    tables = np.ones((1, 512), np.complex64)
    with pytest.raises(RuntimeError, match="rtlws_cdd_open: null engine"):
        cdd.CddPlan(None, 9, 5, 11, 1, 0, tables)
    with pytest.raises(RuntimeError, match="rtlws_cdd_open: log2_nfft must be 9 .. 14"):          # the arguments come first
        cdd.CddPlan(None, 8, 5, 11, 1, 0, np.ones((1, 256), np.complex64))
    with pytest.raises(RuntimeError, match="rtlws_cdd_open: ksum must divide hop"):
        cdd.CddPlan(None, 9, 5, 11, 1, 3, tables)
    with pytest.raises(RuntimeError, match="rtlws_cdd_open: null tables"):                        # ... and the table before the engine
        cdd.CddPlan(None, 9, 5, 11, 1, 0, None)
    L = cdd.lib()
    assert L.rtlws_cdd_samples_needed(None, 1) == -1 and "null plan" in cdd.last_error()
    L.rtlws_cdd_close(None)
    # a run's refusals that need no plan come before the null plan's, in the header's order:
    # (d_in, in_stride, nseg, d_out, out_stride, layout)
    run = lambda *a: L.rtlws_cdd_run(None, *a, None)
    for args, text in (((64, 512, -1, 64, 512, 0), "nseg must be 0 .. 1048576"), ((64, 512, (1 << 20) + 1, 64, 512, 0), "nseg must be 0 .. 1048576"),
                       ((64, 512, 1, 64, 512, 2), "unknown layout"), ((64, 512, 1, 64, 512, -1), "unknown layout"),
                       ((None, 512, 1, 64, 512, 0), "null pointer"), ((64, 512, 1, None, 512, 0), "null pointer"),
                       ((68, 512, 1, 64, 512, 0), "d_in must be 8-byte aligned"), ((64, 512, 1, 66, 512, 0), "d_out must be 4-byte aligned"),
                       ((64, 512, 1, 68, 512, 0), "null plan"), ((64, 512, 0, 64, 512, 1), "null plan")):
        assert run(*args) == -1 and text in cdd.last_error(), (args, cdd.last_error())


def test_the_pinned_surface_holds_with_the_submodule(built, cdd):
    """tests/test_python_api_cpu.py's snapshot with rtlws.cdd imported: no new public name, no new Engine method, CddPlan
    no _Plan subclass"""
    import test_python_api_cpu as api
    rec, now = api._recorded(), api.snapshot(built)
    assert built.cdd is cdd
    for part in ("names", "functions", "methods"):
        assert now[part] == rec[part], part
    assert not issubclass(cdd.CddPlan, built._Plan) and issubclass(cdd.CddPlan, built._PlanBase)
    assert "cdd" not in api.SATELLITES
    assert "librtlws_cdd.so (include/rtlws_cdd.h)" in cdd.lib.__doc__
    assert {"supported", "geometry", "chirp", "overlap", "dedisperse", "CddPlan"} <= set(vars(cdd))


def test_the_new_sources_carry_no_conditionals():
    for path in NEW_SOURCES:
        lines = [ln.strip() for ln in open(path) if re.match(r"\s*#", ln)]
        other = [ln for ln in lines if not re.match(r"#\s*(include|pragma|define)\b", ln)]
        guards = [ln for ln in other if re.match(r"#\s*(ifndef RTLWS_\w+_H|endif\b|ifdef __cplusplus)", ln)]
        assert other == guards, (path, [ln for ln in other if ln not in guards])
        assert sum(ln.startswith("#ifndef") for ln in lines) == (0 if path.endswith(".hip") else 1), path


def test_no_kernel_of_the_library_spills(built, cdd):
    """the code object's metadata: one kernel per log2_nfft, no spill, no scratch, inside the 128 registers of the
    1024-thread workgroup, no static LDS (the tile is dynamic: at most 136 KiB of the 160 a compute unit has)"""
    from rtlws import codeobj
    mine = [k for k in codeobj.kernels(cdd.CDD_LIB) if "cdd_kernel" in k["name"]]
    assert len(mine) == 6
    for k in mine:
        assert not k["vgpr_spill_count"] and not k.get("sgpr_spill_count", 0) and not k["private_segment_fixed_size"], k["name"]
        assert k["vgpr_count"] <= 128 and k.get("agpr_count", 0) == 0, k["name"]
        assert k["group_segment_fixed_size"] <= 160 * 1024, k["name"]
    assert max(cdd.geometry(t, 0, 0, 1, 0)[3] for t in range(9, 15)) == 136 * 1024 <= 160 * 1024


def test_the_makefile_builds_it():
    txt = open(os.path.join(ROOT, "rtl-ws_amd", "Makefile")).read()
    assert re.search(r"^SATELLITES := .*\bcdd\b", txt, flags=re.M)
    out = subprocess.run(["nm", "-D", "--undefined-only", os.path.join(ROOT, "rtl-ws_amd", "lib", "librtlws_cdd.so")],
                         capture_output=True, text=True, check=True).stdout
    assert "rtlws_engine_device" in out and "rtlws_engine_stream" in out          # the engine is librtlws_hip.so's

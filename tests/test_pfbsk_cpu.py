"""CPU suite of include/rtlws_pfbsk.h (librtlws_pfbsk.so): the ABI, the kernels' resources from the code-object
metadata, sizes, the two host helpers and the refusals -- and the numpy restatement's own properties
(tests/pfbsk_ref.py), which hold the yardstick and the fixed cases of tests/test_pfbsk_gpu.py rather than the code under
test.  No GPU is used."""
import ctypes as C
import math
import re
import subprocess

import numpy as np
import pytest

import pfb_ref
import pfbsk_ref
import pfbspec_ref
from test_abi_cpu import _declared_functions, _exported

POWER, DB, PAYLOAD = pfbspec_ref.OUT_POWER_SUM, pfbspec_ref.OUT_MEAN_DB, pfbspec_ref.OUT_PAYLOAD_U8
INF, NAN = math.inf, math.nan


def test_pfbsk_library_exports_its_header_and_nothing_else(built):
    built.pfbsk_lib()
    declared = _declared_functions("rtlws_pfbsk.h")
    assert len(declared) == 9
    assert _exported(built.PFBSK_LIB) == set(declared) == set(built.PFBSK_SYMBOLS)
    dyn = subprocess.run(["readelf", "-d", built.PFBSK_LIB], capture_output=True, text=True, check=True).stdout
    assert "librtlws_hip.so" in dyn and "$ORIGIN" in dyn
    # the siblings export what they exported
    for lib, header in (("PFB_LIB", "rtlws_pfb.h"), ("PFBSPEC_LIB", "rtlws_pfbspec.h"), ("PFBXC_LIB", "rtlws_pfbxc.h"),
                        ("PFBBF_LIB", "rtlws_pfbbf.h")):
        assert _exported(getattr(built, lib)) == set(_declared_functions(header)), lib


def test_pfbsk_kernels_do_not_spill(built):
    """Every kernel of the library: no scratch, no spilled register, at most 128 VGPRs and AGPRs (four workgroups of 256
    per compute unit); the kernel names are exactly the instantiations the launch table reaches (log2 M = 4 .. 10, each
    for K below and K at least the tile's frames); the LDS is the channelizer's tile and rtlws_pfbsk_grid reports the code object's LDS and threads."""
    from rtlws import codeobj
    built.pfbsk_lib()
    ks = codeobj.kernels(built.PFBSK_LIB)
    names = {}
    for k in ks:
        d = k.get("demangled", k["name"])
        m = re.search(r"rtlws::pfbsk::pfbsk_kernel<(\d+), (false|true)>", d)
        assert m, d
        names[(int(m.group(1)), m.group(2) == "true")] = k
        assert k["vgpr_spill_count"] == 0 and k["private_segment_fixed_size"] == 0, d
        assert not k.get("sgpr_spill_count", 0), d
        assert k["vgpr_count"] + (k.get("agpr_count") or 0) <= 128, (d, k["vgpr_count"], k.get("agpr_count"))
    assert set(names) == {(k, w) for k in range(4, 11) for w in (False, True)} and len(ks) == 14
    for k in range(4, 11):
        for hop in (1 << k, 1 << (k - 1)):
            for k_avg, nsub in ((1, 1), (3, 7), (4096 >> k, 2), (65536, 65535)):
                kernel = names[(k, k_avg >= 4096 >> k)]
                rc, blocks, threads, lds, per = built.pfbsk_grid(k, 3, hop, k_avg, nsub, 5)
                assert rc == 0 and per >= 1 and blocks == -(-5 // per)
                assert threads == kernel["max_flat_workgroup_size"] == 256
                assert lds == kernel["group_segment_fixed_size"] == built.pfb_grid(k, 3, hop, 1)[3] == 34816, (k, lds)


def test_pfbsk_sizes_need_no_gpu(built):
    ok, need = built.pfbsk_supported, built.pfbsk_samples_needed
    for k in range(4, 11):
        for T in (1, 32):
            for hop in (1 << k, 1 << (k - 1)):
                for k_avg, nsub in ((1, 1), (7, 3), (65536, 65535)):
                    for out in (POWER, DB, PAYLOAD, "power", "db", "payload"):
                        assert ok(k, T, hop, k_avg, nsub, out) == 1 and built.pfbsk_last_error() == "", (k, T, hop, k_avg, nsub)
    # the shared rules in the family's words and order, then nsub, then the output
    for args, why in (((3, 0, 4, 0, 0, 3), "log2_channels must be 4 .. 10"), ((11, 1, 2048, 1, 1, 0), "log2_channels must be 4 .. 10"),
                      ((4, 0, 4, 0, 0, 3), "taps_per_branch must be 1 .. 32"), ((4, 33, 16, 1, 1, 0), "taps_per_branch must be 1 .. 32"),
                      ((6, 8, 48, 0, 0, 3), "hop must be M or M / 2"), ((6, 8, 16, 1, 1, 0), "hop must be M or M / 2"),
                      ((6, 8, 64, 0, 0, 3), "k_avg must be 1 .. 65536"), ((6, 8, 64, 65537, 1, 0), "k_avg must be 1 .. 65536"),
                      ((6, 8, 64, 1, 0, 3), "nsub must be 1 .. 65535"), ((6, 8, 64, 1, 65536, 0), "nsub must be 1 .. 65535"),
                      ((6, 8, 64, 1, -1, 0), "nsub must be 1 .. 65535"), ((6, 8, 64, 1, 1, 3), "unknown output"),
                      ((6, 8, 64, 1, 1, -1), "unknown output")):
        assert ok(*args) == 0 and built.pfbsk_last_error() == "rtlws_pfbsk: " + why, (args, built.pfbsk_last_error())
    assert built.pfbspec_supported(6, 8, 64, 0) == 0 and built.pfbspec_last_error() == "rtlws_pfbspec: k_avg must be 1 .. 65536"

    for k, T in ((4, 1), (6, 8), (10, 32)):
        M = 1 << k
        t = 4096 // M
        for hop in (M, M // 2):
            for k_avg in (1, 2, t - 1, t, t + 1, 2 * t + 3):
                for nsub in (1, 3, t + 1):
                    for n in (1, 2, 5):
                        want = (n * nsub * k_avg - 1) * hop + T * M
                        assert need(k, T, hop, k_avg, nsub, n) == want == pfbsk_ref.samples_needed(M, T, hop, k_avg, nsub, n)
                        assert want == built.pfbspec_samples_needed(k, T, hop, k_avg, n * nsub)
                    assert need(k, T, hop, k_avg, nsub, 0) == 0
    assert need(6, 8, 64, 65536, 65535, 3) == (3 * 65535 * 65536 - 1) * 64 + 512
    assert need(6, 8, 64, 1, 1, 1 << 40) == -1 and built.pfbsk_last_error().endswith("more spectra than one grid holds")
    assert need(6, 8, 64, 1, 1, -1) == -1 and built.pfbsk_last_error().endswith("nspectra must be >= 0")
    assert need(6, 8, 16, 1, 1, 1) == -1 and "hop" in built.pfbsk_last_error()
    assert need(6, 8, 64, 0, 1, 1) == -1 and "k_avg" in built.pfbsk_last_error()
    assert need(6, 8, 64, 1, 0, 1) == -1 and "nsub" in built.pfbsk_last_error()
    assert need(3, 8, 8, 1, 1, 1) == -1 and need(6, 33, 64, 1, 1, 1) == -1

    # the grid: whole rows per workgroup, the figure the library reports
    for k in (4, 6, 10):
        M = 1 << k
        for k_avg, nsub in ((1, 1), (1, 5), (3, 2), (4096 // M, 3), (65536, 65535)):
            per = built.pfbsk_grid(k, 8, M, k_avg, nsub, 1)[4]
            assert per >= 1
            for n in (0, 1, per, per + 1, 2 * per + 3, 1 << 27):
                rc, blocks, threads, lds, g = built.pfbsk_grid(k, 8, M // 2, k_avg, nsub, n)
                assert (rc, blocks, threads, g) == (0, -(-n // per), 256, per), (k, k_avg, nsub, n)
                assert lds == built.pfb_grid(k, 8, M, 1)[3]
        assert built.pfbsk_grid(k, 8, M, 1, 1, 1 << 62)[0] == -1 and "grid" in built.pfbsk_last_error()
        assert built.pfbsk_grid(k, 8, M, 1, 1, -1)[0] == -1 and "nspectra" in built.pfbsk_last_error()
    assert built.pfbsk_grid(3, 1, 8, 1, 1, 1)[0] == -1 and built.pfbsk_grid(6, 0, 64, 1, 1, 1)[0] == -1
    assert built.pfbsk_grid(6, 8, 63, 1, 1, 1)[0] == -1 and built.pfbsk_grid(6, 8, 64, 1, 0, 1)[0] == -1
    assert built.pfbsk_lib().rtlws_pfbsk_grid(6, 8, 64, 3, 2, 1, None, None, None, None) == 0


def test_pfbsk_refusals_need_no_gpu(built):
    L = built.pfbsk_lib()
    err = built.pfbsk_last_error
    # no engine, no plan: a text, never a crash
    taps = np.ones(64, np.int16)
    assert not L.rtlws_pfbsk_open(None, 6, 1, taps.ctypes.data) and err() == "rtlws_pfbsk_open: null engine (no usable HIP device: there is no CPU path)"
    assert not L.rtlws_pfbsk_open(None, 3, 1, taps.ctypes.data) and err() == "rtlws_pfbsk_open: log2_channels must be 4 .. 10"
    assert not L.rtlws_pfbsk_open(None, 6, 33, taps.ctypes.data) and err() == "rtlws_pfbsk_open: taps_per_branch must be 1 .. 32"
    assert not L.rtlws_pfbsk_open(None, 6, 1, None) and err() == "rtlws_pfbsk_open: null taps"
    with pytest.raises(RuntimeError):
        built.PfbSkPlan(None, 6, taps)
    with pytest.raises(RuntimeError):
        built.PfbSkPlan(None, 6, taps[:63])
    L.rtlws_pfbsk_close(None)

    A, B, K, S1, S2 = (i << 20 for i in range(1, 6))          # stand-ins for device pointers: never dereferenced
    base = (("plan", None), ("iq", A), ("n", 100), ("hop", 64), ("k", 3), ("nsub", 4), ("ps", 2.0 ** -40), ("lo", 1.25), ("hi", 1.8),
            ("output", DB), ("shifted", 0), ("scale", 1.0), ("clean", B), ("cstride", 64), ("kept", K), ("kstride", 64),
            ("s1", S1), ("s2", S2), ("sstride", 64), ("st", None))

    def run(**kw):
        assert set(kw) <= {k for k, _ in base}
        return L.rtlws_pfbsk_run(*[kw.get(k, d) for k, d in base]), err()

    for kw, word in (({"hop": 0}, "hop must be M or M / 2"), ({"hop": 48}, "hop"), ({"hop": 4}, "hop"), ({"hop": 2048}, "hop"),
                     ({"k": 0}, "k_avg must be 1 .. 65536"), ({"k": 65537}, "k_avg"),
                     ({"nsub": 0}, "nsub must be 1 .. 65535"), ({"nsub": -1}, "nsub"), ({"nsub": 65536}, "nsub"),
                     ({"output": 3}, "unknown output"), ({"shifted": 2}, "shifted must be 0 or 1"),
                     ({"scale": 0.0}, "scale must be finite and > 0"), ({"scale": NAN, "output": PAYLOAD}, "scale must be"),
                     ({"ps": 0.0}, "power_scale must be finite and > 0"), ({"ps": -1.0}, "power_scale"), ({"ps": INF}, "power_scale"),
                     ({"ps": NAN}, "power_scale"), ({"lo": -0.5}, "ratio bounds"), ({"lo": NAN}, "ratio bounds"),
                     ({"lo": INF, "hi": INF}, "ratio bounds"), ({"hi": NAN}, "ratio bounds"), ({"lo": 2.0, "hi": 1.0}, "ratio bounds"),
                     ({"hi": -INF}, "ratio bounds"),
                     ({"n": -1}, "nspectra must be >= 0"), ({"n": 1 << 62}, "more spectra than one grid holds"),
                     ({"cstride": 12}, "clean_stride must be >= M"), ({"cstride": 66}, "clean_stride must be a multiple of 4"),
                     ({"cstride": 72, "output": PAYLOAD}, "clean_stride must be a multiple of 16"),
                     ({"kstride": 12}, "kept_stride must be >= M"), ({"kstride": 66}, "kept_stride must be a multiple of 4"),
                     ({"sstride": 8}, "sub_stride must be >= M"), ({"sstride": 70}, "sub_stride must be a multiple of 4"),
                     ({"s1": None}, "d_s1 and d_s2 must both be given or both be null"), ({"s2": None}, "d_s1 and d_s2 must both"),
                     ({"iq": None}, "null pointer"), ({"clean": None}, "null pointer"), ({"iq": A + 8}, "d_iq_cu8 must be 16-byte"),
                     ({"clean": B + 4}, "d_clean must be 16-byte"), ({"kept": K + 4}, "d_kept must be 16-byte"),
                     ({"s1": S1 + 8}, "d_s1 and d_s2 must be 16-byte"), ({"s2": S2 + 4}, "d_s1 and d_s2 must be 16-byte"),
                     ({}, "null plan"), ({"output": POWER, "scale": NAN}, "null plan"), ({"hi": INF}, "null plan"),
                     ({"lo": 0.0, "hi": 0.0}, "null plan"), ({"kept": None, "kstride": 0}, "null plan"),
                     ({"s1": None, "s2": None, "sstride": 0}, "null plan"), ({"cstride": 80, "output": PAYLOAD}, "null plan"),
                     ({"n": 0, "iq": None, "clean": None}, "null plan")):
        rc, why = run(**kw)
        assert rc == -1 and word in why and why.startswith("rtlws_pfbsk_run: "), (kw, why)

    # the order: a call that breaks rule i and every later rule is refused for rule i
    chain = (({"hop": 48}, "hop"), ({"k": 0}, "k_avg"), ({"nsub": 0}, "nsub"), ({"output": 3}, "output"), ({"shifted": 2}, "shifted"),
             ({"scale": NAN}, "scale must"), ({"ps": NAN}, "power_scale"), ({"lo": NAN}, "ratio bounds"), ({"n": -1}, "nspectra"),
             ({"cstride": 8}, "clean_stride"), ({"kstride": 8}, "kept_stride"), ({"sstride": 8}, "sub_stride"),
             ({"s2": None}, "both"), ({"iq": None}, "null pointer"), ({"clean": B + 4}, "d_clean"), ({"kept": K + 4}, "d_kept"),
             ({"s1": S1 + 4}, "d_s1"), ({}, "null plan"))
    for i, (_, word) in enumerate(chain):
        kw = {}
        for later, _ in reversed(chain[i:]):
            kw.update(later)
        rc, why = run(**kw)
        assert rc == -1 and word in why, (i, kw, why)

    # a refusal here leaves the four siblings' error slots empty
    for name in ("pfb", "pfbspec", "pfbxc", "pfbbf"):
        assert getattr(built, name + "_supported")(6, 8, 64, *{"pfb": (), "pfbbf": ()}.get(name, (3,))) == 1
    assert run(nsub=0)[0] == -1 and err() != ""
    for name in ("pfb", "pfbspec", "pfbxc", "pfbbf"):
        assert getattr(built, name + "_last_error")() == "", name


def test_power_scale_is_the_formula(built):
    L = built.pfbsk_lib()
    cases = [(k, pfbspec_ref.designed_taps(k, T)) for k, T in ((4, 1), (6, 8), (10, 32), (10, 2))]
    cases += [(k, pfb_ref.random_taps(k, T, seed=k + T)) for k, T in ((4, 3), (7, 5), (10, 32))]
    one = np.zeros(64, np.int16)
    one[5] = -32768
    cases += [(6, one), (10, np.full(32 << 10, 32767, np.int16)), (10, np.full(32 << 10, -32768, np.int16)), (4, np.ones(16, np.int16))]
    for k, taps in cases:
        got = built.pfbsk_power_scale(k, taps)
        total = 128 * int(np.abs(taps.astype(np.int64)).sum())
        e = math.ceil(math.log2(total))
        assert 2 ** e >= total > 2 ** (e - 1)
        assert got == 2.0 ** (-2 * e) == pfbsk_ref.power_scale(taps), (k, taps.size, got)
        assert math.frexp(got)[0] == 0.5 and got == float(np.float32(got))             # a power of two, a float
    assert built.pfbsk_power_scale(6, np.zeros(128, np.int16)) == 1.0 == pfbsk_ref.power_scale(np.zeros(128))
    assert built.pfbsk_last_error() == ""
    t = np.ones(64, np.int16)
    assert L.rtlws_pfbsk_power_scale(3, 1, t.ctypes.data) == 0.0 and "log2_channels" in built.pfbsk_last_error()
    assert L.rtlws_pfbsk_power_scale(6, 33, t.ctypes.data) == 0.0 and "taps_per_branch" in built.pfbsk_last_error()
    assert L.rtlws_pfbsk_power_scale(6, 1, None) == 0.0 and built.pfbsk_last_error() == "rtlws_pfbsk_power_scale: null taps"
    with pytest.raises(RuntimeError):
        built.pfbsk_power_scale(3, t)


def test_power_scale_keeps_p_at_most_2_at_full_scale():
    """Every byte 0 or 255 under all-32767 taps (pfb_ref.full_scale_iq), and every byte 0, which puts re = im =
    -128 sum|h| on channel 0, the largest a capture can give: p = P scale <= 2, and more than 1 / 2 in the latter."""
    for k, T, D in ((4, 32, 16), (6, 8, 32), (10, 32, 1024)):
        M = 1 << k
        taps = np.full(T * M, 32767, np.int16)
        y = pfb_ref.pfb_ref(pfb_ref.full_scale_iq(pfb_ref.samples_needed(M, T, D, 6), seed=k), k, taps, D)
        p = (y.real ** 2 + y.imag ** 2) * pfbsk_ref.power_scale(taps)
        assert 0.0 < p.max() <= 2.0, (k, p.max())
        y = pfb_ref.pfb_ref(np.zeros((pfb_ref.samples_needed(M, T, D, 1), 2), np.uint8), k, taps, D)
        p = (y.real ** 2 + y.imag ** 2) * pfbsk_ref.power_scale(taps)
        assert np.argmax(p[0]) == 0 and 0.5 < p[0, 0] <= 2.0, (k, p[0, 0])
    assert np.isfinite(np.float32(65536.0) * np.float32(65536.0 * 4.0))                # K S2 at the largest K and p = 2


def test_bounds_are_the_formula(built):
    L = built.pfbsk_lib()
    for K in (2, 3, 64, 300, 65536):
        for lo, hi in ((0.0, 0.0), (0.5, 1.6), (0.0, INF), (0.77, 0.77), (1e-30, 1e30), (0.1, 1e300)):
            got = built.pfbsk_bounds(K, lo, hi)
            with np.errstate(over="ignore"):
                want = (np.float32(1.0 + lo * ((K - 1.0) / (K + 1.0))), np.float32(1.0 + hi * ((K - 1.0) / (K + 1.0))))
            assert np.float32(got[0]) == want[0] and np.float32(got[1]) == want[1], (K, lo, hi, got, want)
            assert want == pfbsk_ref.bounds(K, lo, hi)
    assert built.pfbsk_bounds(2, 0.5, 1.6) == (float(np.float32(1.0 + 0.5 / 3.0)), float(np.float32(1.0 + 1.6 / 3.0)))
    assert built.pfbsk_bounds(64, 0.0, INF) == (1.0, INF)
    assert L.rtlws_pfbsk_bounds(64, 0.5, 1.6, None, None) == 0 and built.pfbsk_last_error() == ""
    lo, hi = C.c_float(7.0), C.c_float(7.0)
    for K, a, b, word in ((1, 0.5, 1.6, "k_avg"), (0, 0.5, 1.6, "k_avg"), (65537, 0.5, 1.6, "k_avg"), (64, -0.1, 1.6, "sk_lo"),
                          (64, 1.7, 1.6, "sk_lo"), (64, NAN, 1.6, "sk_lo"), (64, 0.5, NAN, "sk_lo"), (64, NAN, NAN, "sk_lo")):
        assert L.rtlws_pfbsk_bounds(K, a, b, C.byref(lo), C.byref(hi)) == -1 and word in built.pfbsk_last_error(), (K, a, b)
        assert lo.value == hi.value == 7.0
    with pytest.raises(RuntimeError):
        built.pfbsk_bounds(1, 0.5, 1.6)


# ---- the yardstick's own properties ---------------------------------------------------------------------------

def test_reference_on_itself():
    k, T, K, L = 5, 4, 6, 3
    M = 1 << k
    taps = pfb_ref.random_taps(k, T, seed=1)
    scale = pfbsk_ref.power_scale(taps)
    for D in (M, M // 2):
        iq = pfb_ref.random_iq(pfbsk_ref.samples_needed(M, T, D, K, L, 4), seed=2)
        # L = 1 with open bounds is the spectrometer
        c, n, s1, s2 = pfbsk_ref.pfbsk_ref(iq, k, taps, K, 1, hop=D)
        short = pfbspec_ref.pfbspec_ref(iq, k, taps, K, D)
        assert c.shape == (4 * L, M) and np.array_equal(c, short) and np.array_equal(s1, short) and np.all(n == 1)
        # a row of L sub-integrations is the sum of the kept short rows, under open bounds and under bounds that flag
        r = pfbsk_ref.ratio(s1, s2, K, scale)
        assert np.all(r >= 1.0) and np.all(r <= K * (1 + 1e-12))                       # Cauchy-Schwarz, and its converse
        for lo, hi in (pfbsk_ref.OPEN, (float(np.median(r)), math.inf), (0.0, float(np.median(r)))):
            c, n, s1b, s2b = pfbsk_ref.pfbsk_ref(iq, k, taps, K, L, lo, hi, hop=D)
            assert np.array_equal(s1b, s1) and np.array_equal(s2b, s2)
            keep = ~((r < lo) | (r > hi))
            assert np.array_equal(n, keep.reshape(4, L, M).sum(axis=1))
            assert np.allclose(c, (short * keep).reshape(4, L, M).sum(axis=1), rtol=1e-14, atol=0.0)
            if (lo, hi) == pfbsk_ref.OPEN:
                assert np.all(n == L)
            else:
                assert 0 < (n < L).sum() and 0 < (n > 0).sum()
            sh = pfbsk_ref.pfbsk_ref(iq, k, taps, K, L, lo, hi, hop=D, shifted=True)
            assert all(np.array_equal(a, np.fft.fftshift(b, axes=1)) for a, b in zip(sh, (c, n, s1, s2)))
        # K = 1: the ratio is 1, in f64 up to roundings and in the f32 restatement exactly
        c, n, s1, s2 = pfbsk_ref.pfbsk_ref(iq, k, taps, 1, L, hop=D)
        assert np.abs(pfbsk_ref.ratio(s1, s2, 1, scale) - 1.0).max() <= 1e-15
        a = s1.astype(np.float32)
        b = (a * np.float32(scale)) * (a * np.float32(scale))
        assert not pfbsk_ref.flagged_f32(a, b, 1, scale, 1.0, 1.0).any()
        assert pfbsk_ref.flagged_f32(a, b, 1, scale, np.nextafter(np.float32(1), np.float32(2)), math.inf).all()
    # all-128 input: u = v = 0, kept under any bounds, +0
    mid = np.full((pfbsk_ref.samples_needed(M, T, M, K, L, 2), 2), 128, np.uint8)
    c, n, s1, s2 = pfbsk_ref.pfbsk_ref(mid, k, taps, K, L, 1.25, 1.8)
    assert not c.any() and not s1.any() and not s2.any() and np.all(n == L)
    z = np.zeros((2, M), np.float32)
    assert not pfbsk_ref.flagged_f32(z, z, K, scale, 1.25, math.inf).any()
    # the f32 clean sum is sequential and skips the flagged
    s = np.array([[1.0], [2.0 ** -24], [2.0 ** -24], [1.0], [3.0], [5.0]], np.float32)
    f = np.array([[False], [False], [False], [True], [False], [False]])
    c32, n32 = pfbsk_ref.clean_rows_f32(s, f, 3)
    assert c32.tolist() == [[1.0], [8.0]] and n32.tolist() == [[3], [2]]
    d = pfbsk_ref.db(np.array([4.0, 0.0, 8.0]), np.array([2, 0, 1]), 3.0, 3)
    assert d[1] == -np.inf and np.allclose(d[[0, 2]], [10 * np.log10(2.0), 10 * np.log10(8.0)], atol=1e-6)


@pytest.mark.parametrize("i", range(len(pfbsk_ref.SEMANTIC_SHAPES)))
def test_semantic_case_in_f64(i):
    """What the f64 reference alone must show on the semantic case: the steady tone's channel is flagged in every
    sub-integration (estimator near 0), the burst's channel in the two sub-integrations that hold a burst (estimator
    far above 1.6), and at most 2 % of all (q, c) have a ratio within 1 % of either bound."""
    k, T, D, K, L, iq, taps, scale, lo, hi = pfbsk_ref.semantic_case(i)
    M = 1 << k
    assert (lo, hi) == pfbsk_ref.bounds(K, 0.5, 1.6) and iq.shape[0] == pfbsk_ref.samples_needed(M, T, D, K, L, 2)
    c, n, s1, s2 = pfbsk_ref.pfbsk_ref(iq, k, taps, K, L, lo, hi, scale, D, nspectra=2)
    r = pfbsk_ref.ratio(s1, s2, K, scale)
    est = pfbsk_ref.estimator(r, K)
    flags = pfbsk_ref.flagged(s1, s2, K, scale, lo, hi)
    assert np.array_equal(flags, (r < lo) | (r > hi))
    tone, burst, where = pfbsk_ref.tone_channel(M), pfbsk_ref.burst_channel(M), list(pfbsk_ref.burst_subs(L))
    print("shape %d: estimator of the tone <= %.4f, of the bursts %s, %.2f %% near a bound, %.1f %% flagged"
          % (i, est[:, tone].max(), est[where, burst], 100 * pfbsk_ref.near_a_bound(r, lo, hi).mean(), 100 * flags.mean()))
    assert flags[:, tone].all() and est[:, tone].max() <= 0.01 and np.all(n[:, tone] == 0)
    assert flags[where, burst].all() and est[where, burst].min() >= 5.0
    assert np.all(n[:, burst] <= L - 1) and np.all(n[:, burst] >= 1)
    assert pfbsk_ref.near_a_bound(r, lo, hi).mean() <= 0.02
    assert 0.5 <= np.median(est) <= 1.5 and flags.mean() <= 0.2                       # noise reads 1 and is mostly kept


def test_db_cases_of_the_gpu_suite_stay_clear_of_the_integers():
    """The captures and scales of tests/test_pfbsk_gpu.py::test_db_and_bytes, from the f64 restatement alone: fewer than
    0.5 % of a case's finite values lie within 2e-3 of an integer, they lie inside the bytes' range, and channels with
    N = 0 and with N = L both occur."""
    for k, T, hop_div in pfbspec_ref.DB_SHAPES:
        for K in (3, (4096 >> k) + 1):
            iq, taps, D, scale, pscale, lo, hi = pfbsk_ref.db_case(k, T, hop_div, K)
            c, n, _, _ = pfbsk_ref.pfbsk_ref(iq, k, taps, K, pfbsk_ref.DB_NSUB, lo, hi, pscale, D, nspectra=pfbsk_ref.DB_ROWS)
            d = pfbsk_ref.db(c, n, scale, K)
            assert d.shape == (pfbsk_ref.DB_ROWS, 1 << k)
            assert np.array_equal(np.isneginf(d), n == 0) and (n == 0).any() and (n == pfbsk_ref.DB_NSUB).any()
            fin = d[n > 0]
            assert 20.0 <= fin.min() and fin.max() <= 120.0, (k, K, fin.min(), fin.max())
            assert pfbspec_ref.near_integer(fin, 2e-3).mean() < 0.005, (k, K)

"""CPU suite of include/rtlws_pfbspec.h (librtlws_pfbspec.so): the ABI, the kernels' resources from the code-object
metadata, sizes and refusals -- and the numpy restatement's own properties (tests/pfbspec_ref.py), which hold the
yardstick rather than the code under test.  No GPU is used."""
import re
import subprocess

import numpy as np
import pytest

import pfb_ref
import pfbspec_ref
from test_abi_cpu import _declared_by_lib, _declared_functions, _exported

POWER, DB, PAYLOAD = pfbspec_ref.OUT_POWER_SUM, pfbspec_ref.OUT_MEAN_DB, pfbspec_ref.OUT_PAYLOAD_U8


def test_pfbspec_library_exports_its_header_and_nothing_else(built):
    built.pfbspec_lib()
    declared = _declared_functions("rtlws_pfbspec.h")
    assert len(declared) == 7
    assert _exported(built.PFBSPEC_LIB) == set(declared)
    assert set(built.PFBSPEC_SYMBOLS) == set(declared)
    dyn = subprocess.run(["readelf", "-d", built.PFBSPEC_LIB], capture_output=True, text=True, check=True).stdout
    assert "librtlws_hip.so" in dyn and "$ORIGIN" in dyn
    # the existing libraries export what they exported
    for lib, names in _declared_by_lib().items():
        assert _exported(getattr(built, lib)) == set(names), lib
    for lib, header in (("FM_LIB", "rtlws_fm.h"), ("LONG_LIB", "rtlws_long.h"), ("ANYLEN_LIB", "rtlws_anylen.h"),
                        ("DDC_LIB", "rtlws_ddc.h"), ("FMBANK_LIB", "rtlws_fmbank.h"), ("PFB_LIB", "rtlws_pfb.h")):
        assert _exported(getattr(built, lib)) == set(_declared_functions(header)), lib


def test_pfbspec_kernels_do_not_spill(built):
    """Every kernel of the library: no scratch, no spilled register, at most 128 VGPRs (four workgroups of 256 per
    compute unit); the kernel names are exactly the instantiations the launch table reaches (one per log2 M =
    4 .. 10); rtlws_pfbspec_grid reports the code object's LDS and threads."""
    from rtlws import codeobj
    built.pfbspec_lib()
    ks = codeobj.kernels(built.PFBSPEC_LIB)
    names = {}
    for k in ks:
        d = k.get("demangled", k["name"])
        m = re.search(r"rtlws::pfbspec::pfbspec_kernel<(\d+)>", d)
        assert m, d
        names[int(m.group(1))] = k
        assert k["vgpr_spill_count"] == 0 and k["private_segment_fixed_size"] == 0, d
        assert not k.get("sgpr_spill_count", 0), d
        assert k["vgpr_count"] + (k.get("agpr_count") or 0) <= 128, (d, k["vgpr_count"])
    assert set(names) == set(range(4, 11)) and len(ks) == 7
    for k in range(4, 11):
        for hop in (1 << k, 1 << (k - 1)):
            for k_avg in (1, 3, 65536):
                rc, blocks, threads, lds, per = built.pfbspec_grid(k, 3, hop, k_avg, 1)
                assert rc == 0 and blocks == 1
                assert threads == names[k]["max_flat_workgroup_size"] == 256
                assert lds == names[k]["group_segment_fixed_size"] <= 40960, (k, lds)


def test_pfbspec_sizes_and_refusals_need_no_gpu(built):
    ok = built.pfbspec_supported
    for k in range(4, 11):
        for T in (1, 8, 32):
            for hop in (1 << k, 1 << (k - 1)):
                for k_avg in (1, 7, 65536):
                    for out in (POWER, DB, PAYLOAD, "power", "db", "payload"):
                        assert ok(k, T, hop, k_avg, out) == 1 and built.pfbspec_last_error() == "", (k, T, hop, k_avg, out)
    for k, T, hop, k_avg, out, word in ((3, 1, 8, 1, POWER, "log2_channels"), (11, 1, 2048, 1, POWER, "log2_channels"),
                                        (4, 0, 16, 1, POWER, "taps_per_branch"), (4, 33, 16, 1, POWER, "taps_per_branch"),
                                        (4, 1, 4, 1, POWER, "hop"), (6, 8, 48, 1, POWER, "hop"), (6, 8, 0, 1, POWER, "hop"),
                                        (6, 8, 64, 0, POWER, "k_avg"), (6, 8, 64, 65537, POWER, "k_avg"), (6, 8, 64, -1, POWER, "k_avg"),
                                        (6, 8, 64, 1, 3, "output"), (6, 8, 64, 1, -1, "output")):
        assert ok(k, T, hop, k_avg, out) == 0 and word in built.pfbspec_last_error(), (k, T, hop, k_avg, out)

    need = built.pfbspec_samples_needed
    for k, T in ((4, 1), (6, 8), (10, 32)):
        M = 1 << k
        t = 4096 // M
        for hop in (M, M // 2):
            for k_avg in (1, 2, t - 1, t, t + 1, 2 * t + 3):
                for n in (1, 2, t - 1, t, t + 1):
                    want = (n * k_avg - 1) * hop + T * M
                    assert need(k, T, hop, k_avg, n) == want == pfbspec_ref.samples_needed(M, T, hop, k_avg, n), (k, hop, k_avg, n)
                    assert want == built.pfb_samples_needed(k, T, hop, n * k_avg)
                assert need(k, T, hop, k_avg, 0) == 0
    assert need(6, 8, 64, 1, 1 << 36) == ((1 << 36) - 1) * 64 + 512
    assert need(6, 8, 64, 1, 1 << 40) == -1 and "grid" in built.pfbspec_last_error()
    assert need(6, 8, 64, 65536, (1 << 31) - 1) == (((1 << 31) - 1) * 65536 - 1) * 64 + 512
    assert need(6, 8, 64, 65536, 1 << 31) == -1 and "grid" in built.pfbspec_last_error()
    assert need(6, 8, 64, 1, -1) == -1 and "nspectra" in built.pfbspec_last_error()
    assert need(6, 8, 16, 1, 1) == -1 and "hop" in built.pfbspec_last_error()
    assert need(6, 8, 64, 0, 1) == -1 and "k_avg" in built.pfbspec_last_error()
    assert need(3, 8, 8, 1, 1) == -1 and need(6, 33, 64, 1, 1) == -1

    # the grid: whole spectra per workgroup, at the borders of a tile in K and in nspectra
    for k in (4, 6, 10):
        M = 1 << k
        t = built.pfb_grid(k, 8, M, 1)[4]
        assert t == 4096 // M
        for k_avg in (1, 2, 3, t - 1, t, t + 1, 2 * t + 3, 65536):
            per = 1 if k_avg >= t else t // k_avg
            for n in (0, 1, per - 1, per, per + 1, 2 * per + 3, 1 << 27):
                if n < 0:
                    continue
                rc, blocks, threads, lds, g = built.pfbspec_grid(k, 8, M // 2, k_avg, n)
                assert (rc, blocks, threads, g) == (0, -(-n // per), 256, per), (k, k_avg, n)
                assert lds == built.pfb_grid(k, 8, M, 1)[3]
        assert built.pfbspec_grid(k, 8, M, 1, 1 << 62)[0] == -1 and "grid" in built.pfbspec_last_error()
        assert built.pfbspec_grid(k, 8, M, t, 1 << 31)[0] == -1 and "grid" in built.pfbspec_last_error()
        assert built.pfbspec_grid(k, 8, M, 1, -1)[0] == -1 and "nspectra" in built.pfbspec_last_error()
    assert built.pfbspec_grid(3, 1, 8, 1, 1)[0] == -1 and built.pfbspec_grid(6, 0, 64, 1, 1)[0] == -1
    assert built.pfbspec_grid(6, 8, 63, 1, 1)[0] == -1 and built.pfbspec_grid(6, 8, 64, 0, 1)[0] == -1
    L = built.pfbspec_lib()
    assert L.rtlws_pfbspec_grid(6, 8, 64, 3, 1, None, None, None, None) == 0

    # no engine, no plan: a text, never a crash
    taps = np.ones(64, np.int16)
    assert not L.rtlws_pfbspec_open(None, 6, 1, taps.ctypes.data) and "no CPU path" in built.pfbspec_last_error()
    assert not L.rtlws_pfbspec_open(None, 3, 1, taps.ctypes.data) and "log2_channels" in built.pfbspec_last_error()
    assert not L.rtlws_pfbspec_open(None, 6, 33, taps.ctypes.data) and "taps_per_branch" in built.pfbspec_last_error()
    assert not L.rtlws_pfbspec_open(None, 6, 1, None) and "null taps" in built.pfbspec_last_error()
    with pytest.raises(RuntimeError):
        built.PfbSpecPlan(None, 6, taps)
    with pytest.raises(RuntimeError):
        built.PfbSpecPlan(None, 6, taps[:63])
    L.rtlws_pfbspec_close(None)

    # the refusals of rtlws_pfbspec_run that need no plan are made before the plan is asked for anything
    A, B = 1 << 20, 2 << 20                                   # stand-ins for device pointers: never dereferenced
    base = (("plan", None), ("iq", A), ("n", 100), ("hop", 64), ("k", 3), ("output", DB), ("shifted", 0), ("scale", 1.0),
            ("out", B), ("stride", 64), ("st", None))

    def run(**kw):
        assert set(kw) <= {k for k, _ in base}
        return L.rtlws_pfbspec_run(*[kw.get(k, d) for k, d in base]), built.pfbspec_last_error()

    for kw, word in (({"hop": 0}, "hop"), ({"hop": 48}, "hop"), ({"hop": 4}, "hop"), ({"hop": 2048}, "hop"), ({"hop": -64}, "hop"),
                     ({"k": 0}, "k_avg"), ({"k": -1}, "k_avg"), ({"k": 65537}, "k_avg"),
                     ({"output": 3}, "output"), ({"output": -1}, "output"), ({"shifted": 2}, "shifted"), ({"shifted": -1}, "shifted"),
                     ({"scale": 0.0}, "scale"), ({"scale": -1.0}, "scale"), ({"scale": float("inf")}, "scale"),
                     ({"scale": float("nan")}, "scale"), ({"scale": float("nan"), "output": PAYLOAD}, "scale"),
                     ({"n": -1}, "nspectra"), ({"n": 1 << 62}, "grid"), ({"n": 1 << 31, "k": 300}, "grid"),
                     ({"stride": 15}, "out_stride"), ({"stride": 12}, "out_stride"), ({"stride": 66}, "multiple of 4"),
                     ({"stride": 72, "output": PAYLOAD}, "multiple of 16"), ({"iq": None}, "null pointer"),
                     ({"out": None}, "null pointer"), ({"iq": A + 8}, "16-byte"), ({"out": B + 8}, "16-byte"),
                     ({"out": B + 4}, "16-byte"), ({}, "null plan"), ({"output": POWER, "scale": float("nan")}, "null plan"),
                     ({"stride": 16}, "null plan"), ({"stride": 80, "output": PAYLOAD}, "null plan"),
                     ({"n": 0, "iq": None, "out": None}, "null plan")):
        rc, why = run(**kw)
        assert rc == -1 and word in why and why.startswith("rtlws_pfbspec_run: "), (kw, why)

    # the order: a call that breaks rule i and every later rule is refused for rule i
    chain = (({"hop": 48}, "hop"), ({"k": 0}, "k_avg"), ({"output": 3}, "output"), ({"shifted": 2}, "shifted"),
             ({"scale": float("nan")}, "scale"), ({"n": -1}, "nspectra"), ({"stride": 8}, "out_stride"),
             ({"iq": None}, "null pointer"), ({"out": B + 4}, "16-byte"), ({}, "null plan"))
    for i, (_, word) in enumerate(chain):
        kw = {}
        for later, _ in reversed(chain[i:]):
            kw.update(later)
        rc, why = run(**kw)
        assert rc == -1 and word in why, (i, kw, why)


# ---- the yardstick's own properties ---------------------------------------------------------------------------

def test_reference_k1_is_the_channelizer_squared():
    k, T = 5, 4
    M = 1 << k
    taps = pfb_ref.random_taps(k, T, seed=1)
    for D in (M, M // 2):
        iq = pfb_ref.random_iq(pfb_ref.samples_needed(M, T, D, 9), seed=2)
        y = pfb_ref.pfb_ref(iq, k, taps, D)
        got = pfbspec_ref.pfbspec_ref(iq, k, taps, 1, D)
        assert got.shape == (9, M) and np.array_equal(got, y.real ** 2 + y.imag ** 2)
        assert np.abs(got - np.abs(y) ** 2).max() <= 1e-15 * got.max()
        # K frames: the sum of K rows of K = 1, and a capture that holds a part of a further group gives no row for it
        got3 = pfbspec_ref.pfbspec_ref(iq[:-1], k, taps, 3, D)
        assert got3.shape == (2, M)
        assert np.abs(got3 - got[:6].reshape(2, 3, M).sum(axis=1)).max() <= 1e-15 * got3.max()


def test_reference_rows_of_a_sub_capture_equal_rows_of_the_whole():
    k, T, K = 5, 4, 3
    M = 1 << k
    taps = pfb_ref.random_taps(k, T, seed=3)
    for D in (M, M // 2):
        iq = pfb_ref.random_iq(pfbspec_ref.samples_needed(M, T, D, K, 7), seed=4)
        whole = pfbspec_ref.pfbspec_ref(iq, k, taps, K, D)
        assert whole.shape == (7, M)
        for j0 in (1, 2, 5):                                   # j0 K odd among them: the sign rule does not reach the power
            assert np.array_equal(pfbspec_ref.pfbspec_ref(iq[j0 * K * D:], k, taps, K, D), whole[j0:])
        assert not np.array_equal(pfbspec_ref.pfbspec_ref(iq[D:], k, taps, K, D), whole[:6])
        assert np.array_equal(pfbspec_ref.pfbspec_ref(iq, k, taps, K, D, shifted=True), np.fft.fftshift(whole, axes=1))
        assert np.array_equal(pfbspec_ref.pfbspec_ref(iq, k, taps, K, D, shifted=True)[:, M // 2], whole[:, 0])


@pytest.mark.parametrize("k,T,c0", [(4, 1, 3), (6, 8, 5), (6, 8, 40), (8, 3, 129)])
def test_reference_full_scale_recipe_reads_0_db(k, T, c0):
    """An unquantised tone of amplitude A on a channel centre with scale = 1 / (A sum(h))^2 reads 0 dB in its channel
    at both hops and any K: the header's recipe with A = 128."""
    M = 1 << k
    taps = pfbspec_ref.designed_taps(k, T) if T > 1 else np.ones(M, np.int16)
    A = 128.0
    scale = 1.0 / (A * taps.astype(np.float64).sum()) ** 2
    for D in (M, M // 2):
        for K in (1, 5):
            x = A * np.exp(2j * np.pi * ((c0 * np.arange(pfbspec_ref.samples_needed(M, T, D, K, 2))) % M) / M)
            s = pfbspec_ref.spectrometer(x, k, taps, K, D)
            assert s.shape == (2, M)
            d = 10.0 * np.log10(s[:, c0] * scale / K)
            assert np.abs(d).max() <= 1e-9, d
            assert np.argmax(pfbspec_ref.spectrometer(x, k, taps, K, D, shifted=True)[0]) == (c0 + M // 2) % M


def test_reference_db_and_bytes():
    s = np.array([0.0, 1.0, 10.0, 1e3, 1e30])
    d = pfbspec_ref.db(s, 2.0, 2)
    assert d[0] == -np.inf and np.allclose(d[1:], [0.0, 10.0, 30.0, 300.0], atol=1e-12)
    assert list(pfbspec_ref.payload(d)) == [0, 0, 10, 30, 255]
    assert list(pfbspec_ref.payload([-3.5, -0.5, 0.999, 1.0, 254.999, 255.0, 255.5, np.inf, -np.inf])) == [0, 0, 0, 1, 254, 255, 255, 255, 0]
    assert list(pfbspec_ref.near_integer([1.0005, 1.002, 7.9995, -np.inf])) == [True, False, True, False]
    assert float(pfbspec_ref.lin_f32(1.0, 3)) == float(np.float32(1.0) / np.float32(3.0))
    assert pfbspec_ref.bound(6, 64) == (16 * 7 + 64 + 4) * 2.0 ** -24


def test_db_cases_of_the_gpu_suite_stay_clear_of_the_integers():
    """The captures and scales of tests/test_pfbspec_gpu.py::test_db_and_bytes, from the f64 restatement alone: the
    values span tens of dB below 120, and fewer than 0.5 % of a case's values lie within 2e-3 of an integer (the
    device may use the +-1 exception for 1 %)."""
    for k, T, hop_div in pfbspec_ref.DB_SHAPES:
        t = 4096 >> k
        for K in (3, t + 1):
            iq, taps, D, scale = pfbspec_ref.db_case(k, T, hop_div, K)
            d = pfbspec_ref.db(pfbspec_ref.pfbspec_ref(iq, k, taps, K, D, nspectra=pfbspec_ref.DB_NSPECTRA), scale, K)
            assert d.shape == (pfbspec_ref.DB_NSPECTRA, 1 << k)
            assert 20.0 <= d.min() and d.max() <= 120.0 and d.max() - d.min() >= 40.0, (k, K, d.min(), d.max())
            assert pfbspec_ref.near_integer(d, 2e-3).mean() < 0.005, (k, K)
            b = pfbspec_ref.payload(d)
            assert b.min() >= 20 and b.max() <= 119


def test_reference_selectivity_through_the_spectrometer(built):
    """pfb_ref.selectivity_case() as one row of K = 64: the thresholds of DESIGN.md 4.14."""
    k, T, c0, iq, boxcar = pfb_ref.selectivity_case()
    for taps, check in ((built.pfb_design(k, T), lambda x: x <= -40.0), (boxcar, lambda x: x >= -15.0)):
        row = pfbspec_ref.pfbspec_ref(iq, k, taps, 64)
        assert row.shape == (1, 1 << k)
        assert check(pfbspec_ref.leakage_db_of_row(row[0], c0))

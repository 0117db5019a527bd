"""CPU suite of include/rtlws_pfb.h (librtlws_pfb.so): the ABI, the kernels' resources from the code-object metadata,
the prototype design, the transform's table, sizes and refusals -- and the numpy restatement's own properties
(tests/pfb_ref.py), which hold the yardstick rather than the code under test.  No GPU is used."""
import re
import subprocess

import numpy as np
import pytest

import ddc_ref
import pfb_ref
from test_abi_cpu import _declared_by_lib, _declared_functions, _exported


def test_pfb_library_exports_its_header_and_nothing_else(built):
    built.pfb_lib()
    declared = _declared_functions("rtlws_pfb.h")
    assert len(declared) == 9
    assert _exported(built.PFB_LIB) == set(declared)
    assert set(built.PFB_SYMBOLS) == set(declared)
    dyn = subprocess.run(["readelf", "-d", built.PFB_LIB], capture_output=True, text=True, check=True).stdout
    assert "librtlws_hip.so" in dyn and "$ORIGIN" in dyn
    # the existing libraries export what they exported
    for lib, names in _declared_by_lib().items():
        assert _exported(getattr(built, lib)) == set(names), lib
    for lib, header in (("FM_LIB", "rtlws_fm.h"), ("LONG_LIB", "rtlws_long.h"), ("ANYLEN_LIB", "rtlws_anylen.h"),
                        ("DDC_LIB", "rtlws_ddc.h"), ("FMBANK_LIB", "rtlws_fmbank.h")):
        assert _exported(getattr(built, lib)) == set(_declared_functions(header)), lib


def test_pfb_kernels_do_not_spill(built):
    """Every kernel of the library: no scratch, no spilled register; the kernel names are exactly the instantiations
    the launch table reaches (one per log2 M = 4 .. 10); rtlws_pfb_grid reports the code object's LDS and threads."""
    from rtlws import codeobj
    built.pfb_lib()
    ks = codeobj.kernels(built.PFB_LIB)
    names = {}
    for k in ks:
        d = k.get("demangled", k["name"])
        m = re.search(r"rtlws::pfb::pfb_kernel<(\d+)>", d)
        assert m, d
        names[int(m.group(1))] = k
        assert k["vgpr_spill_count"] == 0 and k["private_segment_fixed_size"] == 0, d
        assert not k.get("sgpr_spill_count", 0), d
    assert set(names) == set(range(4, 11)) and len(ks) == 7
    for k in range(4, 11):
        for hop in (1 << k, 1 << (k - 1)):
            rc, blocks, threads, lds, tile = built.pfb_grid(k, 3, hop, 1)
            assert rc == 0 and blocks == 1 and tile << k <= 8192
            assert threads == names[k]["max_flat_workgroup_size"] == 256
            assert lds == names[k]["group_segment_fixed_size"] <= 65536, (k, lds)


@pytest.mark.parametrize("k,T", [(4, 1), (4, 8), (6, 8), (10, 32)])
def test_design_equals_the_numpy_expression(built, k, T):
    got = built.pfb_design(k, T)
    f = pfb_ref.design(k, T)
    assert got.dtype == np.int16 and got.shape == f.shape
    want = np.rint(f)
    near_tie = np.abs(np.abs(f - np.floor(f)) - 0.5) < 1e-6
    diff = np.abs(got - want)
    assert np.all(diff[~near_tie] == 0) and np.all(diff <= 1), np.argwhere(diff != 0)[:4]
    assert np.array_equal(got, got[::-1])
    assert got.max() <= 32767 and got.min() >= -32768
    if (k, T) == (6, 8):
        assert abs(int(got.astype(np.int64).sum()) - 2091722) <= 8, got.astype(np.int64).sum()


def test_design_and_twiddles_refuse(built):
    L = built.pfb_lib()
    assert L.rtlws_pfb_design(6, 8, None) == -1 and "null" in built.pfb_last_error()
    buf = np.zeros(64, np.int16)
    for k, T, word in ((3, 1, "log2_channels"), (11, 1, "log2_channels"), (4, 0, "taps_per_branch"), (4, 33, "taps_per_branch")):
        assert L.rtlws_pfb_design(k, T, buf.ctypes.data) == -1 and word in built.pfb_last_error(), (k, T)
    assert L.rtlws_pfb_twiddles(6, None) == -1 and "null" in built.pfb_last_error()
    assert L.rtlws_pfb_twiddles(3, buf.ctypes.data) == -1 and "log2_channels" in built.pfb_last_error()


@pytest.mark.parametrize("k", range(4, 11))
def test_twiddles_equal_numpy(built, k):
    """e^(-2 pi i j / M) from f64, rounded once: within one f32 rounding of numpy's (the two libms may differ in the
    last bit of the f64), the quadrant points exact."""
    got = built.pfb_twiddles(k)
    want = pfb_ref.twiddles(k)
    M = 1 << k
    assert got.shape == (M, 2) and got.dtype == np.float32
    assert np.abs(got.astype(np.float64) - want.astype(np.float64)).max() <= 2.0 ** -24
    assert tuple(got[0]) == (1.0, 0.0) and tuple(got[M // 4]) == (0.0, -1.0)
    assert tuple(got[M // 2]) == (-1.0, 0.0) and tuple(got[3 * M // 4]) == (0.0, 1.0)


def test_pfb_sizes_and_refusals_need_no_gpu(built):
    ok = built.pfb_supported
    for k in range(4, 11):
        for T in (1, 2, 8, 31, 32):
            for hop in (1 << k, 1 << (k - 1)):
                assert ok(k, T, hop) == 1 and built.pfb_last_error() == "", (k, T, hop)
    for k, T, hop, word in ((3, 1, 8, "log2_channels"), (11, 1, 2048, "log2_channels"), (-1, 1, 1, "log2_channels"),
                            (4, 0, 16, "taps_per_branch"), (4, 33, 16, "taps_per_branch"), (4, 1, 4, "hop"),
                            (4, 1, 32, "hop"), (6, 8, 48, "hop"), (6, 8, 0, "hop"), (6, 8, -64, "hop")):
        assert ok(k, T, hop) == 0 and word in built.pfb_last_error(), (k, T, hop)

    need = built.pfb_samples_needed
    for k, T, n in ((4, 1, 1), (6, 8, 100), (10, 32, 7)):
        M = 1 << k
        for hop in (M, M // 2):
            assert need(k, T, hop, n) == (n - 1) * hop + T * M == pfb_ref.samples_needed(M, T, hop, n)
        assert need(k, T, M, 0) == 0
    assert need(6, 8, 64, 1 << 36) == ((1 << 36) - 1) * 64 + 512
    assert need(6, 8, 64, 1 << 40) == -1 and "grid" in built.pfb_last_error()
    assert need(6, 8, 64, -1) == -1 and "nframes" in built.pfb_last_error()
    assert need(6, 8, 16, 1) == -1 and "hop" in built.pfb_last_error()
    assert need(3, 8, 8, 1) == -1 and need(6, 33, 64, 1) == -1

    # the grid at a tile border
    for k in (4, 6, 10):
        M = 1 << k
        rc, blocks, threads, lds, t = built.pfb_grid(k, 8, M, 1)
        assert rc == 0 and t >= 4 and t * M <= 8192
        for n, want in ((0, 0), (1, 1), (t - 1, 1), (t, 1), (t + 1, 2), (2 * t + 3, 3), (1 << 27, -(-(1 << 27) // t))):
            assert built.pfb_grid(k, 8, M // 2, n)[:2] == (0, want), (k, n)
        assert built.pfb_grid(k, 8, M, 1 << 62)[0] == -1 and "grid" in built.pfb_last_error()
        assert built.pfb_grid(k, 8, M, -1)[0] == -1 and "nframes" in built.pfb_last_error()
    assert built.pfb_grid(3, 1, 8, 1)[0] == -1 and built.pfb_grid(6, 0, 64, 1)[0] == -1 and built.pfb_grid(6, 8, 63, 1)[0] == -1
    L = built.pfb_lib()
    assert L.rtlws_pfb_grid(6, 8, 64, 1, None, None, None, None) == 0

    # no engine, no plan: a text, never a crash
    taps = np.ones(64, np.int16)
    assert not L.rtlws_pfb_open(None, 6, 1, taps.ctypes.data) and "no CPU path" in built.pfb_last_error()
    assert not L.rtlws_pfb_open(None, 3, 1, taps.ctypes.data) and "log2_channels" in built.pfb_last_error()
    assert not L.rtlws_pfb_open(None, 6, 33, taps.ctypes.data) and "taps_per_branch" in built.pfb_last_error()
    assert not L.rtlws_pfb_open(None, 6, 1, None) and "null taps" in built.pfb_last_error()
    with pytest.raises(RuntimeError):
        built.PfbPlan(None, 6, taps)
    with pytest.raises(RuntimeError):
        built.PfbPlan(None, 6, taps[:63])
    L.rtlws_pfb_close(None)

    # the refusals of rtlws_pfb_run that need no plan are made before the plan is asked for anything
    A, B = 1 << 20, 2 << 20                                   # stand-ins for device pointers: never dereferenced
    CH, TM = built.PFB_CHANNEL_MAJOR, built.PFB_TIME_MAJOR

    def run(**kw):
        args = [kw.get(k, d) for k, d in (("plan", None), ("iq", A), ("n", 100), ("hop", 64), ("first", 0), ("layout", CH),
                                          ("out", B), ("stride", 100), ("st", None))]
        return L.rtlws_pfb_run(*args), built.pfb_last_error()

    for kw, word in (({"hop": 0}, "hop"), ({"hop": 48}, "hop"), ({"hop": 4}, "hop"), ({"hop": 2048}, "hop"), ({"hop": -64}, "hop"),
                     ({"n": -1}, "nframes"), ({"n": 1 << 62, "stride": 1 << 62}, "grid"), ({"first": -1}, "first_frame_index"),
                     ({"layout": 2}, "layout"), ({"layout": -1}, "layout"), ({"stride": 99}, "out_stride"),
                     ({"layout": TM, "stride": 15}, "out_stride"), ({"iq": None}, "null pointer"), ({"out": None}, "null pointer"),
                     ({"iq": A + 8}, "16-byte"), ({"out": B + 4}, "8-byte"), ({}, "null plan"),
                     ({"layout": TM, "stride": 16}, "null plan"), ({"n": 0, "stride": 0, "iq": None, "out": None}, "null plan")):
        rc, why = run(**kw)
        assert rc == -1 and word in why, (kw, why)


# ---- the yardstick's own properties ---------------------------------------------------------------------------

def test_reference_chunks_equal_the_whole():
    k, T = 5, 4
    M, D = 1 << k, 1 << (k - 1)
    taps = pfb_ref.random_taps(k, T, seed=1)
    n = 41
    iq = pfb_ref.random_iq(pfb_ref.samples_needed(M, T, D, n), seed=2)
    for first in (0, 7, (1 << 40) + 12345):
        whole = pfb_ref.pfb_ref(iq, k, taps, D, first)
        assert whole.shape == (n, M)
        cuts = (0, 1, 18, 41)                                  # an odd cut: 17 frames into the capture
        parts = [pfb_ref.pfb_ref(iq[a * D:(b - 1) * D + T * M], k, taps, D, first + a) for a, b in zip(cuts, cuts[1:])]
        assert np.array_equal(np.concatenate(parts, axis=0), whole)
        without = pfb_ref.pfb_ref(iq[D:], k, taps, D, first)   # the index matters: the odd channels change sign
        assert not np.array_equal(without, whole[1:])
        assert np.array_equal(without[:, 0::2], whole[1:, 0::2]) and np.array_equal(without[:, 1::2], -whole[1:, 1::2])
    # critically sampled: the factor is 1
    assert np.array_equal(pfb_ref.pfb_ref(iq, k, taps, M, 0), pfb_ref.pfb_ref(iq, k, taps, M, 1))


@pytest.mark.parametrize("k,T,c0", [(4, 1, 3), (6, 8, 5), (6, 8, 40), (8, 3, 129)])
def test_reference_tone_on_a_channel_centre_is_constant(built, k, T, c0):
    """x[n] = A e^(2 pi i c0 n / M), unquantised: Y[m][c0] = A sum(h) in every frame, at both hops."""
    M = 1 << k
    taps = built.pfb_design(k, T) if T > 1 else np.ones(M, np.int16)
    A = 77.25
    n = 12
    for D in (M, M // 2):
        x = A * np.exp(2j * np.pi * ((c0 * np.arange(pfb_ref.samples_needed(M, T, D, n))) % M) / M)
        y = pfb_ref.channelize(x, k, taps, D)
        want = A * taps.astype(np.float64).sum()
        assert y.shape == (n, M)
        assert np.abs(y[:, c0] - want).max() <= 1e-9 * abs(want)
        others = np.delete(y, c0, axis=1)
        if T == 1:
            assert np.abs(others).max() <= 1e-9 * abs(want)      # the flat window has its zeros there


def test_reference_with_one_flat_tap_is_the_ideal_bank():
    """T = 1, h = 1, D = M: the ideal mixer and block sum of tests/ddc_ref.py at R = M with words c P / M."""
    k = 5
    M = 1 << k
    P = ddc_ref.P
    n = 50
    iq = pfb_ref.random_iq(n * M, seed=3)
    words = [((c * (P // M) + P // 2) % P) - P // 2 for c in range(M)]
    ideal = ddc_ref.ddc_ideal(iq, M, words, first_dec_index=12345)
    y = pfb_ref.pfb_ref(iq, k, np.ones(M, np.int16), M, 12345)
    want = (ideal[..., 0] + 1j * ideal[..., 1]).T
    assert np.abs(y - want).max() <= 1e-9 * np.abs(want).max()


def test_reference_selectivity(built):
    """The largest mean power two or more channels away from both neighbours of the tone, relative to channel c0:
    the designed prototype (-52.9 dB) against the block sum as a prototype (-13.9 dB: the sinc at 2.5 channels)."""
    k, T, c0, iq, boxcar = pfb_ref.selectivity_case()
    designed = pfb_ref.leakage_db(pfb_ref.pfb_ref(iq, k, built.pfb_design(k, T)), c0)
    box = pfb_ref.leakage_db(pfb_ref.pfb_ref(iq, k, boxcar), c0)
    print("leakage two or more channels away: designed prototype %.1f dB, boxcar %.1f dB" % (designed, box))
    assert designed <= -40.0
    assert box >= -15.0

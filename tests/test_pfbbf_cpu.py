"""CPU suite of include/rtlws_pfbbf.h (librtlws_pfbbf.so): the ABI, the kernels' resources from the code-object
metadata, sizes, geometry and refusals -- and the numpy restatement's own properties (tests/pfbbf_ref.py), which hold
the yardstick rather than the code under test.  No GPU is used."""
import ctypes as C
import re
import subprocess

import numpy as np
import pytest

import pfb_ref
import pfbbf_ref
import pfbspec_ref
import pfbxc_ref
from test_abi_cpu import _declared_functions, _exported


def test_pfbbf_library_exports_its_header_and_nothing_else(built):
    built.pfbbf_lib()
    declared = _declared_functions("rtlws_pfbbf.h")
    assert sorted(declared) == sorted(["rtlws_pfbbf_supported", "rtlws_pfbbf_samples_needed", "rtlws_pfbbf_grid", "rtlws_pfbbf_open",
                                       "rtlws_pfbbf_run", "rtlws_pfbbf_power", "rtlws_pfbbf_close", "rtlws_pfbbf_last_error"])
    assert _exported(built.PFBBF_LIB) == set(declared)
    assert set(built.PFBBF_SYMBOLS) == set(declared)
    dyn = subprocess.run(["readelf", "-d", built.PFBBF_LIB], capture_output=True, text=True, check=True).stdout
    assert "librtlws_hip.so" in dyn and "$ORIGIN" in dyn
    # the libraries it stands beside export what they exported
    for lib, header in (("PFB_LIB", "rtlws_pfb.h"), ("PFBSPEC_LIB", "rtlws_pfbspec.h"), ("PFBXC_LIB", "rtlws_pfbxc.h")):
        assert _exported(getattr(built, lib)) == set(_declared_functions(header)), lib


def test_pfbbf_kernels_keep_their_budgets(built):
    """Every kernel of the library: no scratch, no spilled register, exactly one tile of LDS (34 816 bytes) whatever
    B is; at most 256 VGPRs (two workgroups of 256 per compute unit) in every instantiation, B = 4 among them, and at
    most 168 (three) at B = 1.  The kernel names are exactly the instantiations the launch tables reach: the voltage
    kernel per log2 M = 4 .. 10 and B = 1 .. 4, the power kernel per (log2 M, B) for K >= F and for K < F.
    rtlws_pfbbf_grid reports the code object's LDS and threads."""
    from rtlws import codeobj
    built.pfbbf_lib()
    ks = codeobj.kernels(built.PFBBF_LIB)
    names = set()
    worst = {}
    for k in ks:
        d = k.get("demangled", k["name"])
        m = re.search(r"rtlws::pfbbf::pfbbf_kernel<(\d+), (\d+)>", d)
        if m:
            key = ("voltage", int(m.group(1)), int(m.group(2)))
        else:
            m = re.search(r"rtlws::pfbbf::pfbbf_power_kernel<(\d+), (\d+), (true|false)>", d)
            assert m, d
            key = ("power " + m.group(3), int(m.group(1)), int(m.group(2)))
        assert key not in names, d
        names.add(key)
        assert k["vgpr_spill_count"] == 0 and k["private_segment_fixed_size"] == 0, d
        assert not k.get("sgpr_spill_count", 0), d
        regs = k["vgpr_count"] + (k.get("agpr_count") or 0)
        nbeams = key[2]
        assert regs <= (168 if nbeams == 1 else 256), (d, regs)
        assert k["group_segment_fixed_size"] == 34816 == pfbbf_ref.LDS_BYTES, d
        assert k["max_flat_workgroup_size"] == 256, d
        worst[key[0], nbeams] = max(worst.get((key[0], nbeams), 0), regs)
    print("largest VGPR allocation by (kernel, B): %s" % sorted(worst.items()))
    assert names == {(kind, k, b) for kind in ("voltage", "power true", "power false") for k in range(4, 11) for b in range(1, 5)}
    assert len(ks) == 84
    for k in range(4, 11):
        for hop in (1 << k, 1 << (k - 1)):
            for k_avg in (0, 1, 3, 65536):
                rc, blocks, threads, lds, per = built.pfbbf_grid(k, 3, hop, k_avg, 1)
                assert (rc, blocks, threads, lds) == (0, 1, 256, 34816) == (0, 1, 256, built.pfb_grid(k, 3, hop, 1)[3])


def test_pfbbf_sizes_and_geometry_need_no_gpu(built):
    ok = built.pfbbf_supported
    for k in range(4, 11):
        for T in (1, 8, 32):
            for hop in (1 << k, 1 << (k - 1)):
                for a in (1, 3, 8):
                    for b in (1, 2, 4):
                        assert ok(k, T, hop, a, b) == 1 and built.pfbbf_last_error() == "", (k, T, hop, a, b)
    for k, T, hop, a, b, word in ((3, 1, 8, 1, 1, "log2_channels"), (11, 1, 2048, 1, 1, "log2_channels"),
                                  (4, 0, 16, 1, 1, "taps_per_branch"), (4, 33, 16, 1, 1, "taps_per_branch"),
                                  (4, 1, 4, 1, 1, "hop"), (6, 8, 48, 1, 1, "hop"), (6, 8, 0, 1, 1, "hop"),
                                  (6, 8, 64, 0, 1, "ninputs"), (6, 8, 64, 9, 1, "ninputs"), (6, 8, 64, -1, 1, "ninputs"),
                                  (6, 8, 64, 1, 0, "nbeams"), (6, 8, 64, 1, 5, "nbeams"), (6, 8, 64, 8, -4, "nbeams")):
        assert ok(k, T, hop, a, b) == 0 and word in built.pfbbf_last_error(), (k, T, hop, a, b)

    need = built.pfbbf_samples_needed
    for k, T in ((4, 1), (6, 8), (10, 32)):
        M = 1 << k
        t = 4096 // M
        for hop in (M, M // 2):
            for n in (1, 2, t - 1, t, t + 1, 2 * t + 3):
                want = (n - 1) * hop + T * M
                assert need(k, T, hop, 0, n) == want == pfbbf_ref.samples_needed(M, T, hop, 0, n) == built.pfb_samples_needed(k, T, hop, n)
            for k_avg in (1, 2, t - 1, t, t + 1, 2 * t + 3):
                for n in (1, 2, t - 1, t, t + 1):
                    want = (n * k_avg - 1) * hop + T * M
                    assert need(k, T, hop, k_avg, n) == want == pfbbf_ref.samples_needed(M, T, hop, k_avg, n), (k, hop, k_avg, n)
                    assert want == built.pfbspec_samples_needed(k, T, hop, k_avg, n)
                assert need(k, T, hop, k_avg, 0) == 0
            assert need(k, T, hop, 0, 0) == 0
    assert need(6, 8, 64, 1, 1 << 36) == ((1 << 36) - 1) * 64 + 512
    assert need(6, 8, 64, 1, 1 << 40) == -1 and "grid" in built.pfbbf_last_error()
    assert need(6, 8, 64, 0, 1 << 40) == -1 and "grid" in built.pfbbf_last_error()
    assert need(6, 8, 64, 65536, 1 << 31) == -1 and "grid" in built.pfbbf_last_error()
    assert need(6, 8, 64, 1, -1) == -1 and "nspectra" in built.pfbbf_last_error()
    assert need(6, 8, 64, 0, -1) == -1 and "nframes" in built.pfbbf_last_error()
    assert need(6, 8, 16, 1, 1) == -1 and "hop" in built.pfbbf_last_error()
    assert need(6, 8, 64, -1, 1) == -1 and "k_avg" in built.pfbbf_last_error()
    assert need(6, 8, 64, 65537, 1) == -1 and "k_avg" in built.pfbbf_last_error()
    assert need(3, 8, 8, 1, 1) == -1 and need(6, 33, 64, 1, 1) == -1

    # the grid: the channelizer's geometry (k_avg = 0) or the spectrometer's, one tile
    for k in (4, 6, 10):
        M = 1 << k
        t = 4096 // M
        for n in (0, 1, t - 1, t, t + 1, 2 * t + 3, 1 << 27):
            got = built.pfbbf_grid(k, 8, M // 2, 0, n)
            assert got == (0,) + pfbbf_ref.grid(M, 0, n) == built.pfb_grid(k, 8, M // 2, n), (k, n)
        for k_avg in (1, 2, 3, t - 1, t, t + 1, 2 * t + 3, 65536):
            per = 1 if k_avg >= t else t // k_avg
            for n in (0, 1, per - 1, per, per + 1, 2 * per + 3, 1 << 27):
                got = built.pfbbf_grid(k, 8, M // 2, k_avg, n)
                assert got == (0, -(-n // per), 256, 34816, per) == (0,) + pfbbf_ref.grid(M, k_avg, n), (k, k_avg, n)
                assert got == built.pfbspec_grid(k, 8, M // 2, k_avg, n)
        assert built.pfbbf_grid(k, 8, M, 1, 1 << 62)[0] == -1 and "grid" in built.pfbbf_last_error()
        assert built.pfbbf_grid(k, 8, M, 0, 1 << 62)[0] == -1 and "grid" in built.pfbbf_last_error()
        assert built.pfbbf_grid(k, 8, M, t, 1 << 31)[0] == -1 and "grid" in built.pfbbf_last_error()
        assert built.pfbbf_grid(k, 8, M, 1, -1)[0] == -1 and "nspectra" in built.pfbbf_last_error()
        assert built.pfbbf_grid(k, 8, M, 0, -1)[0] == -1 and "nframes" in built.pfbbf_last_error()
    assert built.pfbbf_grid(3, 1, 8, 1, 1)[0] == -1 and built.pfbbf_grid(6, 0, 64, 1, 1)[0] == -1
    assert built.pfbbf_grid(6, 8, 63, 1, 1)[0] == -1 and built.pfbbf_grid(6, 8, 64, -1, 1)[0] == -1
    assert built.pfbbf_lib().rtlws_pfbbf_grid(6, 8, 64, 3, 1, None, None, None, None) == 0


def test_pfbbf_refusals_in_their_order_need_no_gpu(built):
    L = built.pfbbf_lib()
    # no engine, no plan: a text, never a crash
    taps = np.ones(64, np.int16)
    assert not L.rtlws_pfbbf_open(None, 6, 1, taps.ctypes.data, 2, 1) and "no CPU path" in built.pfbbf_last_error()
    assert not L.rtlws_pfbbf_open(None, 3, 1, taps.ctypes.data, 2, 1) and "log2_channels" in built.pfbbf_last_error()
    assert not L.rtlws_pfbbf_open(None, 6, 33, taps.ctypes.data, 2, 1) and "taps_per_branch" in built.pfbbf_last_error()
    assert not L.rtlws_pfbbf_open(None, 6, 1, taps.ctypes.data, 0, 1) and "ninputs" in built.pfbbf_last_error()
    assert not L.rtlws_pfbbf_open(None, 6, 1, taps.ctypes.data, 9, 1) and "ninputs" in built.pfbbf_last_error()
    assert not L.rtlws_pfbbf_open(None, 6, 1, taps.ctypes.data, 2, 0) and "nbeams" in built.pfbbf_last_error()
    assert not L.rtlws_pfbbf_open(None, 6, 1, taps.ctypes.data, 2, 5) and "nbeams" in built.pfbbf_last_error()
    assert not L.rtlws_pfbbf_open(None, 6, 1, None, 2, 1) and "null taps" in built.pfbbf_last_error()
    with pytest.raises(RuntimeError):
        built.PfbBfPlan(None, 6, taps, 2, 1)
    with pytest.raises(RuntimeError):
        built.PfbBfPlan(None, 6, taps[:63], 2, 1)
    L.rtlws_pfbbf_close(None)

    A, W, X = 1 << 20, 2 << 20, 3 << 20                       # stand-ins for device pointers: never dereferenced
    arr = (C.c_void_p * 2)(A, A + 4096)

    def check(fn, name, base, cases, chain):
        def run(**kw):
            assert set(kw) <= {k for k, _ in base}
            return fn(*[kw.get(k, d) for k, d in base]), built.pfbbf_last_error()

        for kw, word in cases:
            rc, why = run(**kw)
            assert rc == -1 and word in why and why.startswith(name + ": ") and len(why) > len(name) + 2, (kw, why)
        # the order: a call that breaks rule i and every later rule is refused for rule i
        for i, (_, word) in enumerate(chain):
            kw = {}
            for later, _ in reversed(chain[i:]):
                kw.update(later)
            rc, why = run(**kw)
            assert rc == -1 and word in why, (i, kw, why)

    # voltage mode: 100 frames time-major at stride 64, beams 6400 apart
    base = (("plan", None), ("iq", arr), ("a", 2), ("w", W), ("b", 2), ("n", 100), ("hop", 64), ("first", 0), ("layout", 1),
            ("out", X), ("ostride", 64), ("bstride", 6400), ("st", None))
    cases = (({"hop": 0}, "hop"), ({"hop": 48}, "hop"), ({"hop": 4}, "hop"), ({"hop": 2048}, "hop"), ({"hop": -64}, "hop"),
             ({"a": 0}, "ninputs"), ({"a": 9}, "ninputs"), ({"b": 0}, "nbeams"), ({"b": 5}, "nbeams"),
             ({"n": -1}, "nframes"), ({"n": 1 << 62}, "grid"),
             ({"first": -1}, "first_frame_index"), ({"layout": 2}, "layout"), ({"layout": -1}, "layout"),
             ({"ostride": 15}, "out_stride"), ({"layout": 0, "ostride": 99}, "out_stride"),
             ({"bstride": 99 * 64 + 15}, "beam_stride"), ({"layout": 0, "ostride": 100, "bstride": 15 * 100 + 99}, "beam_stride"),
             ({"bstride": -1}, "beam_stride"), ({"ostride": 1 << 40, "bstride": 1 << 41}, "beam_stride"),
             ({"iq": None}, "null pointer"), ({"w": None}, "null pointer"), ({"out": None}, "null pointer"),
             ({"w": W + 8}, "d_weights must be 16-byte"), ({"out": X + 4}, "d_out_cf32 must be 8-byte"),
             ({}, "null plan"), ({"ostride": 16, "bstride": 99 * 16 + 16}, "null plan"), ({"out": X + 8}, "null plan"),
             ({"layout": 0, "ostride": 100, "bstride": 15 * 100 + 100}, "null plan"),
             ({"n": 0, "iq": None, "w": None, "out": None, "bstride": 0}, "null plan"))
    chain = (({"hop": 48}, "hop"), ({"a": 9}, "ninputs"), ({"b": 0}, "nbeams"), ({"n": -1}, "nframes"), ({"first": -1}, "first_frame_index"),
             ({"layout": 2}, "layout"), ({"ostride": 8}, "out_stride"), ({"bstride": 7}, "beam_stride"), ({"w": None}, "null pointer"),
             ({"out": X + 4}, "d_out_cf32"), ({}, "null plan"))
    # ({"w": None} stands for the alignment rule's turn too: a null pointer is aligned)
    check(L.rtlws_pfbbf_run, "rtlws_pfbbf_run", base, cases, chain)
    check(L.rtlws_pfbbf_run, "rtlws_pfbbf_run", base, (),
          (({"out": None}, "null pointer"), ({"w": W + 4}, "d_weights"), ({"out": X + 4}, "d_out_cf32"), ({}, "null plan")))

    # power mode: 100 spectra of K = 3 at stride 64
    base = (("plan", None), ("iq", arr), ("a", 2), ("w", W), ("b", 2), ("n", 100), ("hop", 64), ("k", 3), ("shifted", 0),
            ("out", X), ("rstride", 64), ("st", None))
    cases = (({"hop": 0}, "hop"), ({"hop": 48}, "hop"), ({"hop": 4}, "hop"), ({"hop": 2048}, "hop"),
             ({"k": 0}, "k_avg"), ({"k": -1}, "k_avg"), ({"k": 65537}, "k_avg"),
             ({"shifted": 2}, "shifted"), ({"shifted": -1}, "shifted"),
             ({"a": 0}, "ninputs"), ({"a": 9}, "ninputs"), ({"b": 0}, "nbeams"), ({"b": 5}, "nbeams"),
             ({"n": -1}, "nspectra"), ({"n": 1 << 62}, "grid"), ({"n": 1 << 31, "k": 300}, "grid"),
             ({"rstride": 15}, "row_stride must be >= M"), ({"rstride": 12}, "row_stride must be >= M"),
             ({"rstride": 66}, "row_stride must be a multiple of 4"),
             ({"iq": None}, "null pointer"), ({"w": None}, "null pointer"), ({"out": None}, "null pointer"),
             ({"w": W + 8}, "d_weights must be 16-byte"), ({"out": X + 8}, "d_out must be 16-byte"), ({"out": X + 4}, "d_out must be 16-byte"),
             ({}, "null plan"), ({"rstride": 16}, "null plan"), ({"n": 0, "iq": None, "w": None, "out": None}, "null plan"))
    chain = (({"hop": 48}, "hop"), ({"k": 0}, "k_avg"), ({"shifted": 2}, "shifted"), ({"a": 0}, "ninputs"), ({"b": 5}, "nbeams"),
             ({"n": -1}, "nspectra"), ({"rstride": 8}, "row_stride must be >= M"), ({"iq": None}, "null pointer"),
             ({"out": X + 8}, "d_out must be 16-byte"), ({}, "null plan"))
    check(L.rtlws_pfbbf_power, "rtlws_pfbbf_power", base, cases, chain)
    check(L.rtlws_pfbbf_power, "rtlws_pfbbf_power", base, (),
          (({"rstride": 18}, "row_stride must be a multiple"), ({"w": W + 4}, "d_weights"), ({"out": X + 8}, "d_out"), ({}, "null plan")))


# ---- the yardstick's own properties ---------------------------------------------------------------------------

def _random_case(k, T, D, nframes, A, seed):
    M = 1 << k
    taps = pfb_ref.random_taps(k, T, seed=seed)
    iqs = pfbbf_ref.random_captures(A, pfb_ref.samples_needed(M, T, D, nframes), seed=seed + 1)
    return taps, iqs


def test_reference_one_hot_weights_give_the_channelizer_and_the_spectrometer():
    k, T, K, n, A = 5, 4, 3, 4, 3
    M = 1 << k
    for D in (M, M // 2):
        taps, iqs = _random_case(k, T, D, n * K, A, seed=11)
        W = pfbbf_ref.one_hot(2, A, M, (2, 0))
        for first in (0, 7):
            z = pfbbf_ref.pfbbf_ref(iqs, W, k, taps, D, first)
            assert z.shape == (2, n * K, M) and z.dtype == np.complex128
            assert np.array_equal(z[0], pfb_ref.pfb_ref(iqs[2], k, taps, D, first))
            assert np.array_equal(z[1], pfb_ref.pfb_ref(iqs[0], k, taps, D, first))
        for shifted in (False, True):
            s = pfbbf_ref.pfbbf_power_ref(iqs, W, k, taps, K, D, shifted)
            assert s.shape == (n, 2, M)
            assert np.array_equal(s[:, 0], pfbspec_ref.pfbspec_ref(iqs[2], k, taps, K, D, shifted))
            assert np.array_equal(s[:, 1], pfbspec_ref.pfbspec_ref(iqs[0], k, taps, K, D, shifted))
        # a sub-capture gives the later rows, and the f32 arithmetic passes one capture through unchanged
        part = pfbbf_ref.pfbbf_power_ref([x[2 * K * D:] for x in iqs], W, k, taps, K, D)
        assert np.array_equal(part, pfbbf_ref.pfbbf_power_ref(iqs, W, k, taps, K, D)[2:])
        ys = [pfbxc_ref.standin_frames(x, k, taps, D, n * K) for x in iqs]
        z32 = pfbbf_ref.beams_f32(ys, W)
        assert z32.dtype == np.complex64 and np.array_equal(z32[0], ys[2]) and np.array_equal(z32[1], ys[0])
        assert np.array_equal(pfbbf_ref.power_f32(z32, k, K)[:, 0].view(np.uint32),
                              pfbxc_ref.ordered_sums(pfbxc_ref.products_f32(ys[2], ys[2])[0], k, K).view(np.uint32))
        # the flip is the sign rule and its own inverse
        fl = pfbbf_ref.flip(z32, M, D, 3)
        assert np.array_equal(fl, z32 * pfbbf_ref.signs(M, D, 3, n * K).astype(np.float32)[None])
        assert np.array_equal(pfbbf_ref.flip(fl, M, D, 3).view(np.uint32), z32.view(np.uint32))


def test_reference_is_linear_in_the_weights():
    k, T, n, A, B = 6, 3, 5, 4, 2
    M = 1 << k
    for D in (M, M // 2):
        taps, iqs = _random_case(k, T, D, n, A, seed=21)
        W1, W2 = pfbbf_ref.random_weights(B, A, M, seed=1), pfbbf_ref.random_weights(B, A, M, seed=2)
        assert np.abs(W1).max() <= 2.0 and np.abs(W1).max() > 1.5 and W1.dtype == np.complex64
        z1, z2 = pfbbf_ref.pfbbf_ref(iqs, W1, k, taps, D, 1), pfbbf_ref.pfbbf_ref(iqs, W2, k, taps, D, 1)
        z = pfbbf_ref.pfbbf_ref(iqs, 2.0 * W1.astype(np.complex128) - 1j * W2, k, taps, D, 1)
        assert np.abs(z - (2.0 * z1 - 1j * z2)).max() <= 1e-12 * np.abs(z).max()
        # beam b does not know the other beams, and a beam is the sum of its one-capture beams
        assert np.array_equal(pfbbf_ref.pfbbf_ref(iqs, W1[1:], k, taps, D, 1)[0], z1[1])
        parts = sum(pfbbf_ref.pfbbf_ref([iqs[a]], W1[:, a:a + 1], k, taps, D, 1) for a in range(A))
        assert np.abs(parts - z1).max() <= 1e-12 * np.abs(z1).max()
        # the same capture twice with weights (+1, -1) is nothing at all
        w = pfbbf_ref.one_hot(1, 2, M, (0,))
        w[0, 1] = -1.0
        assert not pfbbf_ref.pfbbf_ref([iqs[0], iqs[0]], w, k, taps, D).any()


@pytest.mark.parametrize("k,T", ((4, 7), (6, 8), (10, 4)))
def test_bounds_hold_for_the_f32_stand_in(k, T):
    """The device emulated by torch's f32 FFT of the exact branch sums, the beams, products and sums in numpy f32 in
    the definition's order: random bytes with random taps and random weights; both hops; (A, B) = (3, 2) and (8, 4)."""
    M = 1 << k
    F = 4096 // M
    n = 2
    worst_v = worst_p = 0.0
    for D in (M, M // 2):
        for A, B in ((3, 2), (8, 4)):
            for K in (1, 3, F + 1):
                taps, iqs = _random_case(k, T, D, n * K, A, seed=k + T + K + A)
                W = pfbbf_ref.random_weights(B, A, M, seed=A + K)
                ys = pfbbf_ref.frames_of(iqs, k, taps, D, n * K)
                got = pfbbf_ref.beams_f32([pfbxc_ref.standin_frames(x, k, taps, D, n * K) for x in iqs], W)
                rv = pfbbf_ref.voltage_ratio(got, pfbbf_ref.beams(ys, W), ys, W, k)
                rp = pfbbf_ref.power_ratio(pfbbf_ref.power_f32(got, k, K), pfbbf_ref.k_sums(pfbbf_ref.beams(ys, W), K), ys, W, k, K)
                worst_v, worst_p = max(worst_v, rv), max(worst_p, rp)
                assert rv <= 1.0 and rp <= 1.0, (D, A, B, K, rv, rp)
                # what the bound is for: one weight conjugated, or one capture left out, falls far outside
                Wc = W.copy()
                Wc[0, A - 1] = np.conj(Wc[0, A - 1])
                assert pfbbf_ref.voltage_ratio(pfbbf_ref.beams_f32([y.astype(np.complex64) for y in ys], Wc), pfbbf_ref.beams(ys, W), ys, W, k) > 100.0
    print("M = %d, T = %d: stand-in's worst ratios: voltage %.4f, power %.4f" % (M, T, worst_v, worst_p))
    assert pfbbf_ref.bound(6, 4) == (8 * 7 + 4 + 3) * 2.0 ** -24
    assert pfbbf_ref.power_bound(6, 4, 64) == (16 * 7 + 8 + 64 + 10) * 2.0 ** -24


def test_reference_delay_case():
    """Four captures that lag by 0, 1, 3, 6 samples: the steered beam has 15.4 times the power of one of its elements
    (A^2 = 16 less the captures' own noise), and the (1, -e^(2 pi i c / M)) beam over captures 0 and 1 is left with
    0.075 of capture 0's power.  The thresholds are half and double these figures of the restatement."""
    k, taps, D, K, iqs, w_steer, w_null = pfbbf_ref.delay_case()
    steer = pfbbf_ref.pfbbf_power_ref(iqs, w_steer, k, taps, K, D, nspectra=1)
    null = pfbbf_ref.pfbbf_power_ref(iqs[:2], w_null, k, taps, K, D, nspectra=1)
    assert steer.shape == (1, 2, 64) and null.shape == (1, 2, 64)
    gain, depth = pfbbf_ref.delay_figures(steer[0], null[0])
    print("steered gain over one element %.4f, null depth %.6f" % (gain, depth))
    assert abs(gain - pfbbf_ref.STEER_GAIN) <= 1e-3 * pfbbf_ref.STEER_GAIN and abs(depth - pfbbf_ref.NULL_DEPTH) <= 1e-3 * pfbbf_ref.NULL_DEPTH
    assert pfbbf_ref.STEER_GAIN_MIN == pfbbf_ref.STEER_GAIN / 2 and pfbbf_ref.NULL_DEPTH_MAX == 2 * pfbbf_ref.NULL_DEPTH
    assert gain >= pfbbf_ref.STEER_GAIN_MIN > 4.0 and depth <= pfbbf_ref.NULL_DEPTH_MAX < 0.25
    # the sign of the convention: steering the other way loses the gain, and adding instead of subtracting fills the null
    wrong = w_steer.copy()
    wrong[0] = np.conj(wrong[0])
    g2, _ = pfbbf_ref.delay_figures(pfbbf_ref.pfbbf_power_ref(iqs, wrong, k, taps, K, D, nspectra=1)[0], null[0])
    filled = w_null.copy()
    filled[0, 1] = -filled[0, 1]
    _, d2 = pfbbf_ref.delay_figures(steer[0], pfbbf_ref.pfbbf_power_ref(iqs[:2], filled, k, taps, K, D, nspectra=1)[0])
    assert g2 < pfbbf_ref.STEER_GAIN_MIN and d2 > 10 * pfbbf_ref.NULL_DEPTH_MAX

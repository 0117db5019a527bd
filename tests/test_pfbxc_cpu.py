"""CPU suite of include/rtlws_pfbxc.h (librtlws_pfbxc.so): the ABI, the kernels' resources from the code-object
metadata, sizes, the pair index and refusals -- and the numpy restatement's own properties (tests/pfbxc_ref.py), which
hold the yardstick rather than the code under test.  No GPU is used."""
import re
import subprocess

import numpy as np
import pytest

import pfb_ref
import pfbspec_ref
import pfbxc_ref
from test_abi_cpu import _declared_functions, _exported


def test_pfbxc_library_exports_its_header_and_nothing_else(built):
    built.pfbxc_lib()
    declared = _declared_functions("rtlws_pfbxc.h")
    assert len(declared) == 8
    assert _exported(built.PFBXC_LIB) == set(declared)
    assert set(built.PFBXC_SYMBOLS) == set(declared)
    dyn = subprocess.run(["readelf", "-d", built.PFBXC_LIB], capture_output=True, text=True, check=True).stdout
    assert "librtlws_hip.so" in dyn and "$ORIGIN" in dyn
    # the libraries it stands beside export what they exported
    for lib, header in (("PFB_LIB", "rtlws_pfb.h"), ("PFBSPEC_LIB", "rtlws_pfbspec.h")):
        assert _exported(getattr(built, lib)) == set(_declared_functions(header)), lib


def test_pfbxc_kernels_do_not_spill(built):
    """Every kernel of the library: no scratch, no spilled register, at most 160 KiB of LDS; within 256 VGPRs at
    A = 2 (two workgroups of 256 per compute unit); the kernel names are exactly the instantiations the launch table
    reaches (one per log2 M = 4 .. 10 and A = 2 .. 4); rtlws_pfbxc_grid reports the code object's LDS and threads."""
    from rtlws import codeobj
    built.pfbxc_lib()
    ks = codeobj.kernels(built.PFBXC_LIB)
    names = {}
    for k in ks:
        d = k.get("demangled", k["name"])
        m = re.search(r"rtlws::pfbxc::pfbxc_kernel<(\d+), (\d+)>", d)
        assert m, d
        names[int(m.group(1)), int(m.group(2))] = k
        assert k["vgpr_spill_count"] == 0 and k["private_segment_fixed_size"] == 0, d
        assert not k.get("sgpr_spill_count", 0), d
        regs = k["vgpr_count"] + (k.get("agpr_count") or 0)
        assert regs <= (256 if int(m.group(2)) == 2 else 512), (d, regs)
        assert k["group_segment_fixed_size"] <= 160 * 1024, d
    assert set(names) == {(k, a) for k in range(4, 11) for a in (2, 3, 4)} and len(ks) == 21
    for (k, a), meta in names.items():
        for hop in (1 << k, 1 << (k - 1)):
            for k_avg in (1, 3, 65536):
                rc, blocks, threads, lds, per = built.pfbxc_grid(k, 3, hop, k_avg, a, 1)
                assert rc == 0 and blocks == 1
                assert threads == meta["max_flat_workgroup_size"] == 256
                assert lds == meta["group_segment_fixed_size"] == a * built.pfb_grid(k, 3, hop, 1)[3], (k, a, lds)


def test_pfbxc_sizes_pairs_and_refusals_need_no_gpu(built):
    ok = built.pfbxc_supported
    for k in range(4, 11):
        for T in (1, 8, 32):
            for hop in (1 << k, 1 << (k - 1)):
                for k_avg in (1, 7, 65536):
                    for a in (2, 3, 4):
                        assert ok(k, T, hop, k_avg, a) == 1 and built.pfbxc_last_error() == "", (k, T, hop, k_avg, a)
    for k, T, hop, k_avg, a, word in ((3, 1, 8, 1, 2, "log2_channels"), (11, 1, 2048, 1, 2, "log2_channels"),
                                      (4, 0, 16, 1, 2, "taps_per_branch"), (4, 33, 16, 1, 2, "taps_per_branch"),
                                      (4, 1, 4, 1, 2, "hop"), (6, 8, 48, 1, 2, "hop"), (6, 8, 0, 1, 2, "hop"),
                                      (6, 8, 64, 0, 2, "k_avg"), (6, 8, 64, 65537, 2, "k_avg"), (6, 8, 64, -1, 2, "k_avg"),
                                      (6, 8, 64, 1, 1, "ninputs"), (6, 8, 64, 1, 5, "ninputs"), (6, 8, 64, 1, 0, "ninputs"),
                                      (6, 8, 64, 1, -2, "ninputs")):
        assert ok(k, T, hop, k_avg, a) == 0 and word in built.pfbxc_last_error(), (k, T, hop, k_avg, a)

    # the pair index: the pairs a < b row-major, -1 for anything else
    for A in range(0, 7):
        for a in range(-1, 6):
            for b in range(-1, 6):
                assert built.pfbxc_pair_index(A, a, b) == pfbxc_ref.pair_index(A, a, b), (A, a, b)
    assert [built.pfbxc_pair_index(4, a, b) for a, b in pfbxc_ref.pairs(4)] == [0, 1, 2, 3, 4, 5]
    assert pfbxc_ref.pairs(3) == [(0, 1), (0, 2), (1, 2)]

    # per capture: the spectrometer's figure
    need = built.pfbxc_samples_needed
    for k, T in ((4, 1), (6, 8), (10, 32)):
        M = 1 << k
        t = 4096 // M
        for hop in (M, M // 2):
            for k_avg in (1, 2, t - 1, t, t + 1, 2 * t + 3):
                for n in (1, 2, t - 1, t, t + 1):
                    want = (n * k_avg - 1) * hop + T * M
                    assert need(k, T, hop, k_avg, n) == want == pfbxc_ref.samples_needed(M, T, hop, k_avg, n), (k, hop, k_avg, n)
                    assert want == built.pfbspec_samples_needed(k, T, hop, k_avg, n)
                assert need(k, T, hop, k_avg, 0) == 0
    assert need(6, 8, 64, 1, 1 << 36) == ((1 << 36) - 1) * 64 + 512
    assert need(6, 8, 64, 1, 1 << 40) == -1 and "grid" in built.pfbxc_last_error()
    assert need(6, 8, 64, 65536, 1 << 31) == -1 and "grid" in built.pfbxc_last_error()
    assert need(6, 8, 64, 1, -1) == -1 and "nspectra" in built.pfbxc_last_error()
    assert need(6, 8, 16, 1, 1) == -1 and "hop" in built.pfbxc_last_error()
    assert need(6, 8, 64, 0, 1) == -1 and "k_avg" in built.pfbxc_last_error()
    assert need(3, 8, 8, 1, 1) == -1 and need(6, 33, 64, 1, 1) == -1

    # the grid: the spectrometer's geometry, A tiles
    for k in (4, 6, 10):
        M = 1 << k
        t = built.pfb_grid(k, 8, M, 1)[4]
        assert t == 4096 // M
        for a in (2, 3, 4):
            for k_avg in (1, 2, 3, t - 1, t, t + 1, 2 * t + 3, 65536):
                per = 1 if k_avg >= t else t // k_avg
                for n in (0, 1, per - 1, per, per + 1, 2 * per + 3, 1 << 27):
                    got = built.pfbxc_grid(k, 8, M // 2, k_avg, a, n)
                    assert got == (0, -(-n // per), 256, a * 34816, per), (k, k_avg, a, n)
                    assert got[:3] + got[4:] == (lambda s: s[:3] + s[4:])(built.pfbspec_grid(k, 8, M // 2, k_avg, n))
        assert built.pfbxc_grid(k, 8, M, 1, 2, 1 << 62)[0] == -1 and "grid" in built.pfbxc_last_error()
        assert built.pfbxc_grid(k, 8, M, t, 2, 1 << 31)[0] == -1 and "grid" in built.pfbxc_last_error()
        assert built.pfbxc_grid(k, 8, M, 1, 2, -1)[0] == -1 and "nspectra" in built.pfbxc_last_error()
        assert built.pfbxc_grid(k, 8, M, 1, 5, 1)[0] == -1 and "ninputs" in built.pfbxc_last_error()
    assert built.pfbxc_grid(3, 1, 8, 1, 2, 1)[0] == -1 and built.pfbxc_grid(6, 0, 64, 1, 2, 1)[0] == -1
    assert built.pfbxc_grid(6, 8, 63, 1, 2, 1)[0] == -1 and built.pfbxc_grid(6, 8, 64, 0, 2, 1)[0] == -1
    L = built.pfbxc_lib()
    assert L.rtlws_pfbxc_grid(6, 8, 64, 3, 2, 1, None, None, None, None) == 0

    # no engine, no plan: a text, never a crash
    taps = np.ones(64, np.int16)
    assert not L.rtlws_pfbxc_open(None, 6, 1, taps.ctypes.data, 2) and "no CPU path" in built.pfbxc_last_error()
    assert not L.rtlws_pfbxc_open(None, 3, 1, taps.ctypes.data, 2) and "log2_channels" in built.pfbxc_last_error()
    assert not L.rtlws_pfbxc_open(None, 6, 33, taps.ctypes.data, 2) and "taps_per_branch" in built.pfbxc_last_error()
    assert not L.rtlws_pfbxc_open(None, 6, 1, taps.ctypes.data, 1) and "ninputs" in built.pfbxc_last_error()
    assert not L.rtlws_pfbxc_open(None, 6, 1, taps.ctypes.data, 5) and "ninputs" in built.pfbxc_last_error()
    assert not L.rtlws_pfbxc_open(None, 6, 1, None, 2) and "null taps" in built.pfbxc_last_error()
    with pytest.raises(RuntimeError):
        built.PfbXcPlan(None, 6, taps, 2)
    with pytest.raises(RuntimeError):
        built.PfbXcPlan(None, 6, taps[:63], 2)
    L.rtlws_pfbxc_close(None)

    # the refusals of rtlws_pfbxc_run that need no plan are made before the plan is asked for anything
    import ctypes as C
    A, B, X = 1 << 20, 2 << 20, 3 << 20                       # stand-ins for device pointers: never dereferenced
    arr = (C.c_void_p * 2)(A, A + 4096)
    base = (("plan", None), ("iq", arr), ("n", 100), ("hop", 64), ("k", 3), ("shifted", 0), ("auto", B), ("astride", 64),
            ("cross", X), ("cstride", 64), ("st", None))

    def run(**kw):
        assert set(kw) <= {k for k, _ in base}
        return L.rtlws_pfbxc_run(*[kw.get(k, d) for k, d in base]), built.pfbxc_last_error()

    for kw, word in (({"hop": 0}, "hop"), ({"hop": 48}, "hop"), ({"hop": 4}, "hop"), ({"hop": 2048}, "hop"), ({"hop": -64}, "hop"),
                     ({"k": 0}, "k_avg"), ({"k": -1}, "k_avg"), ({"k": 65537}, "k_avg"),
                     ({"shifted": 2}, "shifted"), ({"shifted": -1}, "shifted"),
                     ({"n": -1}, "nspectra"), ({"n": 1 << 62}, "grid"), ({"n": 1 << 31, "k": 300}, "grid"),
                     ({"astride": 15}, "auto_stride must be >= M"), ({"astride": 12}, "auto_stride must be >= M"),
                     ({"astride": 66}, "auto_stride must be a multiple of 4"),
                     ({"cstride": 15}, "cross_stride must be >= M"), ({"cstride": 14}, "cross_stride must be >= M"),
                     ({"cstride": 65}, "cross_stride must be a multiple of 2"),
                     ({"iq": None}, "null pointer"), ({"auto": None}, "null pointer"), ({"cross": None}, "null pointer"),
                     ({"auto": B + 8}, "d_auto must be 16-byte"), ({"auto": B + 4}, "d_auto must be 16-byte"),
                     ({"cross": X + 8}, "d_cross must be 16-byte"),
                     ({}, "null plan"), ({"astride": 16, "cstride": 16}, "null plan"), ({"cstride": 66}, "null plan"),
                     ({"n": 0, "iq": None, "auto": None, "cross": None}, "null plan")):
        rc, why = run(**kw)
        assert rc == -1 and word in why and why.startswith("rtlws_pfbxc_run: "), (kw, why)

    # the order: a call that breaks rule i and every later rule is refused for rule i
    chain = (({"hop": 48}, "hop"), ({"k": 0}, "k_avg"), ({"shifted": 2}, "shifted"), ({"n": -1}, "nspectra"),
             ({"astride": 8}, "auto_stride must be >= M"), ({"astride": 18}, "auto_stride must be a multiple"),
             ({"cstride": 8}, "cross_stride must be >= M"), ({"cstride": 17}, "cross_stride must be a multiple"),
             ({"iq": None}, "null pointer"), ({"auto": B + 4}, "d_auto"), ({"cross": X + 8}, "d_cross"), ({}, "null plan"))
    for i, (_, word) in enumerate(chain):
        kw = {}
        for later, _ in reversed(chain[i:]):
            kw.update(later)
        rc, why = run(**kw)
        assert rc == -1 and word in why, (i, kw, why)


# ---- the yardstick's own properties ---------------------------------------------------------------------------

def _random_case(k, T, D, K, n, A, seed):
    M = 1 << k
    taps = pfb_ref.random_taps(k, T, seed=seed)
    iqs = [pfb_ref.random_iq(pfbxc_ref.samples_needed(M, T, D, K, n), seed=seed + 1 + a) for a in range(A)]
    return taps, iqs


def test_reference_swapping_two_inputs_conjugates_the_row():
    k, T, K, n = 5, 4, 3, 4
    M = 1 << k
    for D in (M, M // 2):
        taps, iqs = _random_case(k, T, D, K, n, 3, seed=11)
        autos, cross = pfbxc_ref.pfbxc_ref(iqs, k, taps, K, D)
        assert autos.shape == (n, 3, M) and cross.shape == (n, 3, M) and cross.dtype == np.complex128
        sw_autos, sw_cross = pfbxc_ref.pfbxc_ref([iqs[1], iqs[0], iqs[2]], k, taps, K, D)
        assert np.array_equal(sw_cross[:, 0], np.conj(cross[:, 0]))          # (1,0) = conj (0,1)
        assert np.array_equal(sw_cross[:, 1], cross[:, 2]) and np.array_equal(sw_cross[:, 2], cross[:, 1])
        assert np.array_equal(sw_autos, autos[:, [1, 0, 2]])
        # the autos are the spectrometer's definition, and a sub-capture gives the later rows
        for a in range(3):
            assert np.array_equal(autos[:, a], pfbspec_ref.pfbspec_ref(iqs[a], k, taps, K, D))
        part_a, part_c = pfbxc_ref.pfbxc_ref([x[2 * K * D:] for x in iqs], k, taps, K, D)
        assert np.array_equal(part_a, autos[2:]) and np.array_equal(part_c, cross[2:])
        sh_a, sh_c = pfbxc_ref.pfbxc_ref(iqs, k, taps, K, D, shifted=True)
        assert np.array_equal(sh_a, np.fft.fftshift(autos, axes=2)) and np.array_equal(sh_c[:, :, M // 2], cross[:, :, 0])


def test_reference_the_same_capture_twice_gives_the_auto_and_no_imaginary_part():
    k, T, K, n = 6, 3, 5, 3
    M = 1 << k
    for D in (M, M // 2):
        taps, iqs = _random_case(k, T, D, K, n, 2, seed=21)
        autos, cross = pfbxc_ref.pfbxc_ref([iqs[0], iqs[0], iqs[1]], k, taps, K, D)
        assert np.array_equal(cross[:, 0].real, autos[:, 0]) and not cross[:, 0].imag.any()
        assert np.array_equal(autos[:, 0], autos[:, 1]) and cross[:, 1].imag.any()
        # and in the f32 arithmetic of the definition: re is the auto's bits, im is +0
        y = pfbxc_ref.standin_frames(iqs[0], k, taps, D, n * K)
        a32, c32 = pfbxc_ref.sums_f32([y, y], k, K)
        assert np.array_equal(c32[:, 0].real.view(np.uint32), a32[:, 0].view(np.uint32))
        assert not c32[:, 0].imag.view(np.uint32).any()


def test_reference_order_of_the_sums():
    """ordered_sums: the slices of DESIGN.md 4.15 on a case small enough to write down."""
    k = 10                                                       # F = L = 4: one slice per tile position
    t = np.float32(2.0) ** np.arange(0, -7, -1, dtype=np.float32).reshape(7, 1) * np.ones((1, 1 << k), np.float32)
    got = pfbxc_ref.ordered_sums(t, k, 7)
    assert got.shape == (1, 1024) and got[0, 0] == np.float32(t[:, 0].sum())
    big = np.array([1.0, 2.0 ** -24, 2.0 ** -24, 2.0 ** -24, 2.0 ** -24], np.float32).reshape(5, 1) * np.ones((1, 16), np.float32)
    assert pfbxc_ref.ordered_sums(big, 4, 5)[0, 0] == np.float32(1.0)        # one slice, frame order: the small ones are lost
    k = 7                                                        # F = 32, L = 16
    seq = np.zeros((40, 128), np.float32)
    seq[0], seq[16:20], seq[32] = 1.0, 2.0 ** -24, 2.0 ** -24
    # K = 40 >= F: slice 0 = frames 0 .. 15 and 32 .. 39 -> 1 (+ 2^-24 lost); slice 1 = frames 16 .. 31 -> 4 * 2^-24
    assert pfbxc_ref.ordered_sums(seq, 7, 40)[0, 0] == np.float32(1.0) + np.float32(2.0 ** -22)
    # K = 20 < F: slice 0 = frames 0 .. 15, slice 1 = 16 .. 19
    assert pfbxc_ref.ordered_sums(seq[:20], 7, 20)[0, 0] == np.float32(1.0) + np.float32(2.0 ** -22)
    neg = np.full((3, 16), -0.0, np.float32)
    assert not np.signbit(pfbxc_ref.ordered_sums(neg, 4, 3)).any() and not np.signbit(pfbxc_ref.ordered_sums(neg, 4, 1)).any()


@pytest.mark.parametrize("k,T", pfb_ref.SHAPES)
def test_bound_holds_for_the_f32_stand_in(k, T):
    """The device emulated by torch's f32 FFT of the exact branch sums, the products and sums in numpy f32 in the
    definition's order: random bytes with random taps, and 0/255 bytes with every tap 32767; both hops;
    K in {1, 3, F + 1, 2 F + 3}."""
    M = 1 << k
    F = 4096 // M
    n = 2
    worst = 0.0
    for D in (M, M // 2):
        for K in (1, 3, F + 1, 2 * F + 3):
            ns = pfbxc_ref.samples_needed(M, T, D, K, n)
            for iqs, taps in (([pfb_ref.random_iq(ns, seed=k + T + K + a) for a in range(2)], pfb_ref.random_taps(k, T, seed=100 * k + T)),
                              ([pfb_ref.full_scale_iq(ns, seed=k * T + K + a) for a in range(2)], np.full(T * M, 32767, np.int16))):
                ref_a, ref_c = pfbxc_ref.pfbxc_ref(iqs, k, taps, K, D, nspectra=n)
                got_a, got_c = pfbxc_ref.sums_f32([pfbxc_ref.standin_frames(x, k, taps, D, n * K) for x in iqs], k, K)
                assert got_a.dtype == np.float32 and got_c.dtype == np.complex64 and got_c.shape == (n, 1, M)
                ra, rc = pfbxc_ref.auto_ratio(got_a, ref_a, k, K), pfbxc_ref.cross_ratio(got_c, ref_a, ref_c, k, K)
                worst = max(worst, rc)
                assert ra <= 1.0 and rc <= 1.0, (D, K, ra, rc)
                # what the bound is for: a conjugate the wrong way round, or a frame missing, falls far outside
                assert pfbxc_ref.cross_ratio(np.conj(got_c), ref_a, ref_c, k, K) > 100.0
                if K > 1:
                    short = got_c - (pfbxc_ref.standin_frames(iqs[0], k, taps, D, 1) * np.conj(pfbxc_ref.standin_frames(iqs[1], k, taps, D, 1)))
                    assert pfbxc_ref.cross_ratio(short[:1], ref_a[:1], ref_c[:1], k, K) > 10.0
    print("M = %d, T = %d: stand-in's worst cross ratio to the bound %.4f" % (M, T, worst))
    assert pfbxc_ref.bound(6, 64) == (16 * 7 + 2 * 64 + 6) * 2.0 ** -24


def test_reference_delay_case():
    """x_b lags x_a by one sample: the phase of V_01[c] is +2 pi c_signed / 64 (0.0038 rad off at most at hop M and
    0.0051 at hop M / 2 on the restatement) and the coherence at least 0.9995."""
    for hop_div in (1, 2):
        k, taps, D, K, iqs = pfbxc_ref.delay_case(hop_div)
        autos, cross = pfbxc_ref.pfbxc_ref(iqs, k, taps, K, D, nspectra=1)
        assert autos.shape == (1, 2, 64) and cross.shape == (1, 1, 64)
        dev, coh = pfbxc_ref.delay_figures(cross[0, 0], autos[0, 0], autos[0, 1])
        print("hop M / %d: phase within %.4f rad, coherence >= %.5f" % (hop_div, dev, coh))
        assert dev <= 0.02 and coh >= 0.99
        # the sign of the convention: the other order of the inputs runs the other way
        sw_a, sw_c = pfbxc_ref.pfbxc_ref(iqs[::-1], k, taps, K, D, nspectra=1)
        assert pfbxc_ref.delay_figures(sw_c[0, 0], sw_a[0, 0], sw_a[0, 1])[0] > 3.0


def test_delayed_captures_tell_the_pairs_apart():
    """The multi-receiver captures of the GPU suite, from the restatement alone: every pair's cross row is far from
    every other pair's and from its own conjugate, measured in the bound's own terms.  (With the delays 0, 1, 3, 6 the
    pairs (0,2) and (2,3) share the delay 3: their rows differ by the captures' own noise alone, which is still some
    thousand times the bound.)"""
    k, T, K, D = 6, 8, 65, 64
    taps = pfbspec_ref.designed_taps(k, T)
    iqs = pfbxc_ref.delayed_captures(4, pfbxc_ref.samples_needed(64, T, D, K, 1), seed=9)
    autos, cross = pfbxc_ref.pfbxc_ref(iqs, k, taps, K, D)
    for x in range(6):
        for other in [np.conj(cross[:, x])] + [cross[:, y] for y in range(6) if y != x]:
            wrong = cross.copy()
            wrong[:, x] = other
            assert pfbxc_ref.cross_ratio(wrong, autos, cross, k, K) > 100.0, x

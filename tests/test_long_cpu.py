"""CPU suite of include/rtlws_long.h (librtlws_long.so): the ABI, the descriptor rules, the kernels' resources from
the code-object metadata, and the transform's index maps restated in numpy.  No GPU is used."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest

import long_kernels as lk
from test_abi_cpu import _declared_functions, _exported, ROOT


def test_long_library_exports_its_header_and_nothing_else(built):
    built.long_lib()
    declared = _declared_functions("rtlws_long.h")
    assert len(declared) == 6
    assert _exported(built.LONG_LIB) == set(declared)
    assert set(built.LONG_SYMBOLS) == set(declared)
    # the getter the library reads the engine's stream with is part of librtlws_hip.so's interface
    assert "rtlws_engine_stream" in _exported(built.HIP_LIB) and "rtlws_engine_stream" in built.HIP_SYMBOLS
    assert "rtlws_engine_stream" in _declared_functions("rtlws_hip.h")
    # the drop-in library depends on it and finds it beside itself
    import subprocess
    dyn = subprocess.run(["readelf", "-d", built.AMD_LIB], capture_output=True, text=True, check=True).stdout
    assert "librtlws_long.so" in dyn and "$ORIGIN" in dyn


def test_long_descriptor_rules_need_no_gpu(built):
    ok = lambda **kw: built.long_supported(built.make_desc(**kw))
    for m in lk.SIZES:
        for inp in ("cu8", "cs32", "rf32"):
            for out in ("power_sum", "mean_db", "payload_u8"):
                for k_avg in (1, 3, 1000):
                    for flags in (0, built.FLAG_ROWS_F32):
                        assert ok(n_fft=1 << m, input=inp, output=out, k_avg=k_avg, flags=flags) == 1
                        assert built.long_last_error() == ""
    why = {}
    for name, kw in (("8192", dict(n_fft=8192)), ("12000", dict(n_fft=12000)), ("2^21", dict(n_fft=1 << 21)),
                     ("hann", dict(n_fft=1 << 16, window="hann")), ("cic", dict(n_fft=1 << 16, cic_r=8)),
                     ("k0", dict(n_fft=1 << 16, k_avg=0))):
        assert ok(**kw) == 0, name
        why[name] = built.long_last_error()
        assert why[name], name
    assert "power of two" in why["8192"] and "power of two" in why["12000"] and "2^20" in why["2^21"]
    assert "Hann" in why["hann"] and "CIC" in why["cic"] and "k_avg" in why["k0"]


def test_long_open_without_a_gpu_fails_with_a_text(built):
    """There is no CPU path: no engine, no plan."""
    if built.device_count() > 0:
        pytest.skip("a GPU is present")
    with pytest.raises(RuntimeError):
        built.Engine(0)
    L = built.long_lib()
    assert L.rtlws_long_open(None, ctypes.byref(built.make_desc(1 << 14)), 1) is None
    assert "no CPU path" in built.long_last_error()
    assert L.rtlws_long_workspace_bytes(None) == 0
    assert L.rtlws_long_run(None, None, 1, None, None) == -1
    L.rtlws_long_close(None)
    with pytest.raises(RuntimeError):
        built.Spectrum(16384)                                   # a served size: the engine is what is missing
    assert built.amd_lib().spectrum_alloc(12000) is None


def test_long_kernels_resources_and_coverage_table(built):
    """Every kernel of the library: no scratch, no VGPR spill, at most the 256 registers two wavefronts per SIMD
    have (512 threads per workgroup), and a GPU test that launches it (tests/long_kernels.py)."""
    from rtlws import codeobj
    built.long_lib()
    ks = codeobj.kernels(built.LONG_LIB)
    names = set()
    for k in ks:
        m = re.search(r"rtlws::lng::(long_pass_[ab]<\d+, \d+>)", k.get("demangled", ""))
        assert m, k.get("demangled", k["name"])
        names.add(m.group(1))
        assert k["vgpr_spill_count"] == 0 and k["private_segment_fixed_size"] == 0, m.group(1)
        assert not k.get("sgpr_spill_count", 0), m.group(1)
        assert k["vgpr_count"] + k.get("agpr_count", 0) <= 256, m.group(1)
        assert k["max_flat_workgroup_size"] == 512
    assert names == set(lk.LONG_KERNELS) and len(names) == 24
    src = open(os.path.join(ROOT, "tests", "test_long_gpu.py")).read()
    for test in set(lk.LONG_KERNELS.values()):
        fn, par = re.match(r"tests/test_long_gpu.py::(\w+)\[(\d+)\]$", test).groups()
        assert "def %s(" % fn in src and int(par) in lk.SIZES
    # every size reaches its two kernels through the split the header states
    for m in lk.SIZES:
        assert lk.log2_n1(m) + lk.log2_n2(m) == m and 7 <= lk.log2_n2(m) <= lk.log2_n1(m) <= 10
    # plain HIP C++: no inline assembly in the new sources
    for f in ("spectrum_long.hip", "long_shim.hip", "spectrum_long.h"):
        txt = open(os.path.join(ROOT, "rtl-ws_amd", "csrc", f)).read().lower()
        assert not re.search(r"asm\s*(volatile)?\s*\(", txt), f


def test_pass_a_workgroup_order_is_a_bijection():
    """xcd_chunked() of spectrum_long.hip: workgroup b runs logical tile (b % 8) * (n / 8) + b / 8 when the grid is a
    multiple of 8 -- XCD b % 8 gets one contiguous chunk -- and tile b otherwise: every tile exactly once."""
    chunked = lambda b, n: b if n % 8 else (b % 8) * (n // 8) + b // 8
    for n in (2, 6, 7, 8, 16, 24, 128, 8192, 8190):
        assert sorted(chunked(b, n) for b in range(n)) == list(range(n)), n
    assert [chunked(b, 32) for b in (0, 8, 16, 24)] == [0, 1, 2, 3]       # consecutive tiles on one XCD, in order


# ---- the transform restated in numpy -------------------------------------------------------------------------

def _roots(n, step, count):
    """long_shim.hip roots(): W_n^(i step), i < count, evaluated in long double and rounded once."""
    two_pi = np.longdouble("6.283185307179586476925286766559005768")
    a = -two_pi * (np.arange(count, dtype=np.longdouble) * step) / np.longdouble(n)
    return (np.cos(a).astype(np.float64) + 1j * np.sin(a).astype(np.float64))


def four_step(x, twl=None):
    """N = N1 N2, n = N2 n1 + n2, k = k1 + N1 k2, W_N^j = twh[j >> 10] * twl[j & 1023] (spectrum_long.hip).
    twl: another low table than the library's (tests/test_long_borders_cpu.py puts a defect there)."""
    N = x.size
    m = N.bit_length() - 1
    N1, N2 = 1 << lk.log2_n1(m), 1 << lk.log2_n2(m)
    twl, twh = _roots(N, 1, 1024) if twl is None else twl, _roots(N, 1024, N // 1024)
    a = np.fft.fft(x.reshape(N1, N2), axis=0)                          # [k1, n2]: the N1-point transforms over n1
    j = np.arange(N1)[:, None] * np.arange(N2)[None, :]                # n2 k1 < N
    ws = a * (twh[j >> 10] * twl[j & 1023])                            # the workspace, element (k1, n2)
    b = np.fft.fft(ws, axis=1)                                         # [k1, k2]: the N2-point transforms over n2
    return b.T.reshape(N)                                              # k = k1 + N1 k2


@pytest.mark.parametrize("m", [14, 15, 20])
def test_four_step_maps_and_two_table_twiddles(m):
    N = 1 << m
    rng = np.random.default_rng(m)
    x = rng.standard_normal(N) + 1j * rng.standard_normal(N)
    ref = np.fft.fft(x)
    err = np.abs(four_step(x) - ref).max() / np.abs(ref).max()
    print("m = %d: max err %.3g of the maximum" % (m, err))
    assert err <= 1e-12


def test_slot_rule_equals_the_oracle_row(oracle):
    """Slot of bin k = k1 + N1 k2 is k1 + N1 (k2 ^ N2/2) -- the fft-shift flips the top bit of k2 --, slot N/2 takes
    bin N-1 with the weights (K - k), slot N/2 - 1 is bin N-1's own: the oracle's row of K = 3 frames."""
    from rtlws import synth
    m, K = 14, 3
    N = 1 << m
    N1, N2 = 1 << lk.log2_n1(m), 1 << lk.log2_n2(m)
    iq = synth.tone_noise_iq(K, N, seed=8)
    row = np.zeros(N)
    k1, k2 = np.meshgrid(np.arange(N1), np.arange(N2), indexing="ij")
    k = (k1 + N1 * k2).ravel()
    slot = (k1 + N1 * (k2 ^ (N2 // 2))).ravel()
    assert np.array_equal(slot, (k + N // 2) % N)
    dc = 0.0
    for kf in range(K):
        x = (iq[kf, :, 0].astype(np.float64) - 128) / 128 + 1j * (iq[kf, :, 1].astype(np.float64) - 128) / 128
        pw = np.abs(four_step(x)) ** 2
        keep = k != 0                                                  # the owner of bin 0 stores nothing
        np.add.at(row, slot[keep], pw[k[keep]])
        dc += (K - kf) * pw[N - 1]                                     # carried by the owner of bin N-1
    assert row[N // 2] == 0.0
    row[N // 2] = dc
    ref = oracle.batch_spectra_u8(iq, N, K=K)[0]
    assert np.abs(row - ref).max() <= 1e-12 * ref.max()
    assert abs(row[N // 2] - ref[N // 2]) <= 1e-12 * ref[N // 2]
    assert abs(row[N // 2 - 1] - ref[N // 2 - 1]) <= 1e-12 * ref[N // 2 - 1]


# ---- the sub-transform of a tile: thread and LDS index maps, bank model -----------------------------------------

def _rev16(s):
    return 4 * (s & 3) + (s >> 2)


def _rev8(s):
    return 4 * (s & 1) + (s >> 1)


def _swz(pos, T):
    return pos ^ ((pos >> 2) & 1) if T == 8 else pos


def _out_k(log2l, gi, slot):
    if log2l == 7:
        return gi + 8 * (slot >> 3) + 16 * _rev8(slot & 7)
    if log2l == 8:
        return gi + 16 * _rev16(slot)
    R, G = 1 << (log2l - 8), 1 << (log2l - 4)
    c = gi + G * (slot // R)
    return (c >> 4) + 16 * (c & 15) + 256 * (slot % R)


def _tile_fft(x, accesses):
    """tile_fft<LOG2L> of spectrum_long.hip, thread by thread: x[L, T] in, X[L, T] out; every LDS access of a
    register slot is recorded as the list of the 512 threads' addresses (in 16-byte units)."""
    L, T = x.shape
    log2l = L.bit_length() - 1
    G = L // 16
    W = lambda M, e: np.exp(-2j * np.pi * e / M)
    lds = np.zeros(8192, dtype=complex)
    for pos in range(L):
        lds[_swz(pos, T) * T:_swz(pos, T) * T + T] = x[pos]
    t = np.arange(512)
    col, gi = t % T, t // T

    def stage16(base, stride, tw_m, tw_j):
        addr = [_swz(base + q * stride, T) * T + col for q in range(16)]
        accesses.extend(addr)
        Y = np.fft.fft(np.stack([lds[a] for a in addr]), axis=0)
        return addr, Y * (W(tw_m, tw_j[None, :] * np.arange(16)[:, None]) if tw_m else 1.0)

    addr, Y = stage16(gi, G, L, gi)
    for p in range(16):
        lds[addr[p]] = Y[p]
    out = np.zeros((L, T), dtype=complex)
    if log2l >= 9:
        M2 = L // 16
        J = M2 // 16
        j = gi % J
        addr, Y = stage16((gi // J) * M2 + j, J, M2, j)
        for p in range(16):
            lds[addr[p]] = Y[p]
        R, U = J, 16 // J
        for u in range(U):
            addr = [_swz(R * (gi + u * G) + q, T) * T + col for q in range(R)]
            accesses.extend(addr)
            Y = np.fft.fft(np.stack([lds[a] for a in addr]), axis=0)
            for q in range(R):
                out[_out_k(log2l, gi, R * u + q), col] = Y[q]
    elif log2l == 8:
        addr, Y = stage16(16 * gi, 1, 0, gi)
        for s in range(16):
            out[_out_k(8, gi, s), col] = Y[_rev16(s)]
    else:
        for u in range(2):
            addr = [(8 * (gi + 8 * u) + q) * T + col for q in range(8)]
            accesses.extend(addr)
            Y = np.fft.fft(np.stack([lds[a] for a in addr]), axis=0)
            for s in range(8):
                out[_out_k(7, gi, 8 * u + s), col] = Y[_rev8(s)]
    return out


@pytest.mark.parametrize("log2l", [7, 8, 9, 10])
def test_tile_fft_index_maps_and_lds_banks(log2l):
    """The thread -> (column, positions) maps of every register stage give the L-point DFT of each column, and every
    LDS access (ds_read_b128 / ds_write_b128 of one register slot by one wavefront) is conflict-free under
    tools/lds_sim.py's bank model -- with the bit-0 / bit-2 swizzle at T = 8 and, as the control, not without it."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    argv = sys.argv
    sys.argv = ["lds_sim"]
    try:
        import lds_sim
    finally:
        sys.argv = argv
    L = 1 << log2l
    T = 8192 // L
    rng = np.random.default_rng(log2l)
    x = rng.standard_normal((L, T)) + 1j * rng.standard_normal((L, T))
    accesses = []
    X = _tile_fft(x, accesses)
    ref = np.fft.fft(x, axis=0)
    assert np.abs(X - ref).max() <= 1e-12 * np.abs(ref).max()
    assert len(accesses) == (48 if log2l >= 9 else 32)

    def cycles(addr):
        rd = wr = 0
        for w in range(8):
            a = [2 * int(addr[64 * w + l]) for l in range(64)]           # float2 units
            rd += lds_sim.cycles(a, lds_sim.R128, 4, 64)
            wr += lds_sim.cycles(a, lds_sim.W128, 4, 32)
        return rd, wr

    for addr in accesses:
        assert cycles(addr) == (8 * 4, 8 * 8)                            # the ideal: 4 and 8 LDS cycles per wavefront
    # the tile loads: pass A (columns first), pass B (8 columns x 8 n2 per 64 lanes, columns first)
    t = np.arange(512)
    for i in range(16):
        e = t + 512 * i
        assert cycles(_swz(e // T, T) * T + e % T)[1] == 64
        rest = e >> 6
        n2, col = (rest % (L // 8)) * 8 + ((e >> 3) & 7), (rest // (L // 8)) * 8 + (e & 7)
        assert n2.max() < L and col.max() < T
        assert cycles(_swz(n2, T) * T + col)[1] == 64
    if T == 8:
        gi, col = t // T, t % T
        plain = (4 * gi + 1) * T + col                                   # the last stage's positions, unswizzled
        assert cycles(plain)[0] > 8 * 4

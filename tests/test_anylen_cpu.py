"""CPU suite of include/rtlws_anylen.h (librtlws_anylen.so): the ABI, the descriptor rules, the kernels' resources
from the code-object metadata, and Bluestein's algorithm as the kernels compute it restated in numpy against the
oracle.  No GPU is used."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import anylen_kernels as ak
import anylen_ref
import long_kernels as lk
from test_abi_cpu import _declared_functions, _exported, ROOT


def test_anylen_library_exports_its_header_and_nothing_else(built):
    built.anylen_lib()
    declared = _declared_functions("rtlws_anylen.h")
    assert len(declared) == 7
    assert _exported(built.ANYLEN_LIB) == set(declared)
    assert set(built.ANYLEN_SYMBOLS) == set(declared)
    dyn = subprocess.run(["readelf", "-d", built.ANYLEN_LIB], capture_output=True, text=True, check=True).stdout
    assert "librtlws_hip.so" in dyn and "$ORIGIN" in dyn
    # the drop-in library depends on it and finds it beside itself
    dyn = subprocess.run(["readelf", "-d", built.AMD_LIB], capture_output=True, text=True, check=True).stdout
    assert "librtlws_anylen.so" in dyn and "$ORIGIN" in dyn


def test_anylen_descriptor_rules_need_no_gpu(built):
    ok = lambda **kw: built.anylen_supported(built.make_desc(**kw))
    for n in (2, 3, 12000, 8192, 1 << 19):
        for inp in ("cu8", "cs32", "rf32"):
            for out in ("power_sum", "mean_db", "payload_u8"):
                for k_avg in (1, 3, 1000):
                    for flags in (0, built.FLAG_ROWS_F32):
                        assert ok(n_fft=n, input=inp, output=out, k_avg=k_avg, flags=flags) == 1
                        assert built.anylen_last_error() == ""
    why = {}
    for name, kw in (("1", dict(n_fft=1)), ("2^19+1", dict(n_fft=(1 << 19) + 1)), ("2^20", dict(n_fft=1 << 20)),
                     ("hann", dict(n_fft=12000, window="hann")), ("cic", dict(n_fft=12000, cic_r=8)),
                     ("k0", dict(n_fft=12000, k_avg=0)), ("flag", dict(n_fft=12000, flags=4))):
        assert ok(**kw) == 0, name
        why[name] = built.anylen_last_error()
        assert why[name], name
        assert built.anylen_conv_log2(built.make_desc(**kw)) == -1
    assert "at least 2" in why["1"] and "2^19" in why["2^19+1"] and "2^19" in why["2^20"]   # the text names the limit
    assert "Hann" in why["hann"] and "CIC" in why["cic"] and "k_avg" in why["k0"]
    m_of = lambda n: built.anylen_conv_log2(built.make_desc(n))
    assert [m_of(n) for n in (2, 3, 1000, 8191, 8192)] == [14] * 5
    assert m_of(8193) == 15 and m_of(12000) == 15 and m_of(16384) == 15 and m_of(16385) == 16
    assert m_of(262144) == 19 and m_of(262145) == 20 and m_of(1 << 19) == 20
    for n in (2, 37, 8192, 8193, 12000, 100000, 1 << 19):
        assert m_of(n) == anylen_ref.conv_log2(n) == ak.conv_log2(n) and (1 << m_of(n)) >= 2 * n - 1
    for m, n in ak.PARITY_N.items():                      # the GPU suite's sizes: above 2^15, the smallest N of each M
        assert m_of(n) == m
        assert n == 12000 or m_of(n - 1) == m - 1


def test_anylen_open_with_a_null_engine_fails_with_a_text(built):
    """There is no CPU path: no engine, no plan."""
    L = built.anylen_lib()
    assert L.rtlws_anylen_open(None, ctypes.byref(built.make_desc(12000)), 1) is None
    assert "no CPU path" in built.anylen_last_error()
    with pytest.raises(RuntimeError):
        built.AnyLenPlan(None, built.make_desc(12000))
    assert L.rtlws_anylen_workspace_bytes(None) == 0
    assert L.rtlws_anylen_run(None, None, 1, None, None) == -1 and "null plan" in built.anylen_last_error()
    L.rtlws_anylen_close(None)


def test_anylen_kernels_resources_and_coverage_table(built):
    """Every kernel of the library: 512 threads, no scratch, no spill, at most the 256 registers two wavefronts per
    SIMD have, and a GPU test that launches it (tests/anylen_kernels.py)."""
    from rtlws import codeobj
    built.anylen_lib()
    names = set()
    for k in codeobj.kernels(built.ANYLEN_LIB):
        m = re.search(r"rtlws::anylen::(anylen_pass_\w+<\d+(?:, \d+)?>)", k.get("demangled", ""))
        assert m, k.get("demangled", k["name"])
        names.add(m.group(1))
        assert k["vgpr_spill_count"] == 0 and k["private_segment_fixed_size"] == 0, m.group(1)
        assert not k.get("sgpr_spill_count", 0), m.group(1)
        assert k["vgpr_count"] + k.get("agpr_count", 0) <= 256, m.group(1)
        assert k["max_flat_workgroup_size"] == 512
    assert names == set(ak.ANYLEN_KERNELS) and len(names) == 32
    src = open(os.path.join(ROOT, "tests", "test_anylen_gpu.py")).read()
    for test in set(ak.ANYLEN_KERNELS.values()):
        fn, par = re.match(r"tests/test_anylen_gpu.py::(\w+)\[(\d+)\]$", test).groups()
        assert "def %s(" % fn in src and (int(par) in ak.PARITY_N.values() or int(par) in ak.SMALL_N)
    # each named test reaches the kernel through the split of its N's convolution size
    for name, test in ak.ANYLEN_KERNELS.items():
        m = ak.conv_log2(int(re.search(r"\[(\d+)\]", test).group(1)))
        length = int(re.search(r"<(\d+)", name).group(1))
        assert length == (lk.log2_n1(m) if "pass_a" in name else lk.log2_n2(m)), name
    # plain HIP C++: no inline assembly in the new sources
    for f in ("spectrum_anylen.hip", "anylen_shim.hip", "spectrum_anylen.h", "long_tile.h"):
        txt = open(os.path.join(ROOT, "rtl-ws_amd", "csrc", f)).read().lower()
        assert not re.search(r"asm\s*(volatile)?\s*\(", txt), f


def test_long_library_keeps_exactly_its_kernels(built):
    """The tile's device text moved into csrc/long_tile.h, which both libraries compile: librtlws_long.so still holds
    the kernels of tests/long_kernels.py and no other, and the two source files restate none of the shared text."""
    from rtlws import codeobj
    built.long_lib()
    names = set()
    for k in codeobj.kernels(built.LONG_LIB):
        m = re.search(r"rtlws::lng::(long_pass_[ab]<\d+, \d+>)", k.get("demangled", ""))
        assert m, k.get("demangled", k["name"])
        names.add(m.group(1))
    assert names == set(lk.LONG_KERNELS) and len(names) == 24
    csrc = os.path.join(ROOT, "rtl-ws_amd", "csrc")
    tile = open(os.path.join(csrc, "long_tile.h")).read()
    for fn in ("swz", "fft8", "out_k", "tile_fft", "load_sample", "store_value", "xcd_chunked"):
        assert len(re.findall(r"^__device__ __forceinline__ \w+ %s\(" % fn, tile, flags=re.M)) == 1, fn
        for f in ("spectrum_long.hip", "spectrum_anylen.hip"):
            txt = open(os.path.join(csrc, f)).read()
            assert '#include "long_tile.h"' in txt
            assert not re.search(r"^__device__ .*\b%s\(" % fn, txt, flags=re.M), (f, fn)


# ---- the algorithm restated in numpy against the oracle -----------------------------------------------------------

def _oracle_rows(oracle, add, frames, N, K):
    rows = np.zeros((len(frames) // K, N))
    for f, frame in enumerate(frames):
        assert add(N, frame, rows[f // K]) == 0
    return rows


@pytest.fixture(scope="module")
def small_cases(oracle):
    """(N, K) -> (cu8 frames, the oracle's rows), computed once."""
    from rtlws import synth
    cases = {}
    for N in (37, 1000, 1001):
        iq = synth.tone_noise_iq(6, N, seed=N)
        for K in (1, 3):
            cases[N, K] = (iq, oracle.batch_spectra_u8(iq, N, K=K, nthreads=8))
    return cases


@pytest.mark.parametrize("N", [37, 1000, 1001])
def test_restated_bluestein_equals_the_oracle(small_cases, oracle, N):
    """The integer chirp, the wrap of b, zero padding, M-point transforms, the inverse as the forward transform of
    the conjugate, the dropped final chirp, the slot rule for odd N and the (K - k) DC weights: the oracle's rows
    under the strict metric."""
    from helpers import rel_err, EPS_STRICT, TOL_F64
    h = N // 2
    for K in (1, 3):
        iq, ref = small_cases[N, K]
        got = anylen_ref.bluestein_rows(iq, N, K)
        e = rel_err(got, ref, EPS_STRICT).max()
        print("N = %d K = %d: restated Bluestein max strict rel err %.3g" % (N, K, e))
        assert e <= TOL_F64
        for slot in (N - h, N - h - 1):                                # the DC slot and its left neighbour (bin N-1)
            assert abs(got[:, slot] - ref[:, slot]).max() <= 1e-12 * ref[:, slot].max()
    rng = np.random.default_rng(N)
    s32 = rng.integers(-4000, 4000, size=(2, N, 2), dtype=np.int32)
    f32 = rng.standard_normal((2, N)).astype(np.float32)
    for inp, data, add in (("cs32", s32, oracle.spectrum_add_cmplx_s32), ("rf32", f32, oracle.spectrum_add_real_f32)):
        ref = _oracle_rows(oracle, add, data, N, 2)
        assert rel_err(anylen_ref.bluestein_rows(data, N, 2, inp), ref, EPS_STRICT).max() <= TOL_F64, inp
        assert rel_err(anylen_ref.rows(data, N, 2, inp), ref, EPS_STRICT).max() <= TOL_F64, inp


@pytest.mark.parametrize("N", [37, 1000, 1001])
def test_numpy_reference_equals_the_oracle(small_cases, N):
    """tests/anylen_ref.rows (np.fft.fft and the row rules), the GPU suite's reference above 2048 points."""
    from helpers import rel_err, EPS_STRICT, TOL_F64
    h = N // 2
    for K in (1, 3):
        iq, ref = small_cases[N, K]
        got = anylen_ref.rows(iq, N, K)
        e = rel_err(got, ref, EPS_STRICT).max()
        print("N = %d K = %d: np.fft reference max strict rel err %.3g" % (N, K, e))
        assert e <= 1e-11                                               # a tenth of TOL_F64: it serves as a reference
        for slot in (N - h, N - h - 1):
            assert abs(got[:, slot] - ref[:, slot]).max() <= 1e-13 * ref[:, slot].max()


def test_chirp_uses_the_exact_integer_phase():
    """q = n^2 mod 2N in integers: at N = 2^19 - 1 the product n^2 exceeds 2^37, where n * n / N in double would lose
    the phase; the table agrees with long-double evaluation of exact residues from Python integers."""
    N = (1 << 19) - 1
    w = anylen_ref.chirp(N)
    for n in (0, 1, 2, 1000, 262143, 400001, N - 1):
        q = (n * n) % (2 * N)
        a = -np.longdouble("3.141592653589793238462643383279502884") * np.longdouble(q) / np.longdouble(N)
        assert w[n] == complex(float(np.cos(a)), float(np.sin(a))), n
    assert np.abs(np.abs(w) - 1).max() <= 2.3e-16

"""CPU suite: the twiddle and window tables of the spectrum kernels (rtl-ws_amd/csrc/twiddle_tables.cpp).

The unit is host-only: it is compiled here with g++ and a test-only driver (tests/tools/dump_tables.cpp) that
writes every table to a file.  Each (table, N) must hash to tests/golden/twiddle_tables_sha256.json -- the
tables the f32 and f64 kernels were validated with, so that a change to them cannot hide until a GPU parity
run -- and the f64 tables are checked against an independent numpy.longdouble evaluation."""
import hashlib
import json
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "rtl-ws_amd", "csrc")
SIZES = (2, 3, 5, 6, 1000, 1024, 2048, 4096, 8192)
TWO_PI = np.longdouble("6.283185307179586476925286766559005768")


@pytest.fixture(scope="module")
def tables(tmp_path_factory):
    d = tmp_path_factory.mktemp("tables")
    exe = str(d / "dump_tables")
    b = subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I" + CSRC,
                        os.path.join(CSRC, "twiddle_tables.cpp"), os.path.join(ROOT, "tests", "tools", "dump_tables.cpp"),
                        "-o", exe], capture_output=True, text=True, timeout=300)
    assert b.returncode == 0, b.stdout + b.stderr
    r = subprocess.run([exe, str(d)] + [str(n) for n in SIZES], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    out = {}
    for f in os.listdir(d):
        if f.endswith(".bin"):
            prec, rest = f[:-4].split("_", 1)
            name, n = rest.rsplit("_", 1)
            out["%s/%s/%s" % (prec, name, n)] = (d / f).read_bytes()
    return out


def _f64(tables, key):
    """A double2 table as complex128."""
    return np.frombuffer(tables[key], dtype=np.float64).view(np.complex128)


def test_tables_are_bit_identical_to_the_validated_ones(tables):
    with open(os.path.join(ROOT, "tests", "golden", "twiddle_tables_sha256.json")) as f:
        want = json.load(f)
    assert set(tables) == set(want)
    bad = [k for k in sorted(want) if hashlib.sha256(tables[k]).hexdigest() != want[k]]
    assert not bad, "tables changed: %s" % bad


def _unit_roots(num, den):
    """exp(-2 pi i num/den) in long double, axis values exact: (cos, sin) as two longdouble arrays."""
    num = np.asarray(num, dtype=np.int64) % den
    a = -TWO_PI * num.astype(np.longdouble) / np.longdouble(den)
    c, s = np.cos(a), np.sin(a)
    for q, cv, sv in ((0, 1, 0), (den / 4, 0, -1), (den / 2, -1, 0), (3 * den / 4, 0, 1)):
        hit = num == q
        c[hit], s[hit] = cv, sv
    return c, s, num


def _check_roots(got, c, s, num, den):
    """axis entries exact, every other entry within 1 ulp of the long double value"""
    axis = (4 * num) % den == 0
    assert axis.any()
    assert np.array_equal(got.real[axis], c[axis].astype(np.float64))
    assert np.array_equal(got.imag[axis], s[axis].astype(np.float64))
    for part, ref in ((got.real, c), (got.imag, s)):
        ref64 = ref.astype(np.float64)
        assert np.all(np.abs(part - ref64) <= np.spacing(np.abs(ref64)))


@pytest.mark.parametrize("n", [1000, 1024, 4096, 8192])
def test_f64_direct_twiddles_against_long_double(tables, n):
    k = np.arange(n)
    _check_roots(_f64(tables, "f64/tw64/%d" % n), *_unit_roots(k, n), n)


@pytest.mark.parametrize("n", [1024, 2048, 4096])
def test_f64_fused_twiddles_against_long_double(tables, n):
    rev16 = np.array([4 * (s & 3) + (s >> 2) for s in range(16)])
    e = (np.arange(n // 16)[:, None] * rev16[None, :]).ravel()
    tw1u = _f64(tables, "f64/tw1u_64/%d" % n)
    _check_roots(tw1u, *_unit_roots(e, n), n)
    # the 1/128 input scale is a power of two: folded in exactly
    assert np.array_equal(_f64(tables, "f64/tw1_64/%d" % n), tw1u / 128)
    t = np.arange(n // 16)
    c, s, _ = _unit_roots(-t, n)
    hcs = _f64(tables, "f64/hann_cs64/%d" % n)
    assert np.all(np.abs(hcs.real - (c / 2).astype(np.float64)) <= np.spacing(np.abs(hcs.real)))
    assert np.all(np.abs(hcs.imag - (s / 2).astype(np.float64)) <= np.spacing(np.abs(hcs.imag)))


def test_f32_twiddles_keep_their_libm_axis_values(tables):
    """The f32 tables take cos / sin in double with no exact axes (W_N^(N/4) = 6.1e-17 - 1j): kept as
    the f32 kernels were validated; the f64 tables store the exact axis values."""
    for n in (1000, 8192):       # the direct kernel's sizes: tw1[k] = W_N^k
        tw = np.frombuffer(tables["f32/tw1/%d" % n], dtype=np.float32).view(np.complex64)
        assert tw[n // 4].real != 0 and abs(tw[n // 4].real) < 1e-7 and tw[n // 4].imag == -1
        assert _f64(tables, "f64/tw64/%d" % n)[n // 4] == -1j

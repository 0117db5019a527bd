"""Every spectrum instantiation, launched through the C ABI and held to the f64 oracle.

tests/kernel_matrix.py lists one descriptor per template instantiation of the six spectrum kernels (and a few more
for the runtime-only fields of the row-per-workgroup kernels); tests/test_kernel_matrix_cpu.py holds that list to
the library's code objects.  Here each case runs under the engine options it names, on four rows:
  0  a constant row (u8 128, or zeros): exact zeros in power sums, -inf in dB rows, payload bytes 0;
  1  a row alternating between the extremes (u8 0/255 per decimated sample, int32 min/max, +-3e4): the largest
     butterfly sums;
  2  a pure tone: the widest dynamic range;
  3  tone + noise at K = 1, uniform bytes (full-range int32, Gaussian f32) at K > 1.
Bounds are the ones the rest of the suite holds each path to (tests/helpers.py).  The test is parametrized by
kernel family and N; a failure lists the instantiation and descriptor of every case that broke."""
import contextlib
import zlib

import numpy as np
import pytest

import kernel_matrix as km
from helpers import rel_err, eps_for, f32_db_bad, f32_payload_bad, EPS_K1, EPS_STRICT, TOL, TOL_F64

pytestmark = pytest.mark.gpu
ROWS = 4
ONE_F32_ROUNDING = 2.0 ** -24 * 1.001         # half an ulp, relative
I32_MIN, I32_MAX = -2 ** 31, 2 ** 31 - 1


def _frames(c):
    """The case's input (ROWS * K frames, row-major by row) and the oracle's f64 rows of K-frame sums."""
    from oracle import pyoracle as po
    from rtlws import synth
    K, N = c.K, c.N
    rng = np.random.default_rng(zlib.crc32(c.label().encode()))
    seed = int(rng.integers(1 << 30))
    w = synth.hann(N) if c.window == "hann" else None
    if c.input == "cu8":
        R = max(c.cic_r, 1)
        data = np.empty((ROWS, K, N * R, 2), dtype=np.uint8)
        data[0] = 128
        data[1] = np.where((np.arange(N * R) // R) % 2 == 1, 255, 0)[:, None]
        data[2] = synth.pure_tone_iq(K, N * R, seed=seed)
        data[3] = synth.tone_noise_iq(1, N * R, seed=seed + 1) if K == 1 else synth.uniform_iq(K, N * R, seed=seed + 1)
        data = data.reshape(ROWS * K, N * R, 2)
        if c.cic_r > 1:
            return data, po.batch_spectra_cic_u8(data, N, c.cic_r, K=K, window=w)
        return data, po.batch_spectra_u8(data, N, K=K, window=w)
    n = np.arange(N)
    f, ph = rng.uniform(-0.5, 0.5), rng.uniform(0, 2 * np.pi)
    if c.input == "cs32":
        data = np.empty((ROWS, K, N, 2), dtype=np.int32)
        data[0] = 0
        data[1, :, :, 0] = np.where(n % 2 == 1, I32_MAX, I32_MIN)
        data[1, :, :, 1] = np.where(n % 2 == 1, I32_MIN, I32_MAX)
        tone = 1e6 * np.exp(1j * (2 * np.pi * f * n + ph))
        data[2, :, :, 0], data[2, :, :, 1] = np.round(tone.real), np.round(tone.imag)
        data[3] = rng.integers(I32_MIN, I32_MAX, size=(K, N, 2), dtype=np.int64).astype(np.int32)
        add = po.spectrum_add_cmplx_s32
    else:
        data = np.empty((ROWS, K, N), dtype=np.float32)
        data[0] = 0
        data[1] = np.where(n % 2 == 1, 3e4, -3e4)
        data[2] = np.sin(2 * np.pi * f * n + ph)
        data[3] = rng.standard_normal((K, N))
        add = po.spectrum_add_real_f32
    ref = np.zeros((ROWS, N))
    for r in range(ROWS):
        for k in range(K):
            assert add(N, data[r, k], ref[r], window=w) == 0
    return data.reshape((ROWS * K,) + data.shape[2:]), ref


def _run(engine, c, data, rows_f32=None):
    with contextlib.ExitStack() as st:
        for name, value in c.opts:
            st.enter_context(engine.option(name, value))
        return engine.spectra(data, c.N, k_avg=c.K, input=c.input, window=c.window, output=c.output,
                              cic_r=c.cic_r, gain_db=c.gain_db, f64=c.f64,
                              rows_f32=c.rows_f32 if rows_f32 is None else rows_f32)


def _threads(engine, built, c):
    desc = built.make_desc(c.N, c.K, c.input, c.window, c.output, c.cic_r, c.gain_db)
    with contextlib.ExitStack() as st:
        for name, value in c.opts:
            st.enter_context(engine.option(name, value))
        rc, _, threads, _ = engine.grid(desc, ROWS * c.K)
    assert rc == 0
    return threads


def _payload_cap(ref_row, K, gain):
    """The highest byte a bin at or below the strict floor (1e-9 of the row maximum) may show: its power is only
    known to be below the floor (the f32 transform's absolute error, about 4e-15 of the row maximum in power, is
    orders smaller; DESIGN.md, "Error budget")."""
    g = 10.0 ** (int(gain / 10))
    with np.errstate(divide="ignore"):
        d = 10 * np.log10(g * 1e-9 * ref_row.max() / K)
    return int(np.clip(np.floor(d) + 1, 0, 255)) if np.isfinite(d) else 0


def _check_f32(engine, built, c, got, ref):
    """Problems of an rtlws_spectra_batch result, as strings (empty: the case passes)."""
    bad = []
    fused = c.N in km.FUSED_N
    N, K = c.N, c.K
    if fused:
        v2 = km.instantiation(c)[0] == "spectra_fused_v2"
        threads = _threads(engine, built, c)
        if threads != (N // 32 if v2 else N // 16):
            bad.append("grid reports %d threads per workgroup" % threads)
    if c.output == "power_sum":
        assert got.dtype == np.float32
        if got[0].any():
            bad.append("constant row not all zero")
        tol = TOL if fused else 1e-3
        for r in range(1, ROWS):
            eps = eps_for(K) if (r == 3 and fused) else EPS_K1
            e = rel_err(got[r], ref[r], eps).max()
            if e > tol:
                bad.append("row %d rel err %.3g (eps %g)" % (r, e, eps))
        if K == 1 and not np.array_equal(got[:, N // 2], got[:, N // 2 - 1]):
            bad.append("K = 1 DC slot differs from slot N/2 - 1")
    elif c.output == "mean_db":
        if not np.all(got[0] == -np.inf):
            bad.append("constant row not -inf dB")
        m = f32_db_bad(got, ref, K, fused)
        if m.any():
            with np.errstate(divide="ignore"):
                bad.append("%d dB values outside the budget, worst %.3g dB" % (
                    m.sum(), float(np.abs(got - 10 * np.log10(ref / K))[m].max())))
    else:
        from oracle import pyoracle as po
        assert got.dtype == np.uint8
        for r in range(ROWS):
            want = po.spectrum_payload(ref[r], K, c.gain_db)
            # every byte of the constant row; elsewhere the bins above the strict floor, and the rest (the empty
            # bins of the alternating rows among them, which the oracle may hold at exactly 0) under the floor's byte
            judged = ref[r] > 1e-9 * ref[r].max() if r else np.ones(N, dtype=bool)
            m = f32_payload_bad(got[r], want, ref[r], K, c.gain_db, fused) & judged
            m |= ~judged & (got[r] > _payload_cap(ref[r], K, c.gain_db))
            if m.any():
                bad.append("row %d: %d payload bytes off, e.g. bin %d: %d, want %d" % (
                    r, m.sum(), int(np.argmax(m)), got[r][m][0], want[m][0]))
    return bad


def _check_f64(engine, c, data, got, ref):
    bad = []
    N, K = c.N, c.K
    ok = ref > 1e-9 * ref.max(axis=1, keepdims=True)
    with np.errstate(divide="ignore"):
        want_db = 10 * np.log10(ref / K)
    if c.output == "payload_u8":
        from oracle import pyoracle as po
        want = np.stack([po.spectrum_payload(r, K, c.gain_db) for r in ref])
        if got.dtype != np.uint8 or not np.array_equal(got, want):
            m = got != want
            bad.append("%d payload bytes differ, max by %d" % (m.sum(), int(np.abs(got.astype(int) - want)[m].max())))
        return bad
    if c.rows_f32:
        if got.dtype != np.float32:
            return ["rows_f32 rows are %s" % got.dtype]
        g64 = _run(engine, c, data, rows_f32=False)
        with np.errstate(over="ignore"):
            if not np.array_equal(got, g64.astype(np.float32), equal_nan=True):
                bad.append("rows_f32 rows are not the f64 rows rounded once")
    if c.output == "power_sum":
        if got[0].any():
            bad.append("constant row not all zero")
        e = rel_err(got, ref, EPS_STRICT).max()
        if e > (ONE_F32_ROUNDING if c.rows_f32 else TOL_F64):
            bad.append("strict rel err %.3g" % e)
        if K == 1 and not np.array_equal(got[:, N // 2], got[:, N // 2 - 1]):
            bad.append("K = 1 DC slot differs from slot N/2 - 1")
    else:
        if not np.all(got[0] == -np.inf):
            bad.append("constant row not -inf dB")
        with np.errstate(invalid="ignore"):
            err = np.abs(got.astype(np.float64) - want_db)[ok]
        lim = 1e-9 + (ONE_F32_ROUNDING * np.abs(want_db[ok]) if c.rows_f32 else 0.0)
        if np.any(err > lim):
            bad.append("dB error %.3g" % float(err.max()))
    return bad


def _cases(fam):
    return [c for c in km.CASES if km.family(c) == fam]


@pytest.mark.parametrize("fam", km.FAMILIES)
def test_every_instantiation_against_the_oracle(engine, built, fam):
    failures = []
    for c in _cases(fam):
        data, ref = _frames(c)
        got = _run(engine, c, data)
        assert got.shape == (ROWS, c.N), c.label()
        bad = _check_f64(engine, c, data, got, ref) if c.f64 else _check_f32(engine, built, c, got, ref)
        failures += ["%s%s [%s]: %s" % (km.instantiation(c)[0], km.instantiation(c)[1], c.label(), b) for b in bad]
    assert not failures, "\n".join(failures)


def test_payload_cases_reach_both_clamps():
    """The matrix's payload gains drive the oracle's bytes (which every payload case is held to) into both clamps."""
    from oracle import pyoracle as po
    seen = set()
    for c in km.CASES:
        if c.output == "payload_u8":
            _, ref = _frames(c)
            for r in ref:
                seen.update(np.unique(po.spectrum_payload(r, c.K, c.gain_db)).tolist())
    assert 0 in seen and 255 in seen, sorted(seen)


def test_payload_from_sums_kernels(engine, built, oracle):
    """rtlws_payload_from_sums (payload_kernel, f32 sums) and rtlws_payload_from_sums_f64 (payload_f64_kernel) on
    sums that reach both clamps, zero, and values next to integer dB."""
    rng = np.random.default_rng(5)
    sums = np.concatenate([[0.0, 1e-30, 1.0, 3e37], 10.0 ** rng.uniform(-5, 30, size=4093)])
    L = built.hip_lib()
    for gain, count in ((0, 1), (40, 6), (-30, 2)):
        for f64 in (False, True):
            s = sums.astype(np.float64 if f64 else np.float32)
            d_s, d_o = engine.upload(s), engine.alloc(s.size)
            fn = L.rtlws_payload_from_sums_f64 if f64 else L.rtlws_payload_from_sums
            assert fn(engine.h, d_s.ptr, s.size, count, gain, d_o.ptr, None) == 0, built.last_error()
            got = engine.download(d_o, np.uint8, (s.size,))
            want = oracle.spectrum_payload(s.astype(np.float64), count, gain)
            if f64:
                assert np.array_equal(got, want), gain
            else:
                assert not f32_payload_bad(got, want, s.astype(np.float64), count, gain).any(), gain
            assert got[0] == 0 and (gain < 0 or got[3] == 255)

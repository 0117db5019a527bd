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
kernel family and N; a failure lists the instantiation and descriptor of every case that broke.

Four rows are one trip of a persistent kernel's row loop.  test_every_persistent_instantiation_past_its_grid_cap runs
every persistent case again with its grid pinned at one workgroup per CU and 2 * cu_count + 19 rows (three trips for
the first 19 workgroups, two for the rest, a ragged end), each row a copy of one of the four above, placed so that a
workgroup that fetches, keeps or stores a wrong row on a later trip shows (tests/persistent_trips.py).  A row depends on
its own K frames only and every trip runs the same instructions, so the long batch must repeat the four-row launch
bit for bit; the four-row launch is held to the oracle as above."""
import contextlib
import functools
import zlib

import numpy as np
import pytest

import kernel_matrix as km
import persistent_trips as pt
from helpers import rel_err, eps_for, f32_db_bad, f32_payload_bad, EPS_K1, EPS_STRICT, TOL, TOL_F64

pytestmark = pytest.mark.gpu
ROWS = 4
ONE_F32_ROUNDING = 2.0 ** -24 * 1.001         # half an ulp, relative
I32_MIN, I32_MAX = -2 ** 31, 2 ** 31 - 1


@functools.lru_cache(maxsize=None)
def _frames(c):
    """The case's input (ROWS * K frames, row-major by row) and the oracle's f64 rows of K-frame sums: made once per
    case, shared by the tests of this module, read-only."""
    data, ref = _make_frames(c)
    data.flags.writeable = ref.flags.writeable = False
    return data, ref


def _make_frames(c):
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


def _pool(c, P):
    """_frames(c), and for P > ROWS (spectra_f64_1024x at eight wavefronts per workgroup, cmplx_u8 frames without a
    CIC factor or window) P - ROWS more row groups, tone + noise and uniform bytes in turn, with the oracle's rows."""
    data, ref = _frames(c)
    if P <= ROWS:
        return data, ref
    from oracle import pyoracle as po
    from rtlws import synth
    assert c.input == "cu8" and c.cic_r <= 1 and c.window == "rect"
    seed = zlib.crc32((c.label() + " pool").encode()) % (1 << 30)
    extra = np.concatenate([(synth.uniform_iq if i % 2 else synth.tone_noise_iq)(c.K, c.N, seed=seed + i)
                            for i in range(P - ROWS)])
    return np.concatenate([data, extra]), np.concatenate([ref, po.batch_spectra_u8(extra, c.N, K=c.K)])


def _out_dtype(c):
    return np.uint8 if c.output == "payload_u8" else np.float64 if (c.f64 and not c.rows_f32) else np.float32


def _desc(built, c, grid=False):
    """The case's descriptor; grid: as rtlws_spectra_grid takes it (RTLWS_FLAG_F64 names the f64 entry point's plan)."""
    flags = (built.FLAG_ROWS_F32 if c.f64 and c.rows_f32 else 0) | (built.FLAG_F64 if c.f64 and grid else 0)
    return built.make_desc(c.N, c.K, c.input, c.window, c.output, c.cic_r, c.gain_db, flags)


def _run_gathered(engine, built, c, pool, pm):
    """The batch whose row g is a copy of the pool's row group pm[g], gathered on the device from the uploaded pool
    (runs of consecutive pool rows in one copy), launched under the options in force."""
    pool = np.ascontiguousarray(pool)
    rows, row_in = len(pm), pool.nbytes // (pool.shape[0] // c.K)
    dt = _out_dtype(c)
    d_pool, d_in = engine.upload(pool), engine.alloc(rows * row_in)
    d_out = engine.alloc(rows * c.N * np.dtype(dt).itemsize)
    try:
        g = 0
        while g < rows:
            n = 1
            while g + n < rows and pm[g + n] == pm[g + n - 1] + 1:
                n += 1
            rc = built.hip_lib().rtlws_copy_d2d(engine.h, d_in.ptr + g * row_in, d_pool.ptr + pm[g] * row_in, n * row_in,
                                                None)
            assert rc == 0, built.last_error()
            g += n
        (engine.spectra_batch_f64 if c.f64 else engine.spectra_batch)(_desc(built, c), d_in, rows * c.K, d_out)
        return engine.download(d_out, dt, (rows, c.N))
    finally:
        for b in (d_pool, d_in, d_out):
            b.free()


def _first_difference(big, small, pm, blocks):
    """None where big[g] is small[pm[g]] bit for bit for every row g, else where it first is not."""
    u = {1: np.uint8, 4: np.uint32, 8: np.uint64}[big.dtype.itemsize]
    neq = big.view(u) != small.view(u)[pm]
    if not neq.any():
        return None
    g = int(np.argmax(neq.any(axis=1)))
    k = int(np.argmax(neq[g]))
    return "%d of %d rows differ from the one-trip launch; first row %d (trip %d of workgroup %d, pool row %d) at bin %d: " \
           "%r, one-trip launch %r" % (int(neq.any(axis=1).sum()), len(pm), g, g // blocks, g % blocks, pm[g], k, big[g, k],
                                       small[pm[g], k])


@pytest.mark.parametrize("fam", pt.FAMILIES)
def test_every_persistent_instantiation_past_its_grid_cap(engine, built, fam):
    cus = engine.get_option("cu_count")
    failures, shapes = [], set()
    cases = [c for c in _cases(fam) if pt.persistent(c)]
    assert cases and len(cases) == sum(1 for c in pt.CASES if km.family(c) == fam)
    for c in cases:
        inst = "%s%s [%s]" % (km.instantiation(c)[0], km.instantiation(c)[1], c.label())
        x8 = pt.is_x8(c)
        rows = pt.x8_rows_for(cus) if x8 else pt.rows_for(cus)
        with contextlib.ExitStack() as st:
            for name, value in c.opts + (pt.pin_option(c),):
                st.enter_context(engine.option(name, value))
            # the grid is what the test says it is: one workgroup per CU, and rows for a second and a third trip
            rc, blocks, _, _ = engine.grid(_desc(built, c, grid=True), rows * c.K)
            assert rc == 0 and blocks == cus, (inst, rc, blocks, cus)
            assert rows >= 2 * blocks + 1 and -(-rows // blocks) >= 3, (inst, rows, blocks)
            if x8:   # rows are dealt through the LDS counter after the first eight: every workgroup gets there
                assert rows // blocks > pt.X_STATIC_ROWS, (inst, rows, blocks)
                pm, P = pt.x8_pool_map(blocks, rows)
            else:
                pm, P = pt.pool_map(blocks, rows), ROWS
            shapes.add((blocks, rows, -(-rows // blocks), rows // blocks))
            data, ref = _pool(c, P)
            small = _run(engine, c, data)               # at most one trip per workgroup
            assert small.shape == (P, c.N), inst
            bad = _check_f64(engine, c, data, small, ref) if c.f64 else _check_f32(engine, built, c, small, ref)
            if len({r.tobytes() for r in small}) != P:   # else a row taken for another could go unseen
                bad.append("the pool's %d output rows are not pairwise different" % P)
            big = _run_gathered(engine, built, c, data, pm)
            diff = _first_difference(big, small, pm, blocks)
        failures += ["%s: %s" % (inst, b) for b in bad + ([diff] if diff else [])]
    print("%s: %d cases, each at %s (workgroups, rows, most and fewest trips of a workgroup)" % (
        fam, len(cases), sorted(shapes)))
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

"""GPU suite of include/rtlws_anylen.h: f64 power spectra of any frame length 2 .. 2^19 (Bluestein over the four-step
transform, rtl-ws_amd/csrc/spectrum_anylen.hip) under the strict metric of the f64 batch tests (helpers.rel_err with
EPS_STRICT: 1e-10 over a floor of 1e-9 of the row maximum; f32 rows 6.0e-8).  The reference is the f64 oracle up
to 2048 points and tests/anylen_ref.rows (np.fft.fft and the row rules, pinned to the oracle by
tests/test_anylen_cpu.py) above: the oracle's direct long-double sum takes minutes per frame at 10^5 points."""
import numpy as np
import pytest

import anylen_kernels as ak
import anylen_ref
from helpers import rel_err, EPS_STRICT, TOL_F64

pytestmark = pytest.mark.gpu

TOL_ROWS_F32 = 6.0e-8
ORACLE_MAX_N = 2048


def _check(what, got, ref, tol):
    e = rel_err(got, ref, EPS_STRICT).max()
    print("%s: max strict rel err %.3g (bound %.1e)" % (what, e, tol))
    assert e <= tol, what


def _oracle_rows(oracle, add, frames, N, K):
    """K sequential oracle.spectrum_add_* calls per row into a zeroed buffer."""
    rows = np.zeros((len(frames) // K, N))
    for f, frame in enumerate(frames):
        assert add(N, frame, rows[f // K]) == 0
    return rows


def _ref_rows(oracle, data, N, K, input="cu8"):
    if N > ORACLE_MAX_N:
        return anylen_ref.rows(data, N, K, input)
    if input == "cu8":
        return oracle.batch_spectra_u8(data, N, K=K, nthreads=8)
    return _oracle_rows(oracle, oracle.spectrum_add_cmplx_s32 if input == "cs32" else oracle.spectrum_add_real_f32,
                        data, N, K)


def _payload(ps, K, gain_db):
    """src/cbb_main.c:112,125-128 on a row of K-frame sums, where the oracle's rows are not at hand."""
    g = 10.0 ** (int(gain_db / 10))
    with np.errstate(divide="ignore"):
        d = 10 * np.log10(np.abs(g * ps / K))
    return np.where(d >= 0, np.minimum(d, 255), 0).astype(np.int64).astype(np.uint8)


@pytest.mark.parametrize("N", sorted(ak.PARITY_N.values()))
def test_parity_by_conv_size(engine, oracle, N):
    """One N per convolution size 2^15 .. 2^20: the three inputs, the three row kinds, K = 1 and 3, two rows -- every
    pass-A length 8 .. 10 and every pass-B length 7 .. 10 on both sides of the product (tests/anylen_kernels.py)."""
    from rtlws import synth
    F = 6
    rng = np.random.default_rng(N)
    iq = synth.tone_noise_iq(F, N, seed=N % 1000)
    s32 = rng.integers(-4000, 4000, size=(F, N, 2), dtype=np.int32)
    f32 = rng.standard_normal((F, N)).astype(np.float32)
    for K in (1, 3):
        ref = anylen_ref.rows(iq, N, K)
        _check("cu8 N=%d K=%d f64 rows" % (N, K), engine.spectra_anylen(iq, N, k_avg=K), ref, TOL_F64)
        _check("cu8 N=%d K=%d f32 rows" % (N, K), engine.spectra_anylen(iq, N, k_avg=K, rows_f32=True), ref, TOL_ROWS_F32)
    pay = engine.spectra_anylen(iq, N, k_avg=3, output="payload_u8", gain_db=9)
    assert pay.shape == (2, N)
    for r in range(2):
        assert np.array_equal(pay[r], _payload(ref[r], 3, 9)), (N, r)
    for K in (1, 3):
        ref = anylen_ref.rows(s32, N, K, "cs32")
        _check("cs32 N=%d K=%d f64 rows" % (N, K), engine.spectra_anylen(s32, N, k_avg=K, input="cs32"), ref, TOL_F64)
        ref = anylen_ref.rows(f32, N, K, "rf32")
        _check("rf32 N=%d K=%d f64 rows" % (N, K), engine.spectra_anylen(f32, N, k_avg=K, input="rf32"), ref, TOL_F64)
        _check("rf32 N=%d K=%d f32 rows" % (N, K), engine.spectra_anylen(f32, N, k_avg=K, input="rf32", rows_f32=True),
               ref, TOL_ROWS_F32)


@pytest.mark.parametrize("N", ak.SMALL_N)
def test_small_and_awkward_lengths(engine, oracle, N):
    """M = 2^14, where most of the tile is padding: N = 2 and 3 (one workgroup of pass 4 holds every bin), a prime,
    even and odd lengths, the largest prime below 8192 and 8192 itself -- against the oracle up to 2047 points, the
    numpy reference above, and at 8192 also against rtlws_spectra_batch_f64 on the same frames."""
    from rtlws import synth
    F = 6 if N <= 1001 else 3
    rng = np.random.default_rng(N)
    iq = synth.tone_noise_iq(F, N, seed=N % 1000 + 1)
    for K in (1, 3):
        ref = _ref_rows(oracle, iq, N, K)
        _check("cu8 N=%d K=%d f64 rows" % (N, K), engine.spectra_anylen(iq, N, k_avg=K), ref, TOL_F64)
        _check("cu8 N=%d K=%d f32 rows" % (N, K), engine.spectra_anylen(iq, N, k_avg=K, rows_f32=True), ref, TOL_ROWS_F32)
    if N <= ORACLE_MAX_N:
        pay = engine.spectra_anylen(iq, N, k_avg=3, output="payload_u8", gain_db=9)
        for r in range(F // 3):
            assert np.array_equal(pay[r], oracle.spectrum_payload(ref[r], 3, 9)), (N, r)
    Ko = 2 if N != 2047 else 1                                         # the oracle's direct sum: ~1 s per 2047-point frame
    s32 = rng.integers(-4000, 4000, size=(Ko, N, 2), dtype=np.int32)
    f32 = rng.standard_normal((Ko, N)).astype(np.float32)
    _check("cs32 N=%d K=%d" % (N, Ko), engine.spectra_anylen(s32, N, k_avg=Ko, input="cs32"), _ref_rows(oracle, s32, N, Ko, "cs32"), TOL_F64)
    _check("rf32 N=%d K=%d" % (N, Ko), engine.spectra_anylen(f32, N, k_avg=Ko, input="rf32"), _ref_rows(oracle, f32, N, Ko, "rf32"), TOL_F64)
    if N == 8192:
        for K in (1, 3):
            _check("N=8192 K=%d against rtlws_spectra_batch_f64" % K, engine.spectra_anylen(iq, N, k_avg=K),
                   engine.spectra(iq, N, k_avg=K, f64=True), TOL_F64)


def test_the_longest_frame(engine):
    """N = 2^19, the limit: M = 2^20, one frame."""
    from rtlws import synth
    N = 1 << 19
    iq = synth.tone_noise_iq(1, N, seed=19)
    _check("cu8 N=2^19", engine.spectra_anylen(iq, N), anylen_ref.rows(iq, N, 1), TOL_F64)


@pytest.mark.parametrize("N", [1001, 12000])
def test_dc_slot_rule(engine, oracle, N):
    """Slot i0 = N - N//2 shows bin N-1 with the running-sum weights (K - k) of src/spectrum.c:25-33, slot i0 - 1 its
    plain sum, to 1e-13 relative; rows whose three frames differ, so the weights are visible.  Constant frames give
    exact zeros where the reference gives them."""
    from rtlws import synth
    K = 3
    i0 = N - N // 2
    iq = synth.tone_noise_iq(2 * K, N, seed=77)
    ref = _ref_rows(oracle, iq, N, K)
    single = _ref_rows(oracle, iq, N, 1)
    got = engine.spectra_anylen(iq, N, k_avg=K)
    for r in range(2):
        p = single[r * K:(r + 1) * K, i0 - 1]                           # |X[N-1]|^2 of the three frames
        assert len(set(p.tolist())) == K                              # they differ
        want_dc = sum((K - k) * p[k] for k in range(K))
        assert abs(ref[r, i0] - want_dc) <= 1e-12 * want_dc           # the reference follows the closed form
        assert abs(ref[r, i0] - p.sum()) > 1e-3 * p.sum()             # ... which is not the plain sum
        for slot in (i0, i0 - 1):
            rel = abs(got[r, slot] - ref[r, slot]) / ref[r, slot]
            print("N %d row %d slot %d: rel %.3g" % (N, r, slot, rel))
            assert rel <= 1e-13, (r, slot)
    const = np.full((2, N, 2), 128, dtype=np.uint8)                   # (u8 - 128) / 128 = 0: the reference's rows are zero
    zeros = engine.spectra_anylen(const, N, k_avg=2)
    assert zeros.shape == (1, N) and not zeros.any()


def test_epilogues_12000_k6(engine):
    """dB within 1e-9 dB, payload bytes identical (src/cbb_main.c:112,125-128) for gains 0, 15 and -25."""
    from rtlws import synth
    N, K = 12000, 6
    iq = synth.tone_noise_iq(2 * K, N, seed=21)
    ref = anylen_ref.rows(iq, N, K)
    db = engine.spectra_anylen(iq, N, k_avg=K, output="mean_db")
    db32 = engine.spectra_anylen(iq, N, k_avg=K, output="mean_db", rows_f32=True)
    for r in range(2):
        err = np.abs(db[r] - 10 * np.log10(ref[r] / K)).max()
        print("row %d: mean_db max abs err %.3g dB" % (r, err))
        assert err <= 1e-9
        assert np.array_equal(db32[r], db[r].astype(np.float32))      # the same value, rounded once
    for gain in (0, 15, -25):
        pay = engine.spectra_anylen(iq, N, k_avg=K, output="payload_u8", gain_db=gain)
        for r in range(2):
            assert np.array_equal(pay[r], _payload(ref[r], K, gain)), gain


def test_batch_end_without_slack(engine, built, oracle):
    """An odd-N batch whose last frame ends where the samples end and whose last row ends where the rows end: the
    n >= N guard of pass 1 and the j >= N guard of pass 4.  Once in exactly-sized device buffers, once inside larger
    ones whose bytes around the frames are poison (255, 255 = +0.992 +0.992i if read as a sample) and around the rows
    a marker that must survive; the frames start on an odd 2-byte boundary there."""
    from rtlws import synth
    N, F, G = 1001, 3, 1024
    iq = synth.tone_noise_iq(F, N, seed=31)
    ref = oracle.batch_spectra_u8(iq, N, nthreads=8)
    tight = engine.spectra_anylen(iq, N)                                # upload(iq), alloc(F * N * 8): no slack asked for
    _check("odd N, exactly-sized buffers", tight, ref, TOL_F64)
    raw = np.full(G + 2 + F * N * 2 + G, 255, dtype=np.uint8)
    raw[G + 2:G + 2 + F * N * 2] = iq.reshape(-1)
    d_in = engine.upload(raw)
    d_out = engine.upload(np.full(G + F * N + G, -7.0))
    plan = built.AnyLenPlan(engine, built.make_desc(N), max_frames=F)
    plan.run(d_in.ptr + G + 2, F, d_out.ptr + 8 * G)
    o = engine.download(d_out, np.float64, (G + F * N + G,))
    plan.close()
    d_in.free()
    d_out.free()
    assert (o[:G] == -7.0).all() and (o[G + F * N:] == -7.0).all()       # nothing written outside the rows
    assert np.array_equal(o[G:G + F * N].reshape(F, N), tight)           # nothing read outside the frames


def test_grouping_and_arguments(engine, built):
    """A plan opened with max_frames = 1 runs a batch of several rows bit-identically to one opened for the whole
    batch; the workspace rule; the argument checks of rtlws_anylen_run."""
    from rtlws import synth
    N, K, F = 12001, 2, 8
    M = 1 << 15
    iq = synth.tone_noise_iq(F, N, seed=5)
    whole = engine.spectra_anylen(iq, N, k_avg=K)
    grouped = engine.spectra_anylen(iq, N, k_avg=K, max_frames=1)
    assert np.array_equal(whole, grouped)
    _check("grouped batch", grouped, anylen_ref.rows(iq, N, K), TOL_F64)

    plan = built.AnyLenPlan(engine, built.make_desc(N, k_avg=K), max_frames=1)
    assert plan.workspace_bytes == K * 2 * 16 * M                       # one row's frames in both workspaces
    d_in = engine.upload(iq)
    d_out = engine.alloc((F // K) * N * 8)
    assert plan.run(d_in, 0, d_out, check=False) == 0
    assert plan.run(d_in, 3, d_out, check=False) == -1 and "multiple of k_avg" in built.anylen_last_error()
    assert plan.run(d_in, K, d_out.ptr + 4, check=False) == -1 and "aligned" in built.anylen_last_error()
    assert plan.run(d_in.ptr + 1, K, d_out, check=False) == -1 and "aligned" in built.anylen_last_error()
    assert plan.run(None, K, d_out, check=False) == -1 and "null pointer" in built.anylen_last_error()
    assert plan.run(d_in, K, None, check=False) == -1 and "null pointer" in built.anylen_last_error()
    assert plan.run(d_in, -2, d_out, check=False) == -1
    plan.close()
    # a plan asked for more than the cap holds keeps whole rows within it
    big = built.AnyLenPlan(engine, built.make_desc(1 << 19, k_avg=3), max_frames=1000)
    assert big.workspace_bytes == 30 * (32 << 20)                      # 10 rows of 3 frames, 32 MiB each <= 1 GiB
    big.close()
    for bad in (built.make_desc(N, window="hann"), built.make_desc(N, cic_r=8), built.make_desc(1),
                built.make_desc((1 << 19) + 1), built.make_desc(N, k_avg=0)):
        with pytest.raises(RuntimeError):
            built.AnyLenPlan(engine, bad)
    d_in.free()
    d_out.free()


def test_capture_and_replay_anylen(built):
    """One rtlws_anylen_run after rtlws_anylen_open, captured on a single stream (a linear chain of four kernels) and
    replayed, equals the eager result bit for bit: open has done the tables, the chirp's transform, the workspaces
    and the LDS opt-in."""
    import torch
    from rtlws import synth
    dev = torch.device("cuda", 0)
    eng = built.Engine(0)
    N, F = 12000, 4
    iq_host = synth.tone_noise_iq(F, N, seed=19)
    iq = torch.from_numpy(iq_host).to(dev)
    out = torch.zeros((F, N), dtype=torch.float64, device=dev)
    plan = built.AnyLenPlan(eng, built.make_desc(N), max_frames=F)
    g = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        with torch.cuda.graph(g, stream=side):
            plan.run(iq.data_ptr(), F, out.data_ptr(), stream=built.torch_stream_handle())
    torch.cuda.current_stream().wait_stream(side)
    assert float(out.abs().sum()) == 0.0            # capture enqueued nothing
    g.replay()
    torch.cuda.synchronize()
    first = out.clone()
    out.zero_()
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, first)
    eager = torch.zeros((F, N), dtype=torch.float64, device=dev)
    plan.run(iq.data_ptr(), F, eager.data_ptr(), stream=built.torch_stream_handle())
    torch.cuda.synchronize()
    assert torch.equal(eager, out)
    _check("captured run", out.cpu().numpy(), anylen_ref.rows(iq_host, N, 1), TOL_F64)
    plan.close()
    eng.close()


def test_dropin_opt_in(built, monkeypatch):
    """spectrum.h at N = 12000 in a process that sets RTLWS_ANY_LENGTH: the three spectrum_add_* accumulate into a
    NON-ZERO buffer like the reference (src/spectrum.c:25-33); len != N returns -1 and leaves the buffer alone.
    Without the variable the size is refused as before."""
    from rtlws import synth
    N = 12000
    i0 = N - N // 2
    monkeypatch.delenv("RTLWS_ANY_LENGTH", raising=False)
    assert built.amd_lib().spectrum_alloc(N) is None
    monkeypatch.setenv("RTLWS_ANY_LENGTH", "0")
    assert built.amd_lib().spectrum_alloc(N) is None
    monkeypatch.setenv("RTLWS_ANY_LENGTH", "1")
    rng = np.random.default_rng(12)
    s = built.Spectrum(N)
    iq = synth.tone_noise_iq(2, N, seed=3)
    s32 = rng.integers(-4000, 4000, size=(N, 2), dtype=np.int32)
    f32 = rng.standard_normal(N).astype(np.float32)
    ps = rng.uniform(1.0, 2.0, size=N)
    ref = ps.copy()
    before = ps.copy()

    def ref_add(frame, input):
        """src/spectrum.c:25-33 with the frame's powers from np.fft.fft"""
        p = anylen_ref.rows(frame[None], N, 1, input)[0]
        for i in range(N):
            ref[i] += p[i] if i != i0 else ref[i - 1]

    assert s.add_cmplx_u8(iq[0], ps, length=N - 1) == -1 and np.array_equal(ps, before)
    assert s.add_cmplx_u8(iq[0], ps) == 0
    ref_add(iq[0], "cu8")
    assert s.add_cmplx_u8(iq[1], ps) == 0
    ref_add(iq[1], "cu8")
    _check("drop-in cmplx_u8 N=%d" % N, ps, ref, TOL_F64)
    assert s.add_cmplx_s32(s32, ps) == 0
    ref_add(s32, "cs32")
    _check("drop-in cmplx_s32 N=%d" % N, ps, ref, TOL_F64)
    assert s.add_real_f32(f32, ps) == 0
    ref_add(f32, "rf32")
    _check("drop-in real_f32 N=%d" % N, ps, ref, TOL_F64)
    s.free()
    assert built.amd_lib().spectrum_alloc((1 << 19) + 1) is None       # above the limit: refused with the variable set, too
    monkeypatch.delenv("RTLWS_ANY_LENGTH")
    assert built.amd_lib().spectrum_alloc(N) is None                   # not opted in: refused as before

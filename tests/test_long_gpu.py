"""GPU suite of include/rtlws_long.h: f64 power spectra of 2^14 .. 2^20-point frames (the four-step transform of
rtl-ws_amd/csrc/spectrum_long.hip) against the f64 oracle, under the strict metric of the f64 batch tests
(helpers.rel_err with EPS_STRICT: 1e-10 over a floor of 1e-9 of the row maximum; f32 rows 6.0e-8 as in smoke())."""
import numpy as np
import pytest

from helpers import rel_err, EPS_STRICT, TOL_F64

pytestmark = pytest.mark.gpu

TOL_ROWS_F32 = 6.0e-8


def _oracle_rows(oracle, add, frames, N, K):
    """K sequential oracle.spectrum_add_* calls per row into a zeroed buffer."""
    rows = np.zeros((len(frames) // K, N))
    for f, frame in enumerate(frames):
        assert add(N, frame, rows[f // K]) == 0
    return rows


def _check(what, got, ref, tol):
    e = rel_err(got, ref, EPS_STRICT).max()
    print("%s: max strict rel err %.3g (bound %.1e)" % (what, e, tol))
    assert e <= tol, what


@pytest.mark.parametrize("m", range(14, 21))
def test_batch_parity(engine, oracle, m):
    """Every size (both parities of m, both extreme splits), K = 1 and 3, the three inputs, f64 and f32 rows, and
    the payload bytes: every kernel of the library is launched here (tests/long_kernels.py)."""
    from rtlws import synth
    N = 1 << m
    F = 6 if m <= 17 else 3
    rng = np.random.default_rng(100 + m)
    iq = synth.tone_noise_iq(F, N, seed=40 + m)
    for K in (1, 3):
        ref = oracle.batch_spectra_u8(iq, N, K=K, nthreads=8)
        _check("cu8 tone+noise N=2^%d K=%d f64 rows" % (m, K), engine.spectra_long(iq, N, k_avg=K), ref, TOL_F64)
        _check("cu8 tone+noise N=2^%d K=%d f32 rows" % (m, K), engine.spectra_long(iq, N, k_avg=K, rows_f32=True), ref,
               TOL_ROWS_F32)
    pay = engine.spectra_long(iq, N, k_avg=3, output="payload_u8", gain_db=9)
    for r in range(F // 3):
        assert np.array_equal(pay[r], oracle.spectrum_payload(ref[r], 3, 9)), (m, r)
    uq = synth.uniform_iq(F, N, seed=60 + m)
    for K in (1, 3):
        ref = oracle.batch_spectra_u8(uq, N, K=K, nthreads=8)
        _check("cu8 uniform N=2^%d K=%d f64 rows" % (m, K), engine.spectra_long(uq, N, k_avg=K), ref, TOL_F64)
    s32 = rng.integers(-4000, 4000, size=(3, N, 2), dtype=np.int32)
    f32 = rng.standard_normal((3, N)).astype(np.float32)
    for K in (1, 3):
        ref = _oracle_rows(oracle, oracle.spectrum_add_cmplx_s32, s32, N, K)
        _check("cs32 N=2^%d K=%d f64 rows" % (m, K), engine.spectra_long(s32, N, k_avg=K, input="cs32"), ref, TOL_F64)
        _check("cs32 N=2^%d K=%d f32 rows" % (m, K), engine.spectra_long(s32, N, k_avg=K, input="cs32", rows_f32=True),
               ref, TOL_ROWS_F32)
        ref = _oracle_rows(oracle, oracle.spectrum_add_real_f32, f32, N, K)
        _check("rf32 N=2^%d K=%d f64 rows" % (m, K), engine.spectra_long(f32, N, k_avg=K, input="rf32"), ref, TOL_F64)


def test_constant_frame_gives_exact_zeros(engine):
    for m in (14, 17, 20):
        N = 1 << m
        iq = np.full((2, N, 2), 128, dtype=np.uint8)
        got = engine.spectra_long(iq, N, k_avg=2)
        assert got.shape == (1, N) and not got.any(), m


def test_dc_slot_rule_at_65536(engine, oracle):
    """Slot N/2 shows bin N-1 with the running-sum weights (K - k) of src/spectrum.c:25-33, slot N/2 - 1 its plain
    sum: rows whose three frames differ, so the weights are visible."""
    from rtlws import synth
    N, K = 65536, 3
    iq = synth.tone_noise_iq(2 * K, N, seed=77)
    ref = oracle.batch_spectra_u8(iq, N, K=K, nthreads=8)
    single = oracle.batch_spectra_u8(iq, N, K=1, nthreads=8)
    got = engine.spectra_long(iq, N, k_avg=K)
    for r in range(2):
        p = single[r * K:(r + 1) * K, N // 2 - 1]                       # |X[N-1]|^2 of the three frames
        assert len(set(p.tolist())) == K                              # they differ
        want_dc = sum((K - k) * p[k] for k in range(K))
        assert abs(ref[r, N // 2] - want_dc) <= 1e-12 * want_dc       # the oracle follows the closed form
        assert abs(ref[r, N // 2] - p.sum()) > 1e-3 * p.sum()         # ... which is not the plain sum
        for slot in (N // 2, N // 2 - 1):
            rel = abs(got[r, slot] - ref[r, slot]) / ref[r, slot]
            print("row %d slot %d: rel %.3g" % (r, slot, rel))
            assert rel <= 1e-12, (r, slot)


def test_epilogues_16384_k6(engine, oracle):
    """dB to 1e-11 dB, payload bytes IDENTICAL (src/cbb_main.c:112,125-128), for the gains
    test_f64_inputs_window_cic_and_epilogues uses."""
    from rtlws import synth
    N, K = 16384, 6
    iq = synth.tone_noise_iq(2 * K, N, seed=21)
    ref = oracle.batch_spectra_u8(iq, N, K=K, nthreads=8)
    db = engine.spectra_long(iq, N, k_avg=K, output="mean_db")
    db32 = engine.spectra_long(iq, N, k_avg=K, output="mean_db", rows_f32=True)
    for r in range(2):
        want = oracle.mean_db(ref[r], K)
        err = np.abs(db[r] - want).max()
        print("row %d: mean_db max abs err %.3g dB" % (r, err))
        assert err <= 1e-11
        assert np.array_equal(db32[r], db[r].astype(np.float32))      # the same value, rounded once
    for gain in (0, 15, -25, 9, -9, 100):
        pay = engine.spectra_long(iq, N, k_avg=K, output="payload_u8", gain_db=gain)
        for r in range(2):
            assert np.array_equal(pay[r], oracle.spectrum_payload(ref[r], K, gain)), gain


def test_grouping_and_arguments(engine, built, oracle):
    """A batch larger than the plan's frames in flight runs as consecutive groups: the same bytes as the same
    frames run one row per call, and as a second run.  Argument checks of rtlws_long_run."""
    from rtlws import synth
    N, K, F = 16384, 2, 12
    iq = synth.tone_noise_iq(F, N, seed=5)
    desc = built.make_desc(N, k_avg=K)
    plan = built.LongPlan(engine, desc, max_frames=4)
    assert plan.workspace_bytes == 4 * 16 * N                          # two rows in flight: six groups' worth of frames
    d_in = engine.upload(iq)
    d_out = engine.alloc((F // K) * N * 8)
    plan.run(d_in, F, d_out)
    whole = engine.download(d_out, np.float64, (F // K, N))
    engine._chk(built.hip_lib().rtlws_memset_dev(engine.h, d_out.ptr, 0, d_out.nbytes, None), "memset")
    plan.run(d_in, F, d_out)
    again = engine.download(d_out, np.float64, (F // K, N))
    assert np.array_equal(whole, again)                                # deterministic
    engine._chk(built.hip_lib().rtlws_memset_dev(engine.h, d_out.ptr, 0, d_out.nbytes, None), "memset")
    for r in range(F // K):
        plan.run(d_in.ptr + r * K * N * 2, K, d_out.ptr + r * N * 8)
    by_row = engine.download(d_out, np.float64, (F // K, N))
    assert np.array_equal(whole, by_row)
    _check("grouped batch", whole, oracle.batch_spectra_u8(iq, N, K=K, nthreads=8), TOL_F64)

    assert plan.run(d_in, 0, d_out, check=False) == 0
    assert plan.run(d_in, 3, d_out, check=False) == -1 and "multiple of k_avg" in built.long_last_error()
    assert plan.run(d_in, K, d_out.ptr + 4, check=False) == -1 and "aligned" in built.long_last_error()
    assert plan.run(None, K, d_out, check=False) == -1
    assert plan.run(d_in, -2, d_out, check=False) == -1
    plan.close()
    # a plan asked for more than the cap holds keeps whole rows within it
    big = built.LongPlan(engine, built.make_desc(1 << 20, k_avg=3), max_frames=1000)
    assert big.workspace_bytes == 63 * (16 << 20)                      # 21 rows of 3 frames <= 1 GiB
    big.close()
    for bad in (built.make_desc(N, window="hann"), built.make_desc(N, cic_r=8), built.make_desc(12000),
                built.make_desc(8192), built.make_desc(1 << 21), built.make_desc(N, k_avg=0)):
        with pytest.raises(RuntimeError):
            built.LongPlan(engine, bad)
    d_in.free()
    d_out.free()


@pytest.mark.parametrize("N", [16384, 1 << 20])
def test_dropin_long_frames(built, oracle, N):
    """spectrum.h at sizes above 8192: the three spectrum_add_* accumulate into a NON-ZERO buffer like the
    reference (src/spectrum.c:25-33); len != N returns -1 and leaves the buffer alone."""
    from rtlws import synth
    rng = np.random.default_rng(N % 1000)
    s = built.Spectrum(N)
    iq = synth.tone_noise_iq(2, N, seed=3)
    s32 = rng.integers(-4000, 4000, size=(N, 2), dtype=np.int32)
    f32 = rng.standard_normal(N).astype(np.float32)
    ps = rng.uniform(1.0, 2.0, size=N)
    ref = ps.copy()
    before = ps.copy()
    assert s.add_cmplx_u8(iq[0], ps, length=N - 1) == -1 and np.array_equal(ps, before)
    assert s.add_cmplx_u8(iq[0], ps) == 0 and oracle.spectrum_add_cmplx_u8(N, iq[0], ref) == 0
    assert s.add_cmplx_u8(iq[1], ps) == 0 and oracle.spectrum_add_cmplx_u8(N, iq[1], ref) == 0
    _check("drop-in cmplx_u8 N=%d" % N, ps, ref, TOL_F64)
    assert s.add_cmplx_s32(s32, ps) == 0 and oracle.spectrum_add_cmplx_s32(N, s32, ref) == 0
    _check("drop-in cmplx_s32 N=%d" % N, ps, ref, TOL_F64)
    assert s.add_real_f32(f32, ps) == 0 and oracle.spectrum_add_real_f32(N, f32, ref) == 0
    _check("drop-in real_f32 N=%d" % N, ps, ref, TOL_F64)
    s.free()
    assert built.amd_lib().spectrum_alloc(12000) is None               # not a power of two: refused as before
    assert built.amd_lib().spectrum_alloc(1 << 21) is None


def test_capture_and_replay_long(built, oracle):
    """One rtlws_long_run after rtlws_long_open, captured on a single stream (a linear chain: pass A, pass B) and
    replayed, equals the eager result: open has done the tables, the workspace and the LDS opt-in."""
    import torch
    from rtlws import synth
    dev = torch.device("cuda", 0)
    eng = built.Engine(0)
    N, F = 16384, 8
    iq_host = synth.tone_noise_iq(F, N, seed=19)
    iq = torch.from_numpy(iq_host).to(dev)
    out = torch.zeros((F, N), dtype=torch.float64, device=dev)
    plan = built.LongPlan(eng, built.make_desc(N), max_frames=F)
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
    _check("captured run", out.cpu().numpy(), oracle.batch_spectra_u8(iq_host, N, nthreads=8), TOL_F64)
    plan.close()
    eng.close()

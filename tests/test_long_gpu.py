"""GPU suite of include/rtlws_long.h: f64 power spectra of 2^14 .. 2^20-point frames (the four-step transform of
rtl-ws_amd/csrc/spectrum_long.hip) against the f64 oracle, under the strict metric of the f64 batch tests
(helpers.rel_err with EPS_STRICT: 1e-10 over a floor of 1e-9 of the row maximum; f32 rows 6.0e-8 as in smoke()).
The first tests launch every kernel instantiation (tests/long_kernels.py); those from
test_accuracy_against_long_double on hold the rows to a long-double FFT under a whole-row metric two to four orders
tighter, and walk every pass length, sample size, row kind and group border (tests/long_border_cases.py), bit for bit
where that can be asked."""
import numpy as np
import pytest

import long_border_cases as bc
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


# ---- every pass length, kind and group border (tests/long_border_cases.py) ----------------------------------------

def _bits(a):
    """an array's bytes as unsigned integers of its item size: equality of these is equality bit for bit"""
    a = np.ascontiguousarray(a)
    return a.view({1: np.uint8, 4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def _oracle_any(oracle, data, N, K, input):
    if input == "cu8":
        return oracle.batch_spectra_u8(data, N, K=K, nthreads=8)
    return _oracle_rows(oracle, oracle.spectrum_add_cmplx_s32 if input == "cs32" else oracle.spectrum_add_real_f32,
                        data, N, K)


def _rows_kw(rows, gain):
    return dict(rows_f32=True) if rows == "f32" else dict(output="payload_u8", gain_db=gain) if rows == "u8" else {}


def _check_kind(oracle, what, got, ref, K, rows, gain):
    """rows of one kind against the oracle's f64 rows: TOL_F64, TOL_ROWS_F32, or the exact bytes"""
    assert got.dtype == bc.ROW_DTYPE[rows] and got.shape == ref.shape, what
    if rows == "u8":
        for r in range(len(ref)):
            assert np.array_equal(got[r], oracle.spectrum_payload(ref[r], K, gain)), (what, r)
    else:
        _check(what, got, ref, TOL_F64 if rows == "f64" else TOL_ROWS_F32)


@pytest.mark.parametrize("m", bc.ACCURACY_M)
def test_accuracy_against_long_double(engine, oracle, m):
    """e(row) = rms(row - truth) / mean(truth) against numpy's long-double FFT, one frame per input at K = 1:
    e(kernel) <= 2 max(e(oracle), e(test_long_cpu.four_step)).  The two CPU transforms lie within 1.07 of each other
    on these frames (tests/test_long_borders_cpu.py asserts 1.5), the restatement carries the two-table twiddle's
    extra rounding already, and 2x leaves room for the radix-16 FMA butterflies' other rounding pattern.  The strict
    per-bin metric with its bound 1e-10 passes a twiddle table whose phases are off by 1e-13; this one fails from an rms
    phase error of about 1.4e-15 on (twl's angles times 1 + 1e-13 fail m = 14 .. 18, times 1 + 1e-12 every m).
    Measured on one MI355X: the kernels at 0.93 .. 1.05 of the larger CPU figure (profiles/long_accuracy.txt)."""
    assert np.finfo(np.longdouble).eps <= 2.0 ** -63                    # the truth is wider than what it judges
    N = 1 << m
    frames = bc.accuracy_frames(m)
    worst = 0.0
    for input in bc.INPUTS:
        truth = bc.truth_rows(frames[input], input)[0]
        e_oracle = bc.e_metric(_oracle_any(oracle, frames[input], N, 1, input)[0], truth)
        e_four = bc.e_metric(bc.four_step_rows(frames[input], input)[0], truth)
        got = engine.spectra_long(frames[input], N, input=input)
        assert got.shape == (1, N) and got.dtype == np.float64
        e_kernel = bc.e_metric(got[0], truth)
        bound = 2 * max(e_oracle, e_four)
        print("accuracy m=%d %s: e kernel %.3g, oracle %.3g, four_step %.3g; kernel / max(oracle, four_step) %.3f (bound 2)"
              % (m, input, e_kernel, e_oracle, e_four, 2 * e_kernel / bound))
        worst = max(worst, e_kernel / bound)
    assert worst <= 1.0, m


@pytest.mark.parametrize("m", bc.STORES_M)
def test_one_value_three_stores(engine, oracle, m):
    """store_value at every pass B length: the f32 rows are the launch's own f64 rows rounded once, power and dB;
    the dB rows are within 1e-11 dB of the oracle's mean_db of the launch's own power row, and the payload bytes are
    the oracle's spectrum_payload of that row -- a payload one ulp of the power away from the f64 row shows, which
    against the oracle's rows it could not."""
    from rtlws import synth
    N = 1 << m
    gain = bc.STORES_GAIN[m]
    iq = synth.tone_noise_iq(3, N, seed=50 + m)
    for K in (3, 1):
        p = engine.spectra_long(iq, N, k_avg=K)
        assert p.shape == (3 // K, N) and np.isfinite(p).all() and p.min() > 0
        assert np.array_equal(_bits(engine.spectra_long(iq, N, k_avg=K, rows_f32=True)), _bits(p.astype(np.float32))), K
        db = engine.spectra_long(iq, N, k_avg=K, output="mean_db")
        assert np.array_equal(_bits(engine.spectra_long(iq, N, k_avg=K, output="mean_db", rows_f32=True)),
                              _bits(db.astype(np.float32))), K
        pay = engine.spectra_long(iq, N, k_avg=K, output="payload_u8", gain_db=gain)
        assert pay.dtype == np.uint8 and pay.shape == p.shape
        for r in range(3 // K):
            err = np.abs(db[r] - oracle.mean_db(p[r], K)).max()
            print("m=%d K=%d row %d: mean_db of the launch's own row, max abs err %.3g dB" % (m, K, r, err))
            assert err <= 1e-11
            assert np.array_equal(pay[r], oracle.spectrum_payload(p[r], K, gain)), (K, r)
        assert len(np.unique(pay)) > 2                                  # the gain leaves the bytes something to say
    if m == bc.SATURATION_M:
        # a cmplx_s32 tone of amplitude 2^30 on bin 1000 over +-2^20 of noise: its bin passes 255 dB at gain +40
        rng = np.random.default_rng(m)
        ph = 2 * np.pi * 1000 * np.arange(N) / N
        s32 = rng.integers(-(1 << 20), (1 << 20) + 1, size=(1, N, 2), dtype=np.int64)
        s32[0, :, 0] += np.rint(2.0 ** 30 * np.cos(ph)).astype(np.int64)
        s32[0, :, 1] += np.rint(2.0 ** 30 * np.sin(ph)).astype(np.int64)
        s32 = s32.astype(np.int32)
        p = engine.spectra_long(s32, N, input="cs32")
        pay = engine.spectra_long(s32, N, input="cs32", output="payload_u8", gain_db=bc.SATURATION_GAIN)
        assert np.array_equal(pay[0], oracle.spectrum_payload(p[0], 1, bc.SATURATION_GAIN))
        assert pay[0, (1000 + N // 2) % N] == 255 and 0 < (pay == 255).sum() < 16 and pay.min() < 200


@pytest.mark.parametrize("m", bc.K_SUMS_M)
def test_k_sums_are_the_k1_rows_added_in_order(engine, m):
    """K is a launch argument of one instantiation of long_pass_b: the K = 3 run computes the same pw per frame and
    adds them in frame order to an accumulator that starts at zero, so outside the DC slot its row is (p0 + p1) + p2
    of the K = 1 rows of the same frames bit for bit.  In a K = 1 row the DC slot carries 0 + 1 * pw of bin N - 1: its
    neighbour's value, bit for bit."""
    from rtlws import synth
    N = 1 << m
    iq = synth.tone_noise_iq(3, N, seed=70 + m)
    p = engine.spectra_long(iq, N, k_avg=1)
    s = engine.spectra_long(iq, N, k_avg=3)
    assert p.shape == (3, N) and s.shape == (1, N)
    want = (p[0] + p[1]) + p[2]
    keep = np.arange(N) != N // 2
    assert np.array_equal(_bits(s[0][keep]), _bits(want[keep]))
    assert np.array_equal(_bits(p[:, N // 2]), _bits(p[:, N // 2 - 1]))
    assert len(set(p[:, N // 2].tolist())) == 3                        # the frames differ


@pytest.mark.parametrize("m", bc.SCALING_M)
def test_power_of_two_scaling_is_exact(engine, oracle, m):
    """Frames times a power of two give rows times its square, bit for bit: such a scaling commutes with every
    rounding while nothing overflows or goes subnormal (the numpy restatement has the property exactly,
    tests/test_long_borders_cpu.py), so any path that depends on the input's size, any constant that is not a factor,
    and any workspace element read without having been written shows."""
    N = 1 << m
    rng = np.random.default_rng(m + 1)
    f32 = rng.standard_normal((4, N)).astype(np.float32)
    base = engine.spectra_long(f32, N, k_avg=2, input="rf32")
    assert base.shape == (2, N) and np.isfinite(base).all() and base.min() > 0
    for e in (40, -40):
        scaled = f32 * np.float32(2.0 ** e)
        assert np.array_equal(scaled.astype(np.float64), f32.astype(np.float64) * 2.0 ** e)      # the frames scale exactly
        got = engine.spectra_long(scaled, N, k_avg=2, input="rf32")
        assert np.array_equal(_bits(got), _bits(base * 2.0 ** (2 * e))), e
    s32 = rng.integers(-(1 << 20), (1 << 20) + 1, size=(4, N, 2), dtype=np.int32)
    base = engine.spectra_long(s32, N, k_avg=2, input="cs32")
    got = engine.spectra_long(s32 << 8, N, k_avg=2, input="cs32")
    assert np.array_equal(_bits(got), _bits(base * 2.0 ** 16))
    _check("cs32 N=2^%d within 2^20" % m, base, _oracle_any(oracle, s32, N, 2, "cs32"), TOL_F64)


def test_input_extremes(engine, oracle):
    """The conversion at T = 64 and T = 8 columns of pass A.  One cmplx_s32 frame drawn over all of int32, INT32_MIN and
    INT32_MAX at its first and last sample: no narrower type (24 bits of f32) on its way.  One real_f32 frame of Gaussian
    samples that holds the largest finite f32, the smallest subnormal and -0.0."""
    lo, hi = -(1 << 31), (1 << 31) - 1
    for m in bc.EXTREMES_M:
        N = 1 << m
        rng = np.random.default_rng(m + 2)
        s32 = rng.integers(lo, hi + 1, size=(1, N, 2), dtype=np.int64).astype(np.int32)
        s32[0, 0] = (lo, hi)
        s32[0, N - 1] = (hi, lo)
        _check("cs32 N=2^%d over all of int32" % m, engine.spectra_long(s32, N, input="cs32"),
               _oracle_any(oracle, s32, N, 1, "cs32"), TOL_F64)
        f32 = rng.standard_normal((1, N)).astype(np.float32)
        f32[0, 5] = np.finfo(np.float32).max
        f32[0, N // 3] = np.float32(2.0 ** -149)
        f32[0, N - 7] = np.float32(-0.0)
        assert f32[0, N // 3] > 0 and np.signbit(f32[0, N - 7])
        got = engine.spectra_long(f32, N, input="rf32")
        assert np.isfinite(got).all()
        _check("rf32 N=2^%d with the extremes of f32" % m, got, _oracle_any(oracle, f32, N, 1, "rf32"), TOL_F64)


def test_a_frame_stays_in_its_row(engine):
    """Three real_f32 frames at K = 1, the middle one all NaN: its row is NaN in every slot and the other two rows are,
    bit for bit, those of the two frames run without it -- through a pass A grid that xcd_chunked leaves alone (6
    workgroups at 2^14) and one it permutes (24 at 2^16; the run of two frames has 16)."""
    for m in bc.OWN_ROW_M:
        N = 1 << m
        f32 = np.random.default_rng(m + 3).standard_normal((3, N)).astype(np.float32)
        clean = engine.spectra_long(f32[[0, 2]], N, input="rf32")
        assert np.isfinite(clean).all()
        f32[1] = np.nan
        got = engine.spectra_long(f32, N, input="rf32")
        assert got.shape == (3, N)
        assert np.array_equal(_bits(got[[0, 2]]), _bits(clean)), m
        assert np.isnan(got[1]).all(), m


@pytest.mark.parametrize("m,F", bc.PLACE_CASES)
def test_frame_place_does_not_matter(engine, oracle, m, F):
    """One frame at places 0, 1 and F - 1 of a batch of otherwise different frames gives the same row, bit for bit.
    Pass A deals its grid (F N / 8192 workgroups) through xcd_chunked: the identity at 3 and 5 frames of 2^14 points (6
    and 10 workgroups), a permutation that sends a frame's tiles to different chunks at 4 frames of 2^15 (16) and at 2
    frames of 2^20 (256)."""
    from rtlws import synth
    N = 1 << m
    assert (bc.pass_a_grid(m, F) % 8 == 0) == (m != 14)
    iq = synth.uniform_iq(F + 1, N, seed=90 + m)
    other, iq = iq[F], iq[:F].copy()
    places = sorted({0, 1, F - 1})
    for i in places[1:]:
        iq[i] = iq[0]
    got = engine.spectra_long(iq, N)
    for i in places[1:]:
        assert np.array_equal(_bits(got[i]), _bits(got[0])), i
    _check("N=2^%d, %d frames" % (m, F), got, oracle.batch_spectra_u8(iq, N, nthreads=8), TOL_F64)
    rest = [i for i in range(F) if i not in places]
    if rest:
        assert not np.array_equal(got[rest[0]], got[0])
    else:                                                              # every place holds the frame: another in front of it
        iq[0] = other
        moved = engine.spectra_long(iq, N)
        assert np.array_equal(_bits(moved[F - 1]), _bits(got[0])) and not np.array_equal(moved[0], got[0])


def _run_plan(engine, built, data, N, K, input, rows, max_frames, gain, guard=0, skew=0, poison=255, marker=None):
    """One rtlws_long_run through a plan of max_frames: (rows, workspace bytes).  With a guard the frames lie
    guard + skew bytes into a buffer of poison bytes and end where `guard` more begin, and the rows between `guard`
    marker items on either side, which are returned as well."""
    data = np.ascontiguousarray(data)
    F = data.nbytes // (bc.SAMPLE_BYTES[input] * N)
    dtype = bc.ROW_DTYPE[rows]
    item = bc.ROW_BYTES[rows]
    desc = built.make_desc(N, k_avg=K, input=input, output="payload_u8" if rows == "u8" else "power_sum",
                           gain_db=gain if rows == "u8" else 0, flags=built.FLAG_ROWS_F32 if rows == "f32" else 0)
    raw = np.full(guard + skew + data.nbytes + guard, poison, dtype=np.uint8)
    raw[guard + skew:guard + skew + data.nbytes] = data.reshape(-1).view(np.uint8)
    n_out = (F // K) * N
    plan = built.LongPlan(engine, desc, max_frames=max_frames)
    d_in = engine.upload(raw)
    d_out = engine.upload(np.full(guard + n_out + guard, 0 if marker is None else marker, dtype=dtype))
    try:
        ws = plan.workspace_bytes
        plan.run(d_in.ptr + guard + skew, F, d_out.ptr + item * guard)
        o = engine.download(d_out, dtype, (guard + n_out + guard,))
    finally:
        plan.close()
        d_in.free()
        d_out.free()
    got = o[guard:guard + n_out].reshape(F // K, N)
    return (got, ws) if not guard else (got, ws, o[:guard], o[guard + n_out:])


def test_groups_at_every_sample_and_row_size(engine, built, oracle):
    """rtlws_long_run advances the frames by done * in_bytes and the rows by done / k_avg * row_bytes per group: every
    sample size (2, 8, 4 bytes) under two row sizes and every row size (8, 4, 1) under two sample sizes, ten frames of
    K = 2 as one group, as 4, 4, 2 (a shorter last group), from a max_frames of 3 that the plan rounds up to whole
    rows, and as five groups of one row -- the same bytes every time, and the workspace 16 N bytes per frame in flight."""
    from rtlws import synth
    N, K, F, gain = 1 << bc.GROUP_M, bc.GROUP_K, bc.GROUP_FRAMES, bc.GROUP_GAIN
    rng = np.random.default_rng(N + 1)
    data = {"cu8": synth.tone_noise_iq(F, N, seed=6), "cs32": rng.integers(-(1 << 20), (1 << 20) + 1, size=(F, N, 2), dtype=np.int32),
            "rf32": rng.standard_normal((F, N)).astype(np.float32)}
    ref = {input: _oracle_any(oracle, data[input], N, K, input) for input in bc.INPUTS}
    assert bc.GROUP_MAX_FRAMES[0] == F
    differ = []
    for input, rows in bc.GROUP_KINDS:
        whole = None
        for max_frames in bc.GROUP_MAX_FRAMES:
            got, ws = _run_plan(engine, built, data[input], N, K, input, rows, max_frames, gain)
            assert ws == 16 * N * bc.frames_in_flight(N, K, max_frames), (input, rows, max_frames)
            if whole is None:
                whole = got
                _check_kind(oracle, "%s, %s rows, one group" % (input, rows), whole, ref[input], K, rows, gain)
                assert len(np.unique(whole[-1])) > 2
            elif not np.array_equal(_bits(got), _bits(whole)):
                first = int(np.flatnonzero(_bits(got).ravel() != _bits(whole).ravel())[0])
                differ.append((input, rows, max_frames))
                print("%s, %s rows, max_frames %d (groups %s): differs from the one-group run first at row %d slot %d"
                      % ((input, rows, max_frames, bc.group_plan(F, N, K, max_frames)) + divmod(first, N)))
    assert not differ, differ                                          # every case is run, so that all that differ are named


@pytest.mark.parametrize("m,input,rows", bc.OUTSIDE_CASES)
def test_nothing_outside_frames_and_rows(engine, built, oracle, m, input, rows):
    """Three frames that begin 8 bytes past a 16-byte boundary (rtlws_long_run's minimum alignment) behind 1032 bytes of
    poison and end where 1024 more begin (bytes 255: a NaN as real_f32, full scale as cmplx_u8; bytes 127: about
    2^31 / 128 as cmplx_s32); the rows lie between 1024 marker items that must survive, and are bit for bit those of a
    run on exactly-sized buffers."""
    N, F, gain = 1 << m, bc.OUTSIDE_FRAMES, bc.OUTSIDE_GAIN
    rng = np.random.default_rng(m + 4)
    if input == "cu8":
        from rtlws import synth
        data = synth.tone_noise_iq(F, N, seed=30 + m)
    elif input == "cs32":
        data = rng.integers(-(1 << 20), (1 << 20) + 1, size=(F, N, 2), dtype=np.int32)
    else:
        data = rng.standard_normal((F, N)).astype(np.float32)
    tight = engine.spectra_long(data, N, input=input, **_rows_kw(rows, gain))           # exactly-sized buffers
    _check_kind(oracle, "%s N=2^%d %s rows, exactly-sized buffers" % (input, m, rows), tight,
                _oracle_any(oracle, data, N, 1, input), 1, rows, gain)
    marker = np.uint8(0xA5) if rows == "u8" else bc.ROW_DTYPE[rows](-7.0)
    got, _, front, back = _run_plan(engine, built, data, N, 1, input, rows, F, gain, guard=bc.OUTSIDE_GUARD,
                                    skew=bc.OUTSIDE_SKEW, poison=127 if input == "cs32" else 255, marker=marker)
    assert len(front) == len(back) == bc.OUTSIDE_GUARD
    assert (front == marker).all() and (back == marker).all()            # nothing written outside the rows
    assert np.array_equal(_bits(got), _bits(tight))                      # nothing read outside the frames

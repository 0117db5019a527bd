"""GPU suite of include/rtlws_anylen.h: f64 power spectra of any frame length 2 .. 2^19 (Bluestein over the four-step
transform, rtl-ws_amd/csrc/spectrum_anylen.hip) under the strict metric of the f64 batch tests (helpers.rel_err with
EPS_STRICT: 1e-10 over a floor of 1e-9 of the row maximum; f32 rows 6.0e-8).  The reference is the f64 oracle up
to 2048 points and tests/anylen_ref.rows (np.fft.fft and the row rules, pinned to the oracle by
tests/test_anylen_cpu.py) above: the oracle's direct long-double sum takes minutes per frame at 10^5 points.
The first tests launch every kernel instantiation (tests/anylen_kernels.py); those from test_border_lengths on walk the
borders of the frame length in pass 4's indexing (tests/anylen_border_cases.py) and hold what can be held bit for bit."""
import numpy as np
import pytest

import anylen_border_cases as bc
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
    # the group's offsets done * in_bytes and done / k_avg * row_bytes at the other sample and row sizes (8- and 4-byte
    # samples; 4-byte and, N being odd, unaligned 1-byte rows), and the dB epilogue
    rng = np.random.default_rng(N)
    s32 = rng.integers(-4000, 4000, size=(4, N, 2), dtype=np.int32)
    f32 = rng.standard_normal((4, N)).astype(np.float32)
    for what, data, kw in (("cs32, f32 rows", s32, dict(input="cs32", rows_f32=True)),
                           ("rf32, payload bytes, K = 2", f32, dict(input="rf32", k_avg=2, output="payload_u8", gain_db=9)),
                           ("cu8, mean_db", iq[:4], dict(k_avg=2, output="mean_db"))):
        a = engine.spectra_anylen(data, N, **kw)
        b = engine.spectra_anylen(data, N, max_frames=1, **kw)
        assert a.dtype == b.dtype and a.shape == (4 // kw.get("k_avg", 1), N) and a.any(), what
        assert np.array_equal(a.view(np.uint8), b.view(np.uint8)), what

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


# ---- the borders of the frame length (tests/anylen_border_cases.py) ----------------------------------------------

def _bits(a):
    """an array's bytes as unsigned integers of its item size: equality of these is equality bit for bit"""
    a = np.ascontiguousarray(a)
    return a.view({1: np.uint8, 4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def _border_inputs(N, F):
    from rtlws import synth
    rng = np.random.default_rng(N)
    return {"cu8": synth.tone_noise_iq(F, N, seed=N % 1000 + 2),
            "cs32": rng.integers(-4000, 4000, size=(F, N, 2), dtype=np.int32),
            "rf32": rng.standard_normal((F, N)).astype(np.float32)}


def _border_refs(oracle, data, N, input):
    """K -> reference rows for K = 1 and 3: the oracle up to 2048 points, np.fft.fft (one transform for both K) above"""
    if N <= ORACLE_MAX_N:
        return {K: _ref_rows(oracle, data, N, K, input) for K in (1, 3)}
    X = np.fft.fft(anylen_ref.convert(data, input).reshape(-1, N), axis=1)
    P = X.real ** 2 + X.imag ** 2
    return {K: anylen_ref.rows_from_powers(P, K) for K in (1, 3)}


@pytest.mark.parametrize("N", bc.LENGTHS)
def test_border_lengths(engine, oracle, N):
    """Every length of tests/anylen_border_cases.py (the reason of each is there): around the whole-workgroup return
    and N1 at M = 2^14, the first, the last odd, the last (M = 2 N) and an inner length of every larger M.  The three
    inputs at K = 1 and 3 with f64 rows; cmplx_u8 also with f32 rows and as payload bytes; the DC slot and its
    neighbour of every K = 3 row to 1e-13; a power of two also against rtlws_long.h on the same frames."""
    F = bc.frames_for(N)
    g = bc.geometry(N)
    data = _border_inputs(N, F)
    i0 = N - N // 2
    worst = {"f64": 0.0, "f32": 0.0, "dc": 0.0}
    for input in ("cu8", "cs32", "rf32"):
        ref = _border_refs(oracle, data[input], N, input)
        for K in (1, 3):
            got = engine.spectra_anylen(data[input], N, k_avg=K, input=input)
            assert got.shape == (F // K, N)
            if input == "cu8" and N in bc.POW2:
                _check("N=%d K=%d against rtlws_long.h" % (N, K), got, engine.spectra_long(data[input], N, k_avg=K), TOL_F64)
            worst["f64"] = max(worst["f64"], rel_err(got, ref[K], EPS_STRICT).max())
            _check("%s N=%d K=%d f64 rows" % (input, N, K), got, ref[K], TOL_F64)
        for r in range(F // 3):                                        # got, ref[3]: the K = 3 rows
            for slot in (i0, i0 - 1):
                rel = abs(got[r, slot] - ref[3][r, slot]) / ref[3][r, slot]
                worst["dc"] = max(worst["dc"], rel)
                print("%s N %d row %d slot %d: rel %.3g" % (input, N, r, slot, rel))
                assert rel <= 1e-13, (input, r, slot)
        if input == "cu8":
            got32 = engine.spectra_anylen(data[input], N, k_avg=3, rows_f32=True)
            assert got32.dtype == np.float32
            worst["f32"] = rel_err(got32, ref[3], EPS_STRICT).max()
            _check("cu8 N=%d K=3 f32 rows" % N, got32, ref[3], TOL_ROWS_F32)
            pay = engine.spectra_anylen(data[input], N, k_avg=3, output="payload_u8", gain_db=9)
            assert pay.shape == (F // 3, N) and pay.dtype == np.uint8
            for r in range(F // 3):
                assert np.array_equal(pay[r], _payload(ref[3][r], 3, 9)), (N, r)
    print("border N=%d (M=2^%d, owner of bin N-1 in tile %d of %d, column %d of %d, wrap %s, last run keeps %d): worst "
          "strict rel err f64 rows %.3g, f32 rows %.3g, DC slot and neighbour %.3g"
          % (N, g["m"], g["owner_tile"], g["tiles"], g["owner_col"], g["T"], "cuts a run" if g["wrap_cuts"] else "between runs",
             g["last_run_kept"] or g["T"], worst["f64"], worst["f32"], worst["dc"]))


@pytest.mark.parametrize("N2", sorted(bc.pass_b_lengths()))
def test_k_sums_are_the_k1_rows_added_in_order(engine, N2):
    """One length per pass-4 transform length.  K is a launch argument of one instantiation: the K = 3 run computes the
    same pw per frame and adds them in frame order to an accumulator that starts at zero, so outside the DC slot its
    row is (p0 + p1) + p2 of the K = 1 rows of the same frames bit for bit.  In a K = 1 row the DC slot carries
    0 + 1 * pw of bin N - 1: its neighbour's value, bit for bit."""
    N = bc.pass_b_lengths()[N2]
    assert bc.geometry(N)["N2"] == N2
    i0 = N - N // 2
    iq = _border_inputs(N, 3)["cu8"]
    p = engine.spectra_anylen(iq, N, k_avg=1)
    s = engine.spectra_anylen(iq, N, k_avg=3)
    assert p.shape == (3, N) and s.shape == (1, N)
    want = (p[0] + p[1]) + p[2]
    keep = np.arange(N) != i0
    assert np.array_equal(_bits(s[0][keep]), _bits(want[keep]))
    assert np.array_equal(_bits(p[:, i0]), _bits(p[:, i0 - 1]))
    assert len(set(p[:, i0].tolist())) == 3                            # the frames differ


@pytest.mark.parametrize("N", [bc.INNER_N[15], bc.INNER_N[16]], ids=["odd", "even"])
def test_power_of_two_scaling_is_exact(engine, N):
    """Frames times a power of two give rows times its square, bit for bit: such a scaling commutes with every
    rounding while nothing overflows or goes subnormal (the numpy restatement has the property exactly,
    tests/test_anylen_borders_cpu.py), so any path that depends on the input's size, any constant that is not a
    factor, and any workspace element read without having been written shows."""
    rng = np.random.default_rng(N + 1)
    f32 = rng.standard_normal((4, N)).astype(np.float32)
    base = engine.spectra_anylen(f32, N, k_avg=2, input="rf32")
    assert base.shape == (2, N) and np.isfinite(base).all() and base.min() > 0
    for e in (40, -40):
        scaled = f32 * np.float32(2.0 ** e)
        assert np.array_equal(scaled.astype(np.float64), f32.astype(np.float64) * 2.0 ** e)      # the frames scale exactly
        got = engine.spectra_anylen(scaled, N, k_avg=2, input="rf32")
        assert np.array_equal(_bits(got), _bits(base * 2.0 ** (2 * e))), e
    s32 = rng.integers(-(1 << 20), (1 << 20) + 1, size=(4, N, 2), dtype=np.int32)
    base = engine.spectra_anylen(s32, N, k_avg=2, input="cs32")
    got = engine.spectra_anylen(s32 << 8, N, k_avg=2, input="cs32")
    assert np.array_equal(_bits(got), _bits(base * 2.0 ** 16))
    _check("cs32 N=%d within 2^20" % N, base, anylen_ref.rows(s32, N, 2, "cs32"), TOL_F64)


def test_full_range_cs32(engine):
    """One cmplx_s32 frame drawn over all of int32, with INT32_MIN and INT32_MAX at its first and last sample: the
    conversion has no narrower type on its way.  The odd inner length of M = 2^15."""
    N = bc.INNER_N[15]
    lo, hi = -(1 << 31), (1 << 31) - 1
    s32 = np.random.default_rng(N + 2).integers(lo, hi + 1, size=(1, N, 2), dtype=np.int64).astype(np.int32)
    s32[0, 0] = (lo, hi)
    s32[0, N - 1] = (hi, lo)
    _check("cs32 N=%d over all of int32" % N, engine.spectra_anylen(s32, N, input="cs32"),
           anylen_ref.rows(s32, N, 1, "cs32"), TOL_F64)


@pytest.mark.parametrize("N,F", [(129, 5), (bc.INNER_N[15], 4), (bc.INNER_N[16], 4)])
def test_frame_place_does_not_matter(engine, N, F):
    """One frame at places 0, 1 and F - 1 of a batch of otherwise different frames gives the same row, bit for bit.
    Passes 1 and 3 deal their grid (F M / 8192 workgroups) through xcd_chunked: the identity at 5 frames of M = 2^14
    (10 workgroups), a permutation that sends a frame's tiles to different chunks at 4 frames of M = 2^15 (16) and of
    M = 2^16 (32)."""
    grid = F << (bc.geometry(N)["m"] - 13)
    assert (grid % 8 == 0) == (N != 129)
    iq = _border_inputs(N, F)["cu8"].copy()
    iq[1] = iq[0]
    iq[F - 1] = iq[0]
    assert not np.array_equal(iq[2], iq[0])
    got = engine.spectra_anylen(iq, N)
    assert np.array_equal(_bits(got[1]), _bits(got[0])) and np.array_equal(_bits(got[F - 1]), _bits(got[0]))
    assert not np.array_equal(got[2], got[0])
    _check("N=%d, %d frames" % (N, F), got, anylen_ref.rows(iq, N, 1), TOL_F64)


@pytest.mark.parametrize("input,rows", [("cs32", "f32"), ("rf32", "u8"), ("cu8", "f32")])
def test_batch_end_without_slack_by_kind(engine, built, input, rows):
    """test_batch_end_without_slack at the other sample and row sizes, N odd: the frames begin one sample after a
    sample-aligned guard and end where another begins, both poison (bytes 255: a NaN as real_f32, full scale as
    cmplx_u8; bytes 127: about 2^31 / 128 as cmplx_s32); the rows lie between markers that must survive.  Payload rows
    begin at a 4-byte boundary and, N being odd, every other one at an odd byte."""
    N, F, G = 1001, 3, 1024
    data = _border_inputs(N, F)[input]
    kw = dict(rows_f32=True) if rows == "f32" else dict(output="payload_u8", gain_db=9)
    out_dtype, marker = (np.float32, np.float32(-7.0)) if rows == "f32" else (np.uint8, np.uint8(0xA5))
    tight = engine.spectra_anylen(data, N, input=input, **kw)           # exactly-sized buffers
    ref = anylen_ref.rows(data, N, 1, input)
    if rows == "f32":
        _check("%s odd N, exactly-sized buffers, f32 rows" % input, tight, ref, TOL_ROWS_F32)
    else:
        assert np.array_equal(tight, _payload(ref, 1, 9))
    sample = data.nbytes // (F * N)
    raw = np.full(G + sample + data.nbytes + G, 127 if input == "cs32" else 255, dtype=np.uint8)
    raw[G + sample:G + sample + data.nbytes] = data.reshape(-1).view(np.uint8)
    d_in = engine.upload(raw)
    d_out = engine.upload(np.full(G + F * N + G, marker, dtype=out_dtype))
    item = np.dtype(out_dtype).itemsize
    desc = built.make_desc(N, input=input, output=kw.get("output", "power_sum"), gain_db=kw.get("gain_db", 0),
                           flags=built.FLAG_ROWS_F32 if rows == "f32" else 0)
    plan = built.AnyLenPlan(engine, desc, max_frames=F)
    plan.run(d_in.ptr + G + sample, F, d_out.ptr + item * G)
    o = engine.download(d_out, out_dtype, (G + F * N + G,))
    plan.close()
    d_in.free()
    d_out.free()
    assert (o[:G] == marker).all() and (o[G + F * N:] == marker).all()   # nothing written outside the rows
    assert np.array_equal(_bits(o[G:G + F * N].reshape(F, N)), _bits(tight))   # nothing read outside the frames

"""GPU suite of include/rtlws_pfbspec.h: the polyphase spectrometer (the filter bank's tile, squared and summed over K
frames where the transform leaves it, one launch) against the channelizer's own samples bit for bit (K = 1) and
against the numpy restatement tests/pfbspec_ref.py.

The accuracy criterion is derived, not measured (pfbspec_ref.bound): per row
||got - ref||_1 <= (16 (log2 M + 1) + K + 4) 2^-24 ||ref||_1."""
import numpy as np
import pytest

import pfb_ref
import pfbspec_ref

pytestmark = pytest.mark.gpu

NSPECTRA = (1, 2, 5)
ORDER_SHAPES = [(4, 7), (6, 8), (8, 8), (10, 4)]


def tile_of(built, k):
    rc, _, _, _, t = built.pfb_grid(k, 1, 1 << k, 1)
    assert rc == 0 and t >= 4
    return t


def k_list(t):
    return sorted({K for K in (2, 3, 6, t - 1, t, t + 1, 2 * t + 3) if K >= 2})


def worst_ratio(got, ref, k, k_avg):
    """max over rows of ||got - ref||_1 / (bound ||ref||_1); got, ref [nspectra, M]."""
    err = np.abs(got.astype(np.float64) - ref).sum(axis=1)
    nrm = np.abs(ref).sum(axis=1)
    assert np.all(nrm > 0)
    return float((err / (pfbspec_ref.bound(k, k_avg) * nrm)).max())


@pytest.mark.parametrize("k,T", pfb_ref.SHAPES)
def test_k1_is_the_channelizer_squared_bit_for_bit(engine, built, k, T):
    """K = 1, raw sums, unshifted: fl(fl(re re) + fl(im im)) of rtlws_pfb_run's time-major samples of the same capture,
    formed in numpy f32 and compared as uint32: the transform, the table and the indexing are the channelizer's."""
    M = 1 << k
    t = tile_of(built, k)
    taps = pfb_ref.random_taps(k, T, seed=100 * k + T)
    for D in (M, M // 2):
        for n in (1, t - 1, t, t + 1, 2 * t + 3):
            iq = pfb_ref.random_iq(pfb_ref.samples_needed(M, T, D, n), seed=k + T + n)
            y = engine.pfb(iq, k, taps, hop=D, layout="time")
            assert y.shape == (n, M) and y.dtype == np.complex64
            re, im = y.real.astype(np.float32), y.imag.astype(np.float32)
            want = (re * re).astype(np.float32) + (im * im).astype(np.float32)
            assert want.dtype == np.float32 and np.any(want != 0)
            got = engine.pfbspec(iq, k, taps, 1, hop=D)
            assert got.shape == (n, M) and got.dtype == np.float32
            assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (D, n)


@pytest.mark.parametrize("k,T", pfb_ref.SHAPES)
def test_k_sums_against_f64(engine, built, k, T):
    M = 1 << k
    t = tile_of(built, k)
    ks = k_list(t)
    longest = max(ks) * max(NSPECTRA)
    worst = 0.0
    for D in (M, M // 2):
        nmax = pfb_ref.samples_needed(M, T, D, longest)
        rnd_taps = pfb_ref.random_taps(k, T, seed=100 * k + T)
        cases = (("random", pfb_ref.random_iq(nmax, seed=k + T), rnd_taps),
                 ("full scale", pfb_ref.full_scale_iq(nmax, seed=k * T), np.full(T * M, 32767, np.int16)),
                 ("tone in noise", pfbspec_ref.tone_noise_iq(nmax, (M // 4 + 1.3) / M, seed=7 * k + T),
                  pfbspec_ref.designed_taps(k, T)))
        for kind, iq, taps in cases:
            frames = pfb_ref.pfb_ref(iq, k, taps, D)             # a shorter run is a prefix: the same frames
            assert frames.shape == (longest, M)
            for K in ks:
                ref = pfbspec_ref.k_sums(frames, K)
                for n in NSPECTRA:
                    got = engine.pfbspec(iq[:pfbspec_ref.samples_needed(M, T, D, K, n)], k, taps, K, hop=D)
                    assert got.shape == (n, M) and got.dtype == np.float32
                    r = worst_ratio(got, ref[:n], k, K)
                    worst = max(worst, r)
                    assert r <= 1.0, (kind, D, K, n, r)
            if kind == "tone in noise":                        # a spectrum with a peak: a permuted row would show
                assert np.all(np.argmax(ref, axis=1) == M // 4 + 1)
        mid = np.full((nmax, 2), 128, dtype=np.uint8)
        for K in ks:
            for n in NSPECTRA:
                z = engine.pfbspec(mid[:pfbspec_ref.samples_needed(M, T, D, K, n)], k, rnd_taps, K, hop=D)
                assert z.shape == (n, M) and not z.any() and not np.signbit(z).any(), (D, K, n)
    print("M = %d, T = %d: worst ||got - ref||_1 / bound = %.4f (K = %s)" % (M, T, worst, ks))


@pytest.mark.parametrize("k,T", ORDER_SHAPES)
def test_the_order_of_the_sum_knows_only_m_and_k(engine, built, k, T):
    M = 1 << k
    t = tile_of(built, k)
    taps = pfb_ref.random_taps(k, T, seed=k)
    for K in (3, t + 1):
        per = built.pfbspec_grid(k, T, M, K, 1)[4]
        n = 2 * per + 3                                        # three workgroups, the last one partly filled
        j0 = per // 2 + 1                                      # rows that change their place in the tile and in the grid
        rows = {}
        for D in (M, M // 2):
            iq = pfb_ref.random_iq(pfbspec_ref.samples_needed(M, T, D, K, n), seed=T + K)
            whole = engine.pfbspec(iq, k, taps, K, hop=D)
            assert whole.shape == (n, M) and np.all(whole > 0)
            again = engine.pfbspec(iq, k, taps, K, hop=D)
            assert np.array_equal(again.view(np.uint32), whole.view(np.uint32)), (K, D)
            for start in (j0, n - 1):
                part = engine.pfbspec(iq[start * K * D:], k, taps, K, hop=D)
                assert part.shape == (n - start, M)
                assert np.array_equal(part.view(np.uint32), whole[start:].view(np.uint32)), (K, D, start)
            shifted = engine.pfbspec(iq, k, taps, K, hop=D, shifted=True)
            assert np.array_equal(shifted.view(np.uint32), np.fft.fftshift(whole, axes=1).view(np.uint32)), (K, D)
            rows[D] = whole
        # one capture at both hops: other frames, other sums
        iq = pfb_ref.random_iq(pfbspec_ref.samples_needed(M, T, M, K, n), seed=T + K)
        assert not np.array_equal(engine.pfbspec(iq, k, taps, K, hop=M // 2, nspectra=n), rows[M])


@pytest.mark.parametrize("k,T,hop_div", pfbspec_ref.DB_SHAPES)
def test_db_and_bytes(engine, built, k, T, hop_div):
    """Tied to the device's own sums, which are deterministic: MEAN_DB within 2e-4 dB (rtlws_hip.h's figure for this
    output kind) of 10 log10(S_gpu lin) in f64; PAYLOAD_U8 equal to the truncated, clamped f64 value except +-1
    where that value lies within 1e-3 of an integer, for at most 1 % of a case's bytes."""
    M = 1 << k
    t = tile_of(built, k)
    n = pfbspec_ref.DB_NSPECTRA
    for K in (3, t + 1):
        iq, taps, D, scale = pfbspec_ref.db_case(k, T, hop_div, K)
        sums = engine.pfbspec(iq, k, taps, K, hop=D, nspectra=n)
        assert worst_ratio(sums, pfbspec_ref.pfbspec_ref(iq, k, taps, K, D, nspectra=n), k, K) <= 1.0
        for sc, kind in ((scale, "in range"), (scale * 1e-12, "clamped at 0"), (scale * 1e20, "clamped at 255")):
            for shifted in (False, True):
                s = np.fft.fftshift(sums, axes=1) if shifted else sums
                want = pfbspec_ref.db(s, sc, K)
                got = engine.pfbspec(iq, k, taps, K, hop=D, output="db", shifted=shifted, scale=sc, nspectra=n)
                assert got.shape == (n, M) and got.dtype == np.float32
                err = np.abs(got.astype(np.float64) - want).max()
                assert err <= 2e-4, (K, kind, shifted, err)
                byt = engine.pfbspec(iq, k, taps, K, hop=D, output="payload", shifted=shifted, scale=sc, nspectra=n)
                assert byt.shape == (n, M) and byt.dtype == np.uint8
                exact = pfbspec_ref.payload(want)
                off = byt != exact
                assert np.all(np.abs(byt.astype(int) - exact.astype(int))[off] == 1), (K, kind)
                assert np.all(pfbspec_ref.near_integer(want, 1e-3)[off]), (K, kind)
                assert off.mean() <= 0.01, (K, kind, off.mean())
                if kind == "in range":
                    assert 20.0 <= want.min() and want.max() <= 120.0
                elif kind == "clamped at 0":
                    assert want.max() < 0.0 and not byt.any()
                else:
                    assert want.max() > 256.0 and (byt == 255).any() and np.all(byt[want >= 255.0] == 255)
    # all-128 input: exact zeros, -inf, bytes 0
    taps = pfbspec_ref.designed_taps(k, T)
    D = M // hop_div
    for K in k_list(t):
        for n in NSPECTRA:
            mid = np.full((pfbspec_ref.samples_needed(M, T, D, K, n), 2), 128, dtype=np.uint8)
            assert not engine.pfbspec(mid, k, taps, K, hop=D).any()
            d = engine.pfbspec(mid, k, taps, K, hop=D, output="db", scale=3.0)
            assert d.shape == (n, M) and np.all(np.isneginf(d)), (K, n)
            assert not engine.pfbspec(mid, k, taps, K, hop=D, output="payload", scale=3.0).any()


def test_stride_and_nothing_outside_the_rows(engine, built):
    k, T, K = 5, 3, 3
    M = 1 << k
    per = built.pfbspec_grid(k, T, M, K, 1)[4]
    n = per + 3                                                # two workgroups, the second partly filled
    taps = pfb_ref.random_taps(k, T, seed=21)
    plan = built.PfbSpecPlan.open(engine, k, taps)
    for D in (M, M // 2):
        iq = pfb_ref.random_iq(pfbspec_ref.samples_needed(M, T, D, K, n), seed=22)
        ref = pfbspec_ref.pfbspec_ref(iq, k, taps, K, D)
        d_iq = engine.upload(iq)
        for output, dtype, sentinel, stride in (("power", np.float32, np.float32(-12345.5), M + 4),
                                                ("db", np.float32, np.float32(-12345.5), M + 4),
                                                ("payload", np.uint8, np.uint8(0xA5), M + 16)):
            tail = 64
            total = n * stride + tail
            d_out = engine.upload(np.full(total, sentinel, dtype=dtype))
            plan.run(d_iq, n, K, d_out, hop=D, output=output, scale=1e-9, out_stride=stride)
            engine.sync()
            out = engine.download(d_out, dtype, (total,))
            body = out[:n * stride].reshape(n, stride)
            got = body[:, :M]
            if output == "power":
                assert worst_ratio(got, ref, k, K) <= 1.0, D
            else:
                want = pfbspec_ref.db(ref, 1e-9, K)
                assert np.abs((got if output == "db" else got.astype(np.float64) + 0.5) - want).max() <= 1.0
                assert np.all(got != sentinel)
            assert np.all(body[:, M:] == sentinel) and np.all(out[n * stride:] == sentinel), (D, output)
            # no spectra: nothing happens; with a device the refusals still hold and write nothing
            assert plan.run(d_iq, 0, K, d_out, hop=D, output=output, out_stride=stride) == 0
            for kw, word in (({"hop": M // 4}, "hop"), ({"hop": 2 * M}, "hop"), ({"out_stride": 16}, "out_stride"),
                             ({"out_stride": stride + 2}, "multiple"), ({"shifted": 2}, "shifted"), ({"scale": 0.0}, "scale")):
                if output == "power" and "scale" in kw:
                    continue
                args = dict(hop=D, output=output, out_stride=stride)
                args.update(kw)
                assert plan.run(d_iq, n, K, d_out, check=False, **args) == -1 and word in built.pfbspec_last_error(), kw
            assert plan.run(d_iq, n, 0, d_out, hop=D, output=output, out_stride=stride, check=False) == -1
            assert "k_avg" in built.pfbspec_last_error()
            assert plan.run(d_iq.ptr + 8, n, K, d_out, hop=D, output=output, out_stride=stride, check=False) == -1
            assert "16-byte" in built.pfbspec_last_error()
            assert plan.run(d_iq, n, K, d_out.ptr + 4, hop=D, output=output, out_stride=stride, check=False) == -1
            assert "16-byte" in built.pfbspec_last_error()
            assert plan.run(d_iq, -1, K, d_out, hop=D, output=output, out_stride=stride, check=False) == -1
            assert "nspectra" in built.pfbspec_last_error()
            engine.sync()
            again = engine.download(d_out, dtype, (total,))
            assert np.array_equal(again.view(np.uint8), out.view(np.uint8))
            d_out.free()
        d_iq.free()
    plan.close()


def test_capture_and_replay(built):
    """A run is one kernel launch: captured on a side stream the way tests/test_pfb_gpu.py captures the channelizer,
    replayed twice, identical to an eager launch."""
    import torch
    dev = torch.device("cuda", 0)
    eng = built.Engine(0)
    k, T, K = 6, 4, 5
    M, D = 1 << k, 1 << (k - 1)
    n = built.pfbspec_grid(k, T, D, K, 1)[4] + 5
    taps = pfb_ref.random_taps(k, T, seed=31)
    plan = built.PfbSpecPlan.open(eng, k, taps)
    iq_host = pfb_ref.random_iq(pfbspec_ref.samples_needed(M, T, D, K, n), seed=32)
    iq = torch.from_numpy(iq_host).to(dev)
    out = torch.zeros((n, M), dtype=torch.float32, device=dev)

    def launch(o):
        plan.run(iq.data_ptr(), n, K, o.data_ptr(), hop=D, shifted=True, stream=built.torch_stream_handle())

    g = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        with torch.cuda.graph(g, stream=side):
            launch(out)
    torch.cuda.current_stream().wait_stream(side)
    assert float(out.abs().sum()) == 0.0                 # capture enqueued nothing
    g.replay()
    torch.cuda.synchronize()
    first = out.clone()
    out.zero_()
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(first, out)
    eager = torch.zeros_like(out)
    launch(eager)
    torch.cuda.synchronize()
    assert torch.equal(first, eager)
    assert worst_ratio(out.cpu().numpy(), pfbspec_ref.pfbspec_ref(iq_host, k, taps, K, D, shifted=True), k, K) <= 1.0
    plan.close()
    eng.close()


def test_selectivity_through_the_spectrometer(engine, built):
    """pfb_ref.selectivity_case() as one row of K = 64: leakage two or more channels from the tone's neighbours,
    the thresholds of DESIGN.md 4.14."""
    k, T, c0, iq, boxcar = pfb_ref.selectivity_case()
    designed = engine.pfbspec(iq, k, built.pfb_design(k, T), 64)
    box = engine.pfbspec(iq, k, boxcar, 64)
    assert designed.shape == box.shape == (1, 1 << k)
    ld = pfbspec_ref.leakage_db_of_row(designed[0].astype(np.float64), c0)
    lb = pfbspec_ref.leakage_db_of_row(box[0].astype(np.float64), c0)
    print("leakage two or more channels away: designed prototype %.1f dB, boxcar %.1f dB" % (ld, lb))
    assert ld <= -40.0
    assert lb >= -15.0

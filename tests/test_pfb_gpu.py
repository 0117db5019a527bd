"""GPU suite of include/rtlws_pfb.h: the polyphase channelizer (integer branch filters and one f32 M-point transform
per frame, one launch for all M channels) against the numpy restatement tests/pfb_ref.py.

The accuracy criterion is derived, not measured: the branch sums are exact, so the error is one conversion to f32 and
the f32 transform; per frame ||got - ref||_2 <= 8 (log2 M + 1) 2^-24 ||ref||_2 (pfb_ref.bound)."""
import numpy as np
import pytest

import pfb_ref

pytestmark = pytest.mark.gpu


def tile_of(built, k):
    rc, _, _, _, t = built.pfb_grid(k, 1, 1 << k, 1)
    assert rc == 0 and t >= 4
    return t


def worst_ratio(got, ref, k):
    """max over frames of ||got - ref||_2 / (bound ||ref||_2); got, ref [nframes, M]."""
    err = np.linalg.norm(got.astype(np.complex128) - ref, axis=1)
    nrm = np.linalg.norm(ref, axis=1)
    assert np.all(nrm > 0)
    return float((err / (pfb_ref.bound(k) * nrm)).max())


@pytest.mark.parametrize("k,T", pfb_ref.SHAPES)
def test_matrix(engine, built, k, T):
    M = 1 << k
    t = tile_of(built, k)
    counts = (1, t - 1, t, t + 1, 2 * t + 3)
    longest = counts[-1]
    worst = 0.0
    for D in (M, M // 2):
        nmax = pfb_ref.samples_needed(M, T, D, longest)
        cases = (("random", pfb_ref.random_iq(nmax, seed=k + T), pfb_ref.random_taps(k, T, seed=100 * k + T)),
                 ("full scale", pfb_ref.full_scale_iq(nmax, seed=k * T), np.full(T * M, 32767, np.int16)))
        for kind, iq, taps in cases:
            ref = pfb_ref.pfb_ref(iq, k, taps, D)             # a shorter run is a prefix: the same absolute indices
            assert ref.shape == (longest, M)
            if kind == "full scale" and T >= 7:
                v = np.fft.ifft(ref, axis=1)
                assert max(np.abs(v.real).max(), np.abs(v.imag).max()) > 2 ** 24
            for layout in ("time", "channel"):
                whole = None
                for n in reversed(counts):
                    got = engine.pfb(iq[:pfb_ref.samples_needed(M, T, D, n)], k, taps, hop=D, layout=layout)
                    if layout == "channel":
                        assert got.shape == (M, n)
                        got = got.T
                    assert got.shape == (n, M) and got.dtype == np.complex64
                    r = worst_ratio(got, ref[:n], k)
                    worst = max(worst, r)
                    assert r <= 1.0, (kind, D, layout, n, r)
                    if whole is None:
                        whole = got
                    assert np.array_equal(got, whole[:n]), (kind, D, layout, n)
        mid = np.full((nmax, 2), 128, dtype=np.uint8)
        for layout in ("time", "channel"):
            for n in counts:
                assert not engine.pfb(mid[:pfb_ref.samples_needed(M, T, D, n)], k, cases[0][2], hop=D, layout=layout).any(), n
    print("M = %d, T = %d: worst ||got - ref|| / bound = %.4f (bound %.3g)" % (M, T, worst, pfb_ref.bound(k)))


@pytest.mark.parametrize("k,T", [(4, 7), (6, 8), (8, 8), (10, 4)])
def test_layouts_agree_and_the_sign_rule_is_exact(engine, built, k, T):
    M = 1 << k
    t = tile_of(built, k)
    n = 2 * t + 3
    taps = pfb_ref.random_taps(k, T, seed=k)
    for D in (M, M // 2):
        iq = pfb_ref.random_iq(pfb_ref.samples_needed(M, T, D, n), seed=T)
        by_time = engine.pfb(iq, k, taps, hop=D, layout="time")
        by_channel = engine.pfb(iq, k, taps, hop=D, layout="channel")
        assert np.array_equal(by_channel.T, by_time)
        assert np.array_equal(engine.pfb(iq, k, taps, hop=D, layout="time"), by_time)      # two runs of one input
        shifted = engine.pfb(iq, k, taps, hop=D, first_frame_index=1, layout="time")
        if D == M:
            assert np.array_equal(shifted, by_time)
        else:
            assert np.array_equal(shifted[:, 0::2], by_time[:, 0::2])
            assert np.array_equal(shifted[:, 1::2], -by_time[:, 1::2])
            assert np.any(by_time[:, 1::2] != 0)


@pytest.mark.parametrize("first", [0, (1 << 40) + 12345])
def test_chunks_concatenate_to_one_run(engine, built, first):
    k, T = 6, 8
    M, D = 1 << k, 1 << (k - 1)
    t = tile_of(built, k)
    n = 3 * t + 5
    taps = pfb_ref.random_taps(k, T, seed=11)
    iq = pfb_ref.random_iq(pfb_ref.samples_needed(M, T, D, n), seed=12)
    whole = engine.pfb(iq, k, taps, hop=D, first_frame_index=first, layout="time")
    assert worst_ratio(whole, pfb_ref.pfb_ref(iq, k, taps, D, first), k) <= 1.0
    cuts = (0, t + 3, 2 * t + 1, n)
    for layout, axis in (("time", 0), ("channel", 1)):
        parts = [engine.pfb(iq[a * D:(b - 1) * D + T * M], k, taps, hop=D, first_frame_index=first + a, layout=layout)
                 for a, b in zip(cuts, cuts[1:])]
        got = np.concatenate(parts, axis=axis)
        assert np.array_equal(got if axis == 0 else got.T, whole), layout
    # the absolute index is in the sign: the middle chunk starts at an odd frame
    assert (t + 3) % 2 == 1
    a, b = cuts[1], cuts[2]
    assert not np.array_equal(engine.pfb(iq[a * D:(b - 1) * D + T * M], k, taps, hop=D, first_frame_index=first, layout="time"),
                              whole[a:b])


def test_stride_and_nothing_outside_the_streams(engine, built):
    k, T = 5, 3
    M = 1 << k
    t = tile_of(built, k)
    n = t + 1
    taps = pfb_ref.random_taps(k, T, seed=21)
    sentinel = np.complex64(12345.5 - 54321.25j)
    plan = built.PfbPlan.open(engine, k, taps)
    for D in (M, M // 2):
        iq = pfb_ref.random_iq(pfb_ref.samples_needed(M, T, D, n), seed=22)
        ref = pfb_ref.pfb_ref(iq, k, taps, D, 3)
        d_iq = engine.upload(iq)
        for layout, rows, run_len in (("channel", M, n), ("time", n, M)):
            stride, tail = run_len + 7, 64
            total = rows * stride + tail
            d_out = engine.upload(np.full(total, sentinel, dtype=np.complex64))
            plan.run(d_iq, n, d_out, hop=D, out_stride=stride, first_frame_index=3, layout=layout)
            engine.sync()
            out = engine.download(d_out, np.complex64, (total,))
            body = out[:rows * stride].reshape(rows, stride)
            got = body[:, :run_len] if layout == "time" else body[:, :run_len].T
            assert worst_ratio(got, ref, k) <= 1.0, (D, layout)
            assert np.all(body[:, run_len:] == sentinel) and np.all(out[rows * stride:] == sentinel), (D, layout)
            # no frames: nothing happens; with a device the refusals still hold and write nothing
            assert plan.run(d_iq, 0, d_out, hop=D, out_stride=0 if layout == "channel" else M, layout=layout) == 0
            for kw, word in (({"out_stride": run_len - 1}, "out_stride"), ({"hop": M // 4}, "hop"), ({"hop": 2 * M}, "hop"),
                             ({"first_frame_index": -1}, "first_frame_index"), ({"layout": 2}, "layout")):
                args = dict(hop=D, out_stride=stride, first_frame_index=3, layout=layout)
                args.update(kw)
                assert plan.run(d_iq, n, d_out, check=False, **args) == -1 and word in built.pfb_last_error(), kw
            assert plan.run(d_iq.ptr + 8, n, d_out, hop=D, out_stride=stride, layout=layout, check=False) == -1
            assert "16-byte" in built.pfb_last_error()
            assert plan.run(d_iq, n, d_out.ptr + 4, hop=D, out_stride=stride, layout=layout, check=False) == -1
            assert "8-byte" in built.pfb_last_error()
            assert plan.run(d_iq, -1, d_out, hop=D, out_stride=stride, layout=layout, check=False) == -1
            engine.sync()
            assert np.array_equal(engine.download(d_out, np.complex64, (total,)).view(np.uint32), out.view(np.uint32))
            d_out.free()
        d_iq.free()
    plan.close()


def test_capture_and_replay(built):
    """A run is one kernel launch: captured on a side stream the way tests/test_ddc_gpu.py captures the bank, replayed
    twice, identical to an eager launch."""
    import torch
    dev = torch.device("cuda", 0)
    eng = built.Engine(0)
    k, T = 6, 4
    M, D = 1 << k, 1 << (k - 1)
    n = tile_of(built, k) + 5
    taps = pfb_ref.random_taps(k, T, seed=31)
    plan = built.PfbPlan.open(eng, k, taps)
    iq_host = pfb_ref.random_iq(pfb_ref.samples_needed(M, T, D, n), seed=32)
    iq = torch.from_numpy(iq_host).to(dev)
    out = torch.zeros((M, n), dtype=torch.complex64, device=dev)

    def launch(o):
        plan.run(iq.data_ptr(), n, o.data_ptr(), hop=D, first_frame_index=77, layout="channel",
                 stream=built.torch_stream_handle())

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
    assert worst_ratio(out.cpu().numpy().T, pfb_ref.pfb_ref(iq_host, k, taps, D, 77), k) <= 1.0
    plan.close()
    eng.close()


def test_one_flat_tap_is_the_bank(engine, built):
    """M = 32, T = 1, h = 1, hop M against rtlws_ddc_run at R = 32 with the words of the 32 channel centres: two
    independent kernels on one transform.  The bank lies within 0.5 + R / 64 of the ideal per component
    (DESIGN.md 4.12), this one within its f32 bound's 2-norm of it."""
    k = 5
    M = 1 << k
    n = 2 * tile_of(built, k) + 3
    iq = pfb_ref.random_iq(n * M, seed=41)
    words = [((c * 2048 + 32768) % 65536) - 32768 for c in range(M)]
    bank = engine.ddc(iq, M, words)
    got = engine.pfb(iq, k, np.ones(M, np.int16), hop=M, layout="channel")
    ref = pfb_ref.pfb_ref(iq, k, np.ones(M, np.int16), M)
    assert bank.shape == (M, n, 2) and got.shape == (M, n)
    tol = 0.5 + 32 / 64 + 8 * 6 * 2.0 ** -24 * np.linalg.norm(ref, axis=1)       # per frame
    assert np.all(np.abs(got.real.astype(np.float64) - bank[..., 0]) <= tol[None, :])
    assert np.all(np.abs(got.imag.astype(np.float64) - bank[..., 1]) <= tol[None, :])
    assert np.abs(bank).max() > 100


def test_selectivity_on_the_device(engine, built):
    k, T, c0, iq, boxcar = pfb_ref.selectivity_case()
    designed = pfb_ref.leakage_db(engine.pfb(iq, k, built.pfb_design(k, T), layout="time").astype(np.complex128), c0)
    box = pfb_ref.leakage_db(engine.pfb(iq, k, boxcar, layout="time").astype(np.complex128), c0)
    print("leakage two or more channels away: designed prototype %.1f dB, boxcar %.1f dB" % (designed, box))
    assert designed <= -40.0
    assert box >= -15.0

"""GPU suite of include/rtlws_ddc.h: the down-converter bank (integer NCO mixer fused with the CIC, one launch for
all channels) against the numpy restatement tests/ddc_ref.py.  Every comparison is np.array_equal: each output
integer is defined."""
import numpy as np
import pytest

import ddc_family_channels as channels
import ddc_ref
import fm_ref

pytestmark = pytest.mark.gpu

P = ddc_ref.P
SPECIAL_WORDS = (0, 1, -1, -32768, 32767)
SENTINEL = np.int32(-0x12345678)


@pytest.fixture(scope="module")
def tile(built):
    rc, _, _, _, t = built.ddc_grid(8, 1, 1)
    assert rc == 0 and t >= 16
    return t


def words_for(C, seed):
    """C tuning words: seeded random ones, the special ones at positions 1 .. as far as they fit, and the last
    channel on the first one's word."""
    w = [int(k) for k in np.random.default_rng(seed).integers(-P // 2, P // 2, C)]
    for i, s in enumerate(SPECIAL_WORDS):
        if 1 + i < C - 1:
            w[1 + i] = s
    if C >= 2:
        w[C - 1] = w[0]
    return w


@pytest.mark.parametrize("R", [1, 7, 8, 10, 12, 128])
def test_word_zero_is_the_cic(engine, tile, R):
    """k = 0, one channel: rtlws_cic_block_sums on the same input (T[0] = (16384, 0))."""
    n = 2 * tile + 3
    iq = ddc_ref.random_iq(n * R, seed=R)
    d_iq = engine.upload(iq)
    d_cic = engine.alloc(n * 8)
    engine.cic_block_sums(R, d_iq, n, d_cic)
    engine.sync()
    cic = engine.download(d_cic, np.int32, (n, 2))
    d_iq.free(), d_cic.free()
    got = engine.ddc(iq, R, [0], first_dec_index=987654321)
    assert got.shape == (1, n, 2)
    assert np.array_equal(got[0], cic)
    assert np.array_equal(cic, ddc_ref.block_sums(iq, R))


# every R and every C at least once; C = 8 | 9 are the two sides of a column-tile border, R = 16 | 17 of a K step
BANKS = [(1, 1), (2, 2), (3, 8), (7, 9), (8, 32), (10, 1), (12, 9), (16, 8), (17, 2), (33, 32), (128, 32), (8, 1), (12, 2),
         (10, 32)]


@pytest.mark.parametrize("R,C", BANKS)
def test_bank_matrix(engine, tile, R, C):
    t = tile
    words = words_for(C, seed=1000 * R + C)
    if C >= 8:
        assert set(SPECIAL_WORDS) <= set(words)
    longest = 3 * t + 5
    for kind, make in (("random", ddc_ref.random_iq), ("full scale", ddc_ref.full_scale_iq)):
        iq = make(longest * R, seed=R + C)
        want = ddc_ref.ddc_ref(iq, R, words)             # a shorter run is a prefix: the same absolute indices
        for n in (1, t - 1, t, t + 1, longest):
            got = engine.ddc(iq[:n * R], R, words)
            assert got.shape == (C, n, 2)
            bad = np.argwhere(got != want[:, :n])
            assert bad.size == 0, (kind, n, bad[:4], got[tuple(bad[0])], want[tuple(bad[0])])
            if C >= 2:
                assert np.array_equal(got[0], got[C - 1])
    mid = np.full((longest * R, 2), 128, dtype=np.uint8)
    for n in (1, t - 1, t, t + 1, longest):
        assert not engine.ddc(mid[:n * R], R, words).any(), n


@pytest.mark.parametrize("R", channels.paths("ddc"), ids=channels.path_id)
def test_every_channel_count(engine, built, tile, R):
    """tests/ddc_family_channels.py: C = 1 .. 32 of one set of 32 words over one capture, tile + 17 decimated samples.
    Every launch goes through the plan's run into 32 rows of out_stride > dec_len and a tail, all sentinels: rows
    0 .. C - 1 are the first C of the 32-channel restatement, every other word is untouched -- a ninth "channel" of a
    partly filled column tile would land in row C."""
    n = channels.stream_len(tile)
    stride, tail = n + 7, 64
    rows = channels.MAX_CH
    want = channels.stream_expected("ddc", R, tile)
    fill = np.full((rows * stride + tail, 2), SENTINEL, dtype=np.int32)
    plan = built.DdcPlan.open(engine)
    d_iq = engine.upload(channels.stream_inputs("ddc", R, tile))
    for C in channels.channels("ddc", R):
        rc, blocks, _, _, t = built.ddc_grid(R, C, n)
        assert rc == 0 and t == tile and blocks == -(-n // tile) * 1
        d_out = engine.upload(fill)
        plan.run(R, d_iq, n, channels.WORDS[:C], d_out, out_stride=stride, first_dec_index=channels.FIRST)
        engine.sync()
        out = engine.download(d_out, np.int32, fill.shape)
        d_out.free()
        body = out[:rows * stride].reshape(rows, stride, 2)
        bad = np.argwhere(body[:C, :n] != want[:C])
        assert bad.size == 0, (C, len(bad), bad[:4])
        assert np.all(body[:C, n:] == SENTINEL) and np.all(body[C:] == SENTINEL) and np.all(out[rows * stride:] == SENTINEL), C
    plan.close()
    d_iq.free()


@pytest.mark.parametrize("first", [0, (1 << 40) + 12345])
def test_chunks_concatenate_to_one_run(engine, tile, first):
    t = tile
    R, words = 10, [777, -20001, 32767]
    n = 3 * t + 5
    iq = ddc_ref.random_iq(n * R, seed=5)
    whole = engine.ddc(iq, R, words, first_dec_index=first)
    assert np.array_equal(whole, ddc_ref.ddc_ref(iq, R, words, first))
    cuts = (0, t + 3, 2 * t + 1, n)
    parts = [engine.ddc(iq[a * R:b * R], R, words, first_dec_index=first + a) for a, b in zip(cuts, cuts[1:])]
    assert np.array_equal(np.concatenate(parts, axis=1), whole)
    if first:
        assert not np.array_equal(whole, engine.ddc(iq, R, words))            # the absolute index is in the phase


def test_stride_and_nothing_outside_the_streams(engine, built, tile):
    R, C = 12, 9
    n = tile + 1
    stride, tail = n + 7, 64
    words = words_for(C, seed=3)
    iq = ddc_ref.random_iq(n * R, seed=4)
    sentinel = np.int32(-0x12345678)
    plan = built.DdcPlan.open(engine)
    d_iq = engine.upload(iq)
    d_out = engine.upload(np.full((C * stride + tail, 2), sentinel, dtype=np.int32))
    plan.run(R, d_iq, n, words, d_out, out_stride=stride)
    engine.sync()
    out = engine.download(d_out, np.int32, (C * stride + tail, 2))
    want = ddc_ref.ddc_ref(iq, R, words)
    body = out[:C * stride].reshape(C, stride, 2)
    assert np.array_equal(body[:, :n], want)
    assert np.all(body[:, n:] == sentinel) and np.all(out[C * stride:] == sentinel)
    # no samples: nothing happens; with a device the refusals still hold
    assert plan.run(R, d_iq, 0, words, d_out, out_stride=0) == 0
    assert plan.run(R, d_iq, n, words, d_out, out_stride=n - 1, check=False) == -1 and "out_stride" in built.ddc_last_error()
    assert plan.run(R, d_iq, n, [P // 2], d_out, check=False) == -1 and "tuning word" in built.ddc_last_error()
    assert plan.run(R, d_iq, n, words, d_out, first_dec_index=-1, check=False) == -1
    engine.sync()
    assert np.array_equal(engine.download(d_out, np.int32, (C * stride + tail, 2)), out)
    plan.close()
    d_iq.free(), d_out.free()


def test_capture_and_replay(built, tile):
    """A run is one kernel launch: captured on a side stream the way tests/test_fm_gpu.py captures the FM chain,
    replayed twice, identical to an eager launch and to the restatement."""
    import torch
    dev = torch.device("cuda", 0)
    eng = built.Engine(0)
    plan = built.DdcPlan.open(eng)
    R, C, n = 8, 8, tile + 5
    words = words_for(C, seed=8)
    iq_host = ddc_ref.random_iq(n * R, seed=9)
    iq = torch.from_numpy(iq_host).to(dev)
    out = torch.zeros((C, n, 2), dtype=torch.int32, device=dev)

    def launch(o):
        plan.run(R, iq.data_ptr(), n, words, o.data_ptr(), first_dec_index=77, stream=built.torch_stream_handle())

    g = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        with torch.cuda.graph(g, stream=side):
            launch(out)
    torch.cuda.current_stream().wait_stream(side)
    assert int(out.abs().sum()) == 0                     # capture enqueued nothing
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
    assert np.array_equal(out.cpu().numpy(), ddc_ref.ddc_ref(iq_host, R, words, 77))
    plan.close()
    eng.close()


def fm_capture(n, k0, k2, seed):
    """A u8 capture: an FM-modulated carrier at word k0 (a 1 kHz tone, 300 Hz of deviation at 2.4 MS/s: modulation
    index 0.3, the carrier line dominates), a second, plain carrier at word k2, and a little seeded noise."""
    fs = 2.4e6
    i = np.arange(n, dtype=np.float64)
    ph = 2 * np.pi * ((k0 * np.arange(n, dtype=np.int64)) % P) / P + 0.3 * np.sin(2 * np.pi * 1000.0 * i / fs)
    ph2 = 2 * np.pi * ((k2 * np.arange(n, dtype=np.int64)) % P) / P
    z = 60.0 * np.exp(1j * ph) + 30.0 * np.exp(1j * ph2)
    noise = np.random.default_rng(seed).integers(-3, 4, size=(n, 2))
    iq = np.rint(np.stack([z.real, z.imag], axis=1)) + noise + 128
    return np.clip(iq, 0, 255).astype(np.uint8)


def test_composition_with_the_fm_chain_and_the_spectra(engine, oracle):
    """The bank's streams are what rtlws_fm_audio_blocks and RTLWS_IN_CS32 spectra consume.

    Audio: channel 0 of an R = 12, C = 2 bank through Engine.fm_audio_blocks equals the oracle's chain over
    ddc_ref's output, bit for bit.
    Spectrum: a channel tuned 8 bins of the decimated N-point frame below the carrier shows it in slot N/2 + 8.  The
    offset is 8 P / (N R) words -- an integer at R = 8 (64 words at N = 1024) but at no N when R = 12 (P / 12 is no
    integer): there the nearest word, 43, puts the carrier at bin 8.06 and the maximum in the same slot.  Both are
    checked, on the device's rows and on the oracle's rows of ddc_ref's stream."""
    k0, k2 = 5000, -9000
    N, L, nb = 1024, 1024, 2
    for R, off in ((12, 43), (8, 64)):
        assert abs(off - 8 * P / (N * R)) < 0.5
        n = L * nb
        iq = fm_capture(n * R, k0, k2, seed=R)
        words = [k0, k0 - off]
        got = engine.ddc(iq, R, words)
        want = ddc_ref.ddc_ref(iq, R, words)
        assert np.array_equal(got, want)
        if R == 12:
            st = fm_ref.random_state(6)
            audio, st_out = engine.fm_audio_blocks(got[0], L, st)
            want_audio, want_st = fm_ref.oracle_chain(oracle, want[0], L, st)
            assert audio.size == nb * (L // 4) and np.any(audio != 0)
            assert np.array_equal(audio, want_audio) and np.array_equal(st_out, want_st)
        rows = engine.spectra(got[1], N, input="cs32", f64=True)
        assert rows.shape == (nb, N)
        for r in range(nb):
            ps = np.zeros(N)
            assert oracle.spectrum_add_cmplx_s32(N, want[1][r * N:(r + 1) * N], ps) == 0
            assert int(np.argmax(ps)) == N // 2 + 8, (R, r, int(np.argmax(ps)))
            assert int(np.argmax(rows[r])) == N // 2 + 8, (R, r, int(np.argmax(rows[r])))

"""GPU suite of include/rtlws_ddcfir.h: the down-converter bank with an int16 FIR as the channel filter (one launch
for all channels) against the numpy restatement tests/ddcfir_ref.py.  Every comparison is np.array_equal: each
output integer is defined.  Engine.ddcfir uploads a capture of exactly rtlws_ddcfir_samples_needed samples, so every
run here is also a run against the end of its allocation."""
import numpy as np
import pytest

import ddc_family_channels as channels
import ddc_ref
import ddcfir_ref as ref
import fm_ref

pytestmark = pytest.mark.gpu

P = ref.P
SPECIAL_WORDS = (0, 1, -1, 777, -20001, 32767, -32768)
FIRST = 123456789
SENTINEL = np.int32(-0x12345678)
R_AXIS, l_axis, aligned = ref.R_AXIS, ref.l_axis, ref.aligned          # shared with tests/fmfir_ref.py's stage-A matrix
C_AXIS = (1, 2, 7, 8, 9, 32)
S_AXIS = (0, 14, 30)
BYTES = ("random", "full scale", "all 0", "all 255")
TAPS = ("random", "+max", "-max")


def matrix():
    """(R, L, C, s, first, bytes, taps): every (R, L) of the axes, the other axes cycled over them with strides that
    share no factor with their lengths, the extremes together in front."""
    cases = [(16, 256, 32, 0, FIRST, "full scale", "+max"), (128, 256, 32, 0, FIRST, "full scale", "-max"),
             (3, 256, 32, 0, FIRST, "full scale", "-max"), (17, 255, 32, 0, FIRST, "full scale", "+max")]
    i = 0
    for R in R_AXIS:
        for L in l_axis(R):
            cases.append((R, L, C_AXIS[i % 6], S_AXIS[(i // 2) % 3], (0, FIRST)[i % 2], BYTES[(i // 3) % 4], TAPS[(i // 5) % 3]))
            i += 1
    return cases


MATRIX = matrix()


def test_the_matrix_covers_every_axis_with_every_instantiation():
    for inst in (True, False):
        mine = [c for c in MATRIX if aligned(c[0], c[1]) == inst]
        assert {c[0] for c in mine} == {R for R in R_AXIS if any(aligned(R, L) == inst for L in l_axis(R))}
        assert {c[0] for c in mine} >= ({8, 12, 16, 128} if inst else set(R_AXIS))
        for R in R_AXIS:
            assert {c[1] for c in mine if c[0] == R} == {L for L in l_axis(R) if aligned(R, L) == inst}
        assert {c[2] for c in mine} == set(C_AXIS) and {c[3] for c in mine} == set(S_AXIS)
        assert {c[4] for c in mine} == {0, FIRST} and {c[5] for c in mine} == set(BYTES) and {c[6] for c in mine} == set(TAPS)


@pytest.fixture(scope="module")
def tile(built):
    rc, _, _, _, t = built.ddcfir_grid(8, 8, 1, 1)
    assert rc == 0 and t >= 32
    return t


def dec_lens(t):
    return (1, 15, 16, 17, 127, t - 1, t, t + 1, 2 * t + 5)


def words_for(C, seed):
    """C tuning words: the special ones from position seed on, as many as fit beside one seeded random word."""
    w = [int(k) for k in np.random.default_rng(seed).integers(-P // 2, P // 2, C)]
    for i in range(min(C - 1, len(SPECIAL_WORDS)) if C > 1 else 1):
        w[(1 + i) % C] = SPECIAL_WORDS[(seed + i) % len(SPECIAL_WORDS)]
    return w


def make_iq(kind, n, seed):
    if kind == "random":
        return ref.random_iq(n, seed)
    if kind == "full scale":
        return ref.full_scale_iq(n, seed)
    return np.full((n, 2), 0 if kind == "all 0" else 255, dtype=np.uint8)


def make_taps(kind, L, seed):
    if kind == "random":
        return ref.random_taps(L, seed)
    return np.full(L, ref.MAX_TAP if kind == "+max" else -ref.MAX_TAP, dtype=np.int16)


@pytest.mark.parametrize("case", range(len(MATRIX)), ids=["R%d-L%d-C%d-s%d" % c[:4] for c in MATRIX])
def test_bank_matrix(engine, tile, case):
    R, L, C, s, first, bytes_kind, taps_kind = MATRIX[case]
    words = words_for(C, seed=case)
    if C >= 8:
        assert set(SPECIAL_WORDS) <= set(words)
    taps = make_taps(taps_kind, L, seed=case)
    lens = dec_lens(tile)
    iq = make_iq(bytes_kind, ref.samples_needed(R, L, lens[-1]), seed=1000 + case)
    want = ref.ddcfir_ref(iq, R, taps, words, s, first)      # a shorter run is a prefix: the same absolute indices
    for n in lens:
        got = engine.ddcfir(iq, R, taps, words, out_shift=s, first_dec_index=first, dec_len=n)
        assert got.shape == (C, n, 2)
        bad = np.argwhere(got != want[:, :n])
        assert bad.size == 0, (n, bad[:4], got[tuple(bad[0])], want[tuple(bad[0])])
    mid = np.full_like(iq, 128)
    assert not engine.ddcfir(mid, R, taps, words, out_shift=s, first_dec_index=first).any()


@pytest.mark.parametrize("path", channels.paths("ddcfir"), ids=channels.path_id)
def test_every_channel_count(engine, built, tile, path):
    """tests/ddc_family_channels.py: C = 1 .. 32 of one set of 32 words over one capture of exactly samples_needed,
    tile + 17 decimated samples, at the three load forms of a window (bank_tile<ALIGNED, 1 .. 4> each); ntaps = 1 and 256
    at both sides of the third column tile's borders (48 KiB of dynamic LDS at 256 taps and three column tiles).
    Every launch goes through the plan's run into 32 rows of out_stride > dec_len and a tail, all sentinels: rows
    0 .. C - 1 are the first C of the 32-channel restatement, every other word is untouched."""
    R, L = path
    n = channels.stream_len(tile)
    stride, tail = n + 7, 64
    rows = channels.MAX_CH
    want = channels.stream_expected("ddcfir", path, tile)
    fill = np.full((rows * stride + tail, 2), SENTINEL, dtype=np.int32)
    iq = channels.stream_inputs("ddcfir", path, tile)
    assert iq.shape[0] == built.ddcfir_samples_needed(R, L, n)
    plan = built.DdcFirPlan.open(engine, R, channels.taps_of(path))
    d_iq = engine.upload(iq)
    for C in channels.channels("ddcfir", path):
        rc, blocks, _, lds, t = built.ddcfir_grid(R, L, C, n)
        assert rc == 0 and t == tile and blocks == -(-n // tile) * 1 and lds == -(-C // 8) * -(-L // 16) * 1024
        d_out = engine.upload(fill)
        plan.run(d_iq, n, channels.WORDS[:C], d_out, out_shift=14, out_stride=stride, first_dec_index=channels.FIRST)
        engine.sync()
        out = engine.download(d_out, np.int32, fill.shape)
        d_out.free()
        body = out[:rows * stride].reshape(rows, stride, 2)
        bad = np.argwhere(body[:C, :n] != want[:C])
        assert bad.size == 0, (C, len(bad), bad[:4])
        assert np.all(body[:C, n:] == SENTINEL) and np.all(body[C:] == SENTINEL) and np.all(out[rows * stride:] == SENTINEL), C
    plan.close()
    d_iq.free()


@pytest.mark.parametrize("R", [8, 10, 12, 7])
def test_boxcar_is_the_unfiltered_bank(engine, tile, R):
    """L = R, h = 16384 throughout, s = 14: rtlws_ddc_run's output on the device, bit for bit."""
    n = 2 * tile + 5
    words = words_for(9, seed=R)
    iq = ref.random_iq(n * R, seed=R)
    got = engine.ddcfir(iq, R, ref.boxcar(R), words, out_shift=14, first_dec_index=FIRST)
    assert got.shape == (9, n, 2)
    assert np.array_equal(got, engine.ddc(iq, R, words, first_dec_index=FIRST))


def test_stride_and_nothing_outside_the_streams(engine, built, tile):
    """Sentinels around every channel's range, out_stride > dec_len, the capture allocated at exactly samples_needed."""
    R, L, C = 12, 96, 9
    n = tile + 1
    stride, tail = n + 7, 64
    words = words_for(C, seed=3)
    taps = built.ddcfir_design(R, L)
    need = built.ddcfir_samples_needed(R, L, n)
    assert need == (n - 1) * R + L
    iq = ref.random_iq(need, seed=4)
    sentinel = np.int32(-0x12345678)
    plan = built.DdcFirPlan.open(engine, R, taps)
    d_iq = engine.upload(iq)
    d_out = engine.upload(np.full((C * stride + tail, 2), sentinel, dtype=np.int32))
    plan.run(d_iq, n, words, d_out, out_shift=14, out_stride=stride)
    engine.sync()
    out = engine.download(d_out, np.int32, (C * stride + tail, 2))
    want = ref.ddcfir_ref(iq, R, taps, words, 14)
    body = out[:C * stride].reshape(C, stride, 2)
    assert np.array_equal(body[:, :n], want)
    assert np.all(body[:, n:] == sentinel) and np.all(out[C * stride:] == sentinel)
    # no samples: nothing happens; with a device the refusals still hold
    assert plan.run(d_iq, 0, words, d_out, out_stride=0) == 0
    assert plan.run(d_iq, n, words, d_out, out_stride=n - 1, check=False) == -1 and "out_stride" in built.ddcfir_last_error()
    assert plan.run(d_iq, n, [P // 2], d_out, check=False) == -1 and "tuning word" in built.ddcfir_last_error()
    assert plan.run(d_iq, n, words, d_out, out_shift=31, check=False) == -1 and "out_shift" in built.ddcfir_last_error()
    assert plan.run(d_iq, n, words, d_out, first_dec_index=-1, check=False) == -1
    engine.sync()
    assert np.array_equal(engine.download(d_out, np.int32, (C * stride + tail, 2)), out)
    plan.close()
    d_iq.free(), d_out.free()


@pytest.mark.parametrize("R,L,first", [(10, 80, 0), (12, 96, (1 << 40) + 12345), (16, 7, FIRST)])
def test_chunks_concatenate_to_one_run(engine, tile, R, L, first):
    """Two calls that overlap by L - R samples (L < R: R - L samples between them are skipped) and pass the index."""
    words = [777, -20001, 32767]
    taps = ref.random_taps(L, seed=L)
    n, cut = 2 * tile + 5, tile + 3
    iq = ref.random_iq(ref.samples_needed(R, L, n), seed=5)
    whole = engine.ddcfir(iq, R, taps, words, out_shift=9, first_dec_index=first)
    assert np.array_equal(whole, ref.ddcfir_ref(iq, R, taps, words, 9, first))
    head = engine.ddcfir(iq[:ref.samples_needed(R, L, cut)], R, taps, words, out_shift=9, first_dec_index=first)
    rest = engine.ddcfir(iq[cut * R:], R, taps, words, out_shift=9, first_dec_index=first + cut)
    assert head.shape[1] == cut and rest.shape[1] == n - cut
    assert np.array_equal(np.concatenate([head, rest], axis=1), whole)
    assert not np.array_equal(engine.ddcfir(iq[cut * R:], R, taps, words, out_shift=9, first_dec_index=first), rest)


def test_a_retune_is_the_next_call(engine, built, tile):
    R, L, n = 8, 64, tile + 9
    taps = built.ddcfir_design(R, L)
    iq = ref.random_iq(ref.samples_needed(R, L, n), seed=6)
    plan = built.DdcFirPlan.open(engine, R, taps)
    d_iq = engine.upload(iq)
    d_out = engine.alloc(3 * n * 8)
    for words in ([100, 200, 300], [-5000, 100], [32767]):
        plan.run(d_iq, n, words, d_out, out_shift=14)
        engine.sync()
        got = engine.download(d_out, np.int32, (len(words), n, 2))
        assert np.array_equal(got, ref.ddcfir_ref(iq, R, taps, words, 14))
    plan.close()
    d_iq.free(), d_out.free()


def test_capture_and_replay(built, tile):
    """A run is one kernel launch: captured on a side stream the way tests/test_ddc_gpu.py captures the unfiltered
    bank, replayed twice, identical to an eager launch and to the restatement."""
    import torch
    dev = torch.device("cuda", 0)
    eng = built.Engine(0)
    R, L, C, n = 12, 96, 8, tile + 5
    taps = built.ddcfir_design(R, L)
    plan = built.DdcFirPlan.open(eng, R, taps)
    words = words_for(C, seed=8)
    iq_host = ref.random_iq(ref.samples_needed(R, L, n), seed=9)
    iq = torch.from_numpy(iq_host).to(dev)
    out = torch.zeros((C, n, 2), dtype=torch.int32, device=dev)

    def launch(o):
        plan.run(iq.data_ptr(), n, words, o.data_ptr(), out_shift=14, first_dec_index=77, stream=built.torch_stream_handle())

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
    assert np.array_equal(out.cpu().numpy(), ref.ddcfir_ref(iq_host, R, taps, words, 14, 77))
    plan.close()
    eng.close()


def test_the_stream_argument(built, tile):
    """NULL is the engine's own stream, RTLWS_STREAM_DEFAULT HIP's, anything else the caller's."""
    import torch
    dev = torch.device("cuda", 0)
    eng = built.Engine(0)
    R, L, n = 10, 33, tile + 2
    taps = ref.random_taps(L, seed=10)
    words = [777, -1]
    iq_host = ref.random_iq(ref.samples_needed(R, L, n), seed=11)
    want = ref.ddcfir_ref(iq_host, R, taps, words, 5)
    plan = built.DdcFirPlan.open(eng, R, taps)
    iq = torch.from_numpy(iq_host).to(dev)
    torch.cuda.synchronize()
    own = torch.cuda.Stream()
    for stream, wait in ((built.STREAM_ENGINE, eng.sync), (built.torch_stream_handle(own), own.synchronize),
                         (built.STREAM_DEFAULT, torch.cuda.synchronize)):
        out = torch.zeros((2, n, 2), dtype=torch.int32, device=dev)
        torch.cuda.synchronize()
        plan.run(iq.data_ptr(), n, words, out.data_ptr(), out_shift=5, stream=stream)
        wait()
        assert np.array_equal(out.cpu().numpy(), want), stream
    plan.close()
    eng.close()


def test_selectivity_through_the_device(engine, built):
    """The restatement's figures (tests/test_ddcfir_cpu.py), because the integers are equal."""
    run = lambda iq, R, taps, words, s: engine.ddcfir(iq, R, taps, words, out_shift=s)
    for taps in (built.ddcfir_design(12, 96), ref.boxcar(12)):
        assert ref.selectivity_db(run, taps) == ref.selectivity_db(ref.ddcfir_ref, taps)
    assert ref.selectivity_db(run, built.ddcfir_design(12, 96)) <= -40.0
    assert ref.selectivity_db(run, ref.boxcar(12)) >= -15.0


def test_chain_into_the_fm_demodulator(engine, built, oracle):
    """The designed filter at s = 14 feeds rtlws_fm_audio_blocks at the CIC's gain: the audio of the device's stream is
    the oracle's chain over the restatement's integers, bit for bit."""
    from test_ddc_gpu import fm_capture
    R, L, block, nb = 12, 96, 1024, 2
    taps = built.ddcfir_design(R, L)
    n = block * nb
    iq = fm_capture(ref.samples_needed(R, L, n), 5000, -9000, seed=12)
    got = engine.ddcfir(iq, R, taps, [5000], out_shift=14)
    want = ref.ddcfir_ref(iq, R, taps, [5000], 14)
    assert np.array_equal(got, want)
    st = fm_ref.random_state(6)
    audio, st_out = engine.fm_audio_blocks(got[0], block, st)
    want_audio, want_st = fm_ref.oracle_chain(oracle, want[0], block, st)
    assert audio.size == nb * (block // 4) and np.any(audio != 0)
    assert np.array_equal(audio, want_audio) and np.array_equal(st_out, want_st)

"""GPU suite of include/rtlws_fmfir.h: up to 32 FM stations from one capture behind an int16 FIR in one launch,
against tests/ddcfir_ref.py per channel fed to the oracle's per-block chain (tests/fmfir_ref.py).  Every comparison is
np.array_equal, on audio and on state."""
import numpy as np
import pytest

import ddc_family_channels as channels
import ddcfir_ref
import fm_ref
import fmbank_ref
import fmfir_ref
from test_fmbank_gpu import SENTINEL, check_rows

pytestmark = pytest.mark.gpu

P = ddcfir_ref.P
STATE = fm_ref.STATE


@pytest.fixture(scope="module")
def tile(built):
    rc, _, _, _, t = built.fmfir_grid(8, 8, 1, 20, 1)
    assert rc == 0 and t >= 16
    return t


def check(got, want, what):
    audio, st = got
    want_audio, want_st = want
    assert audio.shape == want_audio.shape and st.shape == want_st.shape, what
    bad = np.argwhere(audio != want_audio)
    assert bad.size == 0, (what, "audio", len(bad), bad[:4])
    bad = np.argwhere(st != want_st)
    assert bad.size == 0, (what, "state", bad[:8])


@pytest.mark.parametrize("R,L,C,designed", fmfir_ref.BANKS)
def test_bank_matrix(engine, oracle, built, tile, R, L, C, designed):
    bl, nb = fmbank_ref.matrix_shape(tile)
    rc, blocks, _, _, _ = built.fmfir_grid(R, L, C, bl, nb)
    assert rc == 0 and blocks == (3 + 1) * -(-C // 8)
    taps = fmfir_ref.taps_for(R, L, seed=R + L, designed=designed)
    assert designed or L < 2 or {ddcfir_ref.MAX_TAP, -ddcfir_ref.MAX_TAP} <= set(int(h) for h in taps)
    iq, words, states = fmfir_ref.inputs(R, L, C, bl, nb, seed=1000 * R + 10 * L + C)
    assert iq.shape[0] == built.fmfir_samples_needed(R, L, bl, nb)
    if C >= 8:
        assert set(fmbank_ref.SPECIAL_WORDS) <= set(words)
    want = fmfir_ref.expected(oracle, iq, R, taps, words, bl, states)
    got = engine.fm_fir_bank(iq, R, taps, words, bl, states)
    check(got, want, (R, L, C))
    assert np.any(got[0] != 0)
    if C >= 2:
        assert np.array_equal(got[0][0], got[0][C - 1]) and np.array_equal(got[1][0], got[1][C - 1])
    if C >= 3:
        assert not np.array_equal(got[0][0], got[0][1])


@pytest.mark.parametrize("path", channels.paths("fmfir"), ids=channels.path_id)
def test_every_channel_count(engine, oracle, built, tile, path):
    """tests/ddc_family_channels.py: C = 1 .. 32 of one set of 32 words and 32 carried states over one capture of exactly
    samples_needed, two full tiles and a remainder, at the three load forms of a window: 4 ceil(C / 8) workgroups, so
    that with three column tiles blockIdx.x = 0 .. 11 passes through the division by nct and meets every (tile, column
    tile).  Every launch goes through the plan's run into 32 audio rows of audio_stride > the run's length and 32 x 21
    floats of state_out, each with a tail, all sentinels (tests/test_fmbank_gpu.py's check_rows)."""
    R, L = path
    iq, bl, nb = channels.fm_inputs("fmfir", path, tile)
    assert iq.shape[0] == built.fmfir_samples_needed(R, L, bl, nb)
    n = nb * (bl // 4)
    ntiles = -(-n // tile)
    stride, tail = n + 7, 64
    rows = channels.MAX_CH
    want = channels.fm_expected(oracle, "fmfir", path, tile)
    fill_audio = np.full(rows * stride + tail, SENTINEL, dtype=np.float32)
    fill_st = np.full(rows * STATE + tail, SENTINEL, dtype=np.float32)
    plan = built.FmFirPlan.open(engine, R, channels.taps_of(path))
    d_iq = engine.upload(iq)
    d_in = engine.upload(channels.states())
    for C in channels.channels("fmfir", path):
        rc, blocks, _, _, t = built.fmfir_grid(R, L, C, bl, nb)
        assert rc == 0 and t == tile and ntiles == 3 and blocks == (ntiles + 1) * -(-C // 8)
        d_out, d_audio = engine.upload(fill_st), engine.upload(fill_audio)
        plan.run(d_iq, bl, nb, channels.WORDS[:C], d_in, d_out, d_audio, audio_stride=stride)
        engine.sync()
        audio = engine.download(d_audio, np.float32, fill_audio.shape)
        st = engine.download(d_out, np.float32, fill_st.shape)
        d_out.free(), d_audio.free()
        check_rows(audio, st, want, C, n, stride, (path, C))
    assert np.array_equal(engine.download(d_in, np.float32, (rows, STATE)), channels.states())
    plan.close()
    d_iq.free(), d_in.free()


@pytest.mark.parametrize("shift", [0, 30])
def test_shifts(engine, oracle, tile, shift):
    """Both ends of out_shift: at 30 most integers are 0, the atan2(0, 0) branch."""
    R, L, C = 8, 40, 9
    bl, nb = fmbank_ref.matrix_shape(tile)
    taps = fmfir_ref.taps_for(R, L, seed=shift)
    iq, words, states = fmfir_ref.inputs(R, L, C, bl, nb, seed=300 + shift)
    if shift == 30:
        streams = ddcfir_ref.ddcfir_ref(iq, R, taps, words, shift)
        assert np.mean(streams == 0) > 0.5 and np.any(np.all(streams == 0, axis=2))
    check(engine.fm_fir_bank(iq, R, taps, words, bl, states, out_shift=shift),
          fmfir_ref.expected(oracle, iq, R, taps, words, bl, states, shift), shift)


STAGE_A_PAIRS = fmfir_ref.stage_a_pairs()


def _stage_a_run(engine, case, seed):
    iq, taps, words, states = fmfir_ref.stage_a_inputs(case, seed)
    got = engine.fm_fir_bank(iq, case.R, taps, words, case.block_len, states, out_shift=case.shift, first_dec_index=case.first)
    return (iq, taps, words, states), got


@pytest.mark.parametrize("index", range(len(STAGE_A_PAIRS)), ids=["R%d-L%d" % p for p in STAGE_A_PAIRS])
def test_stage_a_at_every_window_form(engine, oracle, built, tile, index):
    """fmfir_ref.stage_a_matrix: phases<ALIGNED> at every (decim, ntaps) of the filtered down-converter's matrix, the
    channel counts, out_shift, first_dec_index, byte kinds, tap kinds and block shapes cycled over them
    (tests/test_fmfir_cpu.py holds the matrix to its conditions: every np mod 32 class of the last pair of row tiles,
    1, 2 and 16 K steps, every ntaps mod 16, per instantiation)."""
    case = fmfir_ref.stage_a_matrix(tile)[index]
    assert (case.R, case.L) == STAGE_A_PAIRS[index]
    (iq, taps, words, states), got = _stage_a_run(engine, case, seed=5000 + index)
    assert iq.shape[0] == built.fmfir_samples_needed(case.R, case.L, case.block_len, case.nblocks)
    want = fmfir_ref.expected(oracle, iq, case.R, taps, words, case.block_len, states, case.shift, case.first)
    check(got, want, case.id)
    assert np.any(got[0] != 0)


@pytest.mark.parametrize("which", [0, 1], ids=["aligned", "generic"])
def test_stage_a_device_composition(engine, tile, which):
    """Once per instantiation, a case of the stage-A matrix with several tiles and column tiles: Engine.ddcfir followed
    by Engine.fm_audio_blocks per channel, on the device, equals the fused launch (test_device_composition's form)."""
    index = fmfir_ref.composition_cases(tile)[which]
    case = fmfir_ref.stage_a_matrix(tile)[index]
    assert case.aligned == (which == 0)
    (iq, taps, words, states), (audio, st) = _stage_a_run(engine, case, seed=5000 + index)
    streams = engine.ddcfir(iq, case.R, taps, words, out_shift=case.shift, first_dec_index=case.first)
    assert streams.shape == (case.C, case.nblocks * case.block_len, 2)
    for c in range(case.C):
        want_audio, want_st = engine.fm_audio_blocks(streams[c], case.block_len, states[c])
        assert np.array_equal(audio[c], want_audio) and np.array_equal(st[c], want_st), (case.id, c)
    assert np.any(audio != 0)


@pytest.mark.parametrize("R", [8, 10, 7])
def test_boxcar_is_the_unfiltered_bank(engine, oracle, tile, R):
    """L = R, every tap 16384, s = 14: rtlws_fmbank_run bit for bit, on the device and on the restatement."""
    C = 9
    bl, nb = fmbank_ref.matrix_shape(tile)
    iq, words, states = fmfir_ref.inputs(R, R, C, bl, nb, seed=70 + R)
    assert iq.shape[0] == nb * bl * R
    got = engine.fm_fir_bank(iq, R, ddcfir_ref.boxcar(R), words, bl, states, out_shift=14)
    check(got, engine.fm_bank(iq, R, words, bl, states), ("device", R))
    check(got, fmbank_ref.expected(oracle, iq, R, words, bl, states), ("restatement", R))


@pytest.mark.parametrize("nb", [1, 3])
@pytest.mark.parametrize("bl", [20, 22, 23, 25])
def test_block_shapes(engine, oracle, bl, nb):
    """The odd-sample and odd-output skips, all inside one tile."""
    R, L, C = fmfir_ref.TILE_BANK
    taps = fmfir_ref.taps_for(R, L, seed=bl)
    iq, words, states = fmfir_ref.inputs(R, L, C, bl, nb, seed=bl + nb)
    check(engine.fm_fir_bank(iq, R, taps, words, bl, states), fmfir_ref.expected(oracle, iq, R, taps, words, bl, states), (bl, nb))


CASES = [(regime, residue) for regime in "abc" for residue in range(4)]
TILE_RUNS = [fmfir_ref.TILE_BANK + c for c in CASES] + [b + c for b in fmfir_ref.SKIP_BANKS for c in CASES if c[1] in (1, 3)]


def _tile_case(built, tile, regime, residue, R, L, C):
    case = {(c.regime, c.residue): c for c in fm_ref.tile_cases(tile)}[regime, residue]
    rc, blocks, _, _, t = built.fmfir_grid(R, L, C, case.block_len, case.nblocks)
    assert rc == 0 and t == tile and case.ntiles(tile) >= 4 and blocks == (case.ntiles(tile) + 1) * -(-C // 8), case.id
    return case


@pytest.mark.parametrize("R,L,C,regime,residue", TILE_RUNS)
def test_tile_cases(engine, oracle, built, tile, R, L, C, regime, residue):
    """Every block_len mod 4 over four tiles or more, from carried states (fm_ref.tile_cases)."""
    case = _tile_case(built, tile, regime, residue, R, L, C)
    taps = fmfir_ref.taps_for(R, L, seed=case.block_len)
    iq, words, states = fmfir_ref.inputs(R, L, C, case.block_len, case.nblocks, seed=1000 * case.block_len + 10 * R + C)
    want = fmfir_ref.expected(oracle, iq, R, taps, words, case.block_len, states, key=("tile case", case, R, L, C))
    got = engine.fm_fir_bank(iq, R, taps, words, case.block_len, states)
    check(got, want, (case.id, R, L, C))
    assert np.any(got[0] != 0)
    assert np.array_equal(got[0][0], got[0][C - 1]) and np.array_equal(got[1][0], got[1][C - 1])      # the same station


@pytest.mark.parametrize("name,L", [("axes", 8), ("all128", 8), ("all128", 40)])
def test_branch_inputs(engine, oracle, name, L):
    """fmbank_ref's branch captures at the boxcar (the word-0 channel hits x == 0 with every sign of y), extended by
    ntaps - decim samples; every byte 128 also behind a 40-tap filter: the oracle's response to zeros."""
    R, C, bl, nb = fmbank_ref.BRANCH_R, fmbank_ref.BRANCH_C, fmbank_ref.BRANCH_L, fmbank_ref.BRANCH_NB
    taps = ddcfir_ref.boxcar(R) if L == R else fmfir_ref.taps_for(R, L, seed=91)
    iq = fmbank_ref.branch_captures()[name]
    if name == "all128":
        iq = np.full((fmfir_ref.samples_needed(R, L, bl, nb), 2), 128, dtype=np.uint8)
    else:
        iq = fmfir_ref.extend(iq, L - R)
    words = fmbank_ref.branch_words()
    states = fmbank_ref.states_for(C, seed=90)
    got = engine.fm_fir_bank(iq, R, taps, words, bl, states)
    check(got, fmfir_ref.expected(oracle, iq, R, taps, words, bl, states), (name, L))
    if name == "all128":
        zeros = np.zeros((nb * bl, 2), dtype=np.int32)
        for c in range(C):
            a, s = fm_ref.oracle_chain(oracle, zeros, bl, states[c])
            assert np.array_equal(got[0][c], a) and np.array_equal(got[1][c], s), c
    else:
        streams = ddcfir_ref.ddcfir_ref(iq, R, taps, words)
        x0 = streams[0, :, 0] == 0
        assert np.any(x0 & (streams[0, :, 1] > 0)) and np.any(x0 & (streams[0, :, 1] < 0)) and np.any(x0 & (streams[0, :, 1] == 0))


def _run_chunks(engine, built, plan, iq, R, L, words, bl, states, first, cuts, shift=14):
    """Calls cut at the block indices `cuts`, each on an upload of exactly its samples_needed from sample
    a * bl * R on, swapping two state buffers -> (audio [C, n], final states)."""
    C, nb, quarter = len(words), cuts[-1], bl // 4
    n = nb * quarter
    d_st = [engine.upload(states), engine.alloc(states.nbytes)]
    d_audio = engine.alloc(C * n * 4)
    bufs = []
    for a, b in zip(cuts, cuts[1:]):
        need = built.fmfir_samples_needed(R, L, bl, b - a)
        start = a * bl * R
        assert need == fmfir_ref.samples_needed(R, L, bl, b - a) and start + need <= iq.shape[0]
        d_iq = engine.upload(np.ascontiguousarray(iq[start:start + need]))
        bufs.append(d_iq)
        plan.run(d_iq, bl, b - a, words, d_st[0], d_st[1], d_audio.ptr + a * quarter * 4, out_shift=shift, audio_stride=n,
                 first_dec_index=first + a * bl)
        d_st.reverse()
    engine.sync()
    audio = engine.download(d_audio, np.float32, (C, n))
    st = engine.download(d_st[0], np.float32, (C, STATE))
    for b in (d_audio, *d_st, *bufs):
        b.free()
    return audio, st


@pytest.mark.parametrize("first", [0, (1 << 40) + 12345])
def test_chunks_concatenate_to_one_run(engine, oracle, built, tile, first):
    """Both maps skipping, quarter = tile - 2: calls cut behind blocks 1 and 4 (odd counts, borders in front of tiles),
    neighbouring captures overlapping by ntaps - decim samples, equal the one call and the expected values."""
    R, L, C = fmfir_ref.TILE_BANK
    case = _tile_case(built, tile, "b", 3, R, L, C)
    bl, cuts = case.block_len, (0, 1, 4)
    assert bl % 2 == 1 and cuts[-1] == case.nblocks and L > R
    taps = fmfir_ref.taps_for(R, L, seed=bl)
    iq, words, states = fmfir_ref.inputs(R, L, C, bl, case.nblocks, seed=77)
    want = fmfir_ref.expected(oracle, iq, R, taps, words, bl, states, first=first)
    whole = engine.fm_fir_bank(iq, R, taps, words, bl, states, first_dec_index=first)
    check(whole, want, "one call")
    plan = built.FmFirPlan.open(engine, R, taps)
    chunks = _run_chunks(engine, built, plan, iq, R, L, words, bl, states, first, cuts)
    plan.close()
    check(chunks, whole, cuts)
    if first:
        assert not np.array_equal(whole[0], engine.fm_fir_bank(iq, R, taps, words, bl, states)[0])   # the index is in the phase


def test_stride_and_nothing_outside_the_ranges(engine, oracle, built, tile):
    R, L, C, bl, nb = 12, 36, 9, tile + 6, 5
    n = nb * (bl // 4)
    stride, tail = n + 7, 64
    taps = fmfir_ref.taps_for(R, L, seed=2)
    iq, words, states = fmfir_ref.inputs(R, L, C, bl, nb, seed=3)
    need = iq.shape[0]
    want_audio, want_st = fmfir_ref.expected(oracle, iq, R, taps, words, bl, states)
    sentinel = np.float32(-12345.678)
    plan = built.FmFirPlan.open(engine, R, taps)
    results = []
    for fill in (0, 255):                                # what lies behind samples_needed is not read
        d_iq = engine.upload(np.concatenate([iq, np.full((4096, 2), fill, dtype=np.uint8)]))
        d_in = engine.upload(states)
        d_out = engine.upload(np.full(C * STATE + tail, sentinel, dtype=np.float32))
        d_audio = engine.upload(np.full(C * stride + tail, sentinel, dtype=np.float32))
        plan.run(d_iq, bl, nb, words, d_in, d_out, d_audio, audio_stride=stride)
        engine.sync()
        audio = engine.download(d_audio, np.float32, (C * stride + tail,))
        st = engine.download(d_out, np.float32, (C * STATE + tail,))
        results.append((audio, st))
        body = audio[:C * stride].reshape(C, stride)
        assert np.array_equal(body[:, :n], want_audio), fill
        assert np.all(body[:, n:] == sentinel) and np.all(audio[C * stride:] == sentinel)
        assert np.array_equal(st[:C * STATE].reshape(C, STATE), want_st) and np.all(st[C * STATE:] == sentinel)
        assert np.array_equal(engine.download(d_in, np.float32, (C, STATE)), states)
        if fill == 0:
            for b in (d_iq, d_in, d_out, d_audio):
                b.free()
    assert need == built.fmfir_samples_needed(R, L, bl, nb)
    assert np.array_equal(results[0][0], results[1][0]) and np.array_equal(results[0][1], results[1][1])

    # with a device the refusals still hold and leave the buffers untouched
    err = built.fmfir_last_error
    audio, st = results[1]
    assert plan.run(d_iq, bl, nb, words, d_in, d_out, d_audio, audio_stride=n - 1, check=False) == -1 and "audio_stride" in err()
    assert plan.run(d_iq, bl, nb, [P // 2], d_in, d_out, d_audio, audio_stride=stride, check=False) == -1 and "tuning word" in err()
    assert plan.run(d_iq, bl, nb, words, d_in, d_out, d_audio, out_shift=31, audio_stride=stride, check=False) == -1 and "out_shift" in err()
    assert plan.run(d_iq, bl, nb, words, d_in, d_in.ptr + 4, d_audio, audio_stride=stride, check=False) == -1 and "overlap" in err()
    assert plan.run(d_iq, 19, nb, words, d_in, d_out, d_audio, audio_stride=stride, check=False) == -1 and "block_len" in err()
    engine.sync()
    assert np.array_equal(engine.download(d_audio, np.float32, (C * stride + tail,)), audio)
    assert np.array_equal(engine.download(d_out, np.float32, (C * STATE + tail,)), st)

    # no blocks: the states are copied, nothing else is written
    d_out2 = engine.upload(np.full(C * STATE + tail, sentinel, dtype=np.float32))
    assert plan.run(None, bl, 0, words, d_in, d_out2, None, audio_stride=0) == 0
    engine.sync()
    st2 = engine.download(d_out2, np.float32, (C * STATE + tail,))
    assert np.array_equal(st2[:C * STATE].reshape(C, STATE), states) and np.all(st2[C * STATE:] == sentinel)
    assert np.array_equal(engine.download(d_audio, np.float32, (C * stride + tail,)), audio)
    plan.close()
    for b in (d_iq, d_in, d_out, d_out2, d_audio):
        b.free()


def test_device_composition(engine):
    """Engine.fm_fir_bank equals Engine.ddcfir followed by Engine.fm_audio_blocks per channel: the definition of
    include/rtlws_fmfir.h, on the device."""
    R, L, C, bl, nb = 12, 96, 2, 518, 3
    words = [5000, -9000]
    first, shift = 4242, 13
    taps = ddcfir_ref.design(R, L)
    iq = ddcfir_ref.random_iq(fmfir_ref.samples_needed(R, L, bl, nb), seed=12)
    states = fmbank_ref.states_for(C, seed=13)
    audio, st = engine.fm_fir_bank(iq, R, taps, words, bl, states, out_shift=shift, first_dec_index=first)
    streams = engine.ddcfir(iq, R, taps, words, out_shift=shift, first_dec_index=first)
    assert streams.shape[1] == nb * bl
    for c in range(C):
        want_audio, want_st = engine.fm_audio_blocks(streams[c], bl, states[c])
        assert np.array_equal(audio[c], want_audio) and np.array_equal(st[c], want_st), c
    assert np.any(audio != 0)


def test_capture_and_replay(built, oracle, tile):
    """A run is one kernel launch: two runs, the second over the next blocks with the state buffers swapped, each
    captured into a graph of its own on a side stream; replayed in turn twice they give the expected values of the one
    call, as an eager launch does."""
    import torch
    dev = torch.device("cuda", 0)
    eng = built.Engine(0)
    R, L, C, bl = 8, 40, 8, tile + 6
    cuts, first = (0, 1, 3), 77
    nb, quarter = cuts[-1], bl // 4
    n = nb * quarter
    taps = fmfir_ref.taps_for(R, L, seed=8)
    plan = built.FmFirPlan.open(eng, R, taps)
    iq_host, words, states = fmfir_ref.inputs(R, L, C, bl, nb, seed=9)
    assert all((a * bl * R * 2) % 16 == 0 for a in cuts)
    iq = torch.from_numpy(iq_host).to(dev)
    st = [torch.from_numpy(states).to(dev), torch.zeros((C, STATE), dtype=torch.float32, device=dev)]
    audio = torch.zeros((C, n), dtype=torch.float32, device=dev)

    def launch(i, a):
        lo, hi = cuts[i], cuts[i + 1]
        plan.run(iq.data_ptr() + lo * bl * R * 2, bl, hi - lo, words, st[i % 2].data_ptr(), st[(i + 1) % 2].data_ptr(),
                 a.data_ptr() + lo * quarter * 4, audio_stride=n, first_dec_index=first + lo * bl, stream=built.torch_stream_handle())

    graphs = []
    side = torch.cuda.Stream()
    for i in range(2):
        g = torch.cuda.CUDAGraph()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            with torch.cuda.graph(g, stream=side):
                launch(i, audio)
        torch.cuda.current_stream().wait_stream(side)
        graphs.append(g)
    assert float(audio.abs().sum()) == 0 and float(st[1].abs().sum()) == 0       # capture enqueued nothing
    want_audio, want_st = fmfir_ref.expected(oracle, iq_host, R, taps, words, bl, states, first=first)
    for _ in range(2):
        audio.zero_()
        st[1].zero_()
        st[0].copy_(torch.from_numpy(states))
        for g in graphs:
            g.replay()
        torch.cuda.synchronize()
        assert np.array_equal(audio.cpu().numpy(), want_audio) and np.array_equal(st[0].cpu().numpy(), want_st)
    eager = torch.zeros_like(audio)
    st[0].copy_(torch.from_numpy(states))
    for i in range(2):
        launch(i, eager)
    torch.cuda.synchronize()
    assert torch.equal(eager, audio) and np.array_equal(st[0].cpu().numpy(), want_st)
    plan.close()
    eng.close()

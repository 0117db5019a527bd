"""GPU suite of include/rtlws_fmbank.h: up to 32 FM stations from one capture in one launch, against tests/ddc_ref.py
per channel fed to the oracle's per-block chain.  Every comparison is np.array_equal, on audio and on state."""
import numpy as np
import pytest

import ddc_family_channels as channels
import ddc_ref
import fm_ref
import fmbank_ref

pytestmark = pytest.mark.gpu

P = ddc_ref.P
STATE = fm_ref.STATE
SENTINEL = np.float32(-12345.678)


@pytest.fixture(scope="module")
def tile(built):
    rc, _, _, _, t = built.fmbank_grid(8, 1, 20, 1)
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


@pytest.mark.parametrize("R,C", fmbank_ref.BANKS)
def test_bank_matrix(engine, oracle, built, tile, R, C):
    L, nb = fmbank_ref.matrix_shape(tile)
    assert nb * L <= 5150
    rc, blocks, _, _, _ = built.fmbank_grid(R, C, L, nb)
    assert rc == 0 and blocks == (3 + 1) * -(-C // 8)
    words = fmbank_ref.words_for(C, seed=1000 * R + C)
    if C >= 8:
        assert set(fmbank_ref.SPECIAL_WORDS) <= set(words)
    iq = ddc_ref.random_iq(nb * L * R, seed=R + C)
    states = fmbank_ref.states_for(C, seed=50 + R)
    if C >= 2:
        states[C - 1] = states[0]                        # the same word and the same state: the same station
    want = fmbank_ref.expected(oracle, iq, R, words, L, states)
    got = engine.fm_bank(iq, R, words, L, states)
    check(got, want, (R, C))
    assert np.any(got[0] != 0)
    if C >= 2:
        assert np.array_equal(got[0][0], got[0][C - 1]) and np.array_equal(got[1][0], got[1][C - 1])
    if C >= 3:
        assert not np.array_equal(got[0][0], got[0][1])


def check_rows(audio, st, want, C, n, stride, what):
    """audio f32 [32 * stride + tail] and state_out f32 [32 * 21 + tail] of a launch of C channels into sentinels:
    rows 0 .. C - 1 hold the first C expected rows, every other word its sentinel (compared as bit patterns)."""
    rows = channels.MAX_CH
    want_audio, want_st = want
    mark = SENTINEL.view(np.uint32)
    body = audio[:rows * stride].reshape(rows, stride)
    bad = np.argwhere(body[:C, :n] != want_audio[:C])
    assert bad.size == 0, (what, "audio", len(bad), bad[:4])
    bad = np.argwhere(st[:C * STATE].reshape(C, STATE) != want_st[:C])
    assert bad.size == 0, (what, "state", bad[:8])
    assert np.all(body[:C, n:].view(np.uint32) == mark) and np.all(body[C:].view(np.uint32) == mark), (what, "audio rows")
    assert np.all(audio[rows * stride:].view(np.uint32) == mark) and np.all(st[C * STATE:].view(np.uint32) == mark), (what, "tails")


@pytest.mark.parametrize("R", channels.paths("fmbank"), ids=channels.path_id)
def test_every_channel_count(engine, oracle, built, tile, R):
    """tests/ddc_family_channels.py: C = 1 .. 32 of one set of 32 words and 32 carried states over one capture of two
    full tiles and a remainder: 4 ceil(C / 8) workgroups, so that with three column tiles blockIdx.x = 0 .. 11 passes
    through the division by nct and meets every (tile, column tile).  Every launch goes through the plan's run into 32
    audio rows of audio_stride > the run's length and 32 x 21 floats of state_out, each with a tail, all sentinels."""
    iq, L, nb = channels.fm_inputs("fmbank", R, tile)
    n = nb * (L // 4)
    ntiles = -(-n // tile)
    stride, tail = n + 7, 64
    rows = channels.MAX_CH
    want = channels.fm_expected(oracle, "fmbank", R, tile)
    fill_audio = np.full(rows * stride + tail, SENTINEL, dtype=np.float32)
    fill_st = np.full(rows * STATE + tail, SENTINEL, dtype=np.float32)
    plan = built.FmBankPlan.open(engine)
    d_iq = engine.upload(iq)
    d_in = engine.upload(channels.states())
    for C in channels.channels("fmbank", R):
        rc, blocks, _, _, t = built.fmbank_grid(R, C, L, nb)
        assert rc == 0 and t == tile and ntiles == 3 and blocks == (ntiles + 1) * -(-C // 8)
        d_out, d_audio = engine.upload(fill_st), engine.upload(fill_audio)
        plan.run(R, d_iq, L, nb, channels.WORDS[:C], d_in, d_out, d_audio, audio_stride=stride)
        engine.sync()
        audio = engine.download(d_audio, np.float32, fill_audio.shape)
        st = engine.download(d_out, np.float32, fill_st.shape)
        d_out.free(), d_audio.free()
        check_rows(audio, st, want, C, n, stride, (R, C))
    assert np.array_equal(engine.download(d_in, np.float32, (rows, STATE)), channels.states())
    plan.close()
    d_iq.free(), d_in.free()


@pytest.mark.parametrize("nb", [1, 3])
@pytest.mark.parametrize("L", [20, 22, 23, 25])
def test_block_shapes(engine, oracle, L, nb):
    """The odd-sample and odd-output skips, all inside one tile."""
    R, C = 8, 9
    words = fmbank_ref.words_for(C, seed=L)
    iq = ddc_ref.random_iq(nb * L * R, seed=L + nb)
    states = fmbank_ref.states_for(C, seed=L)
    check(engine.fm_bank(iq, R, words, L, states), fmbank_ref.expected(oracle, iq, R, words, L, states), (L, nb))


def test_tiles_with_block_borders_inside(engine, oracle, built, tile):
    """block_len = 4102 (2 mod 4: half = 2051 is odd, the first half-band's last output of every block is skipped);
    the audio spans at least three tiles and a partial one, and the block borders fall inside tiles."""
    R, C, L = 12, 2, 4102
    quarter = L // 4
    nb = -(-(3 * tile + 1) // quarter)
    if (nb * quarter) % tile == 0:
        nb += 1
    assert all((b * quarter) % tile != 0 for b in range(1, nb + 1))
    words = [777, -20001]
    iq = ddc_ref.random_iq(nb * L * R, seed=41)
    states = fmbank_ref.states_for(C, seed=42)
    check(engine.fm_bank(iq, R, words, L, states), fmbank_ref.expected(oracle, iq, R, words, L, states), L)


# ---- every block shape over several tiles (fm_ref.tile_cases; tests/test_fmbank_cpu.py checks what the cases reach) ----

CASES = [(regime, residue) for regime in "abc" for residue in range(4)]
TILE_RUNS = [fmbank_ref.TILE_BANK + c for c in CASES] + [b + c for b in fmbank_ref.SKIP_BANKS for c in CASES if c[1] in (1, 3)]


def _tile_case(built, tile, regime, residue, R, C):
    """the case of the library's own tile, and its grid: per column tile one workgroup per tile and the one of the states"""
    case = {(c.regime, c.residue): c for c in fm_ref.tile_cases(tile)}[regime, residue]
    rc, blocks, _, _, t = built.fmbank_grid(R, C, case.block_len, case.nblocks)
    assert rc == 0 and t == tile and case.ntiles(tile) >= 4 and blocks == (case.ntiles(tile) + 1) * -(-C // 8), case.id
    return case


@pytest.mark.parametrize("R,C,regime,residue", TILE_RUNS)
def test_tile_cases(engine, oracle, built, tile, R, C, regime, residue):
    """Dozens of tiny blocks per tile (block_len = 23 fills LDS as far as any shape can), borders just in front of
    tiles, long blocks: every block_len mod 4 over four tiles or more, from carried states."""
    case = _tile_case(built, tile, regime, residue, R, C)
    iq, words, states = fmbank_ref.case_inputs(case, R, C)
    want = fmbank_ref.expected(oracle, iq, R, words, case.block_len, states, key=("tile case", case, R, C))
    got = engine.fm_bank(iq, R, words, case.block_len, states)
    check(got, want, (case.id, R, C))
    assert np.any(got[0] != 0)
    assert np.array_equal(got[0][0], got[0][C - 1]) and np.array_equal(got[1][0], got[1][C - 1])      # the same station


@pytest.mark.parametrize("name", ["axes", "all128"])
def test_branch_inputs(engine, oracle, name):
    """The captures of tests/test_fmbank_cpu.py's input conditions: x == 0 with every sign of y, both sides of the
    limiter, both branches of |z| < 1.  Every byte 128: the oracle's response to zeros from the given state."""
    R, C, L, nb = fmbank_ref.BRANCH_R, fmbank_ref.BRANCH_C, fmbank_ref.BRANCH_L, fmbank_ref.BRANCH_NB
    iq = fmbank_ref.branch_captures()[name]
    words = fmbank_ref.branch_words()
    states = fmbank_ref.states_for(C, seed=90)
    got = engine.fm_bank(iq, R, words, L, states)
    check(got, fmbank_ref.expected(oracle, iq, R, words, L, states), name)
    if name == "all128":
        zeros = np.zeros((nb * L, 2), dtype=np.int32)
        for c in range(C):
            a, s = fm_ref.oracle_chain(oracle, zeros, L, states[c])
            assert np.array_equal(got[0][c], a) and np.array_equal(got[1][c], s), c


def _run_chunks(engine, plan, iq, R, words, L, states, first, cuts, stride=None):
    """Calls cut at the block indices `cuts`, swapping two state buffers -> (audio [C, n], final states)."""
    C, nb, quarter = len(words), cuts[-1], L // 4
    n = nb * quarter
    stride = n if stride is None else stride
    d_iq = engine.upload(iq)
    d_st = [engine.upload(states), engine.alloc(states.nbytes)]
    d_audio = engine.alloc(C * stride * 4)
    for a, b in zip(cuts, cuts[1:]):
        plan.run(R, d_iq.ptr + a * L * R * 2, L, b - a, words, d_st[0], d_st[1], d_audio.ptr + a * quarter * 4,
                 audio_stride=stride, first_dec_index=first + a * L)
        d_st.reverse()
    engine.sync()
    audio = engine.download(d_audio, np.float32, (C, stride))[:, :n]
    st = engine.download(d_st[0], np.float32, (C, STATE))
    for b in (d_iq, d_audio, *d_st):
        b.free()
    return audio, st


@pytest.mark.parametrize("first", [0, (1 << 40) + 12345])
def test_chunks_concatenate_to_one_run(engine, oracle, built, tile, first):
    R, C, L, nb = 10, 3, 2 * tile + 8, 5                 # cuts at block multiples, inside tiles; 16-byte aligned chunks
    words = [777, -20001, 32767]
    iq = ddc_ref.random_iq(nb * L * R, seed=5)
    states = fmbank_ref.states_for(C, seed=6)
    want = fmbank_ref.expected(oracle, iq, R, words, L, states, first)
    whole = engine.fm_bank(iq, R, words, L, states, first_dec_index=first)
    check(whole, want, "one call")
    plan = built.FmBankPlan.open(engine)
    for cuts in ((0, 2, 5), (0, 1, 3, 5)):
        assert all((a * L * R * 2) % 16 == 0 for a in cuts)
        check(_run_chunks(engine, plan, iq, R, words, L, states, first, cuts), whole, cuts)
    plan.close()
    if first:
        assert not np.array_equal(whole[0], engine.fm_bank(iq, R, words, L, states)[0])   # the index is in the phase


def test_chunks_of_odd_blocks_with_borders_in_front_of_tiles(engine, oracle, built, tile):
    """Both maps skipping, quarter = tile - 2, a first_dec_index beyond 2^40: calls cut behind blocks 1 and 4, the
    state buffers swapped between them, equal the one call and the expected values."""
    R, C = fmbank_ref.TILE_BANK
    case = _tile_case(built, tile, "b", 3, R, C)
    L, first, cuts = case.block_len, (1 << 40) + 12345, (0, 1, 4)
    assert L % 2 == 1 and cuts[-1] == case.nblocks and all((a * L * R * 2) % 16 == 0 for a in cuts)
    iq, words, states = fmbank_ref.case_inputs(case, R, C)
    want = fmbank_ref.expected(oracle, iq, R, words, L, states, first)
    whole = engine.fm_bank(iq, R, words, L, states, first_dec_index=first)
    check(whole, want, "one call")
    plan = built.FmBankPlan.open(engine)
    chunks = _run_chunks(engine, plan, iq, R, words, L, states, first, cuts)
    plan.close()
    check(chunks, whole, cuts)
    check(chunks, want, cuts)
    unshifted = fmbank_ref.expected(oracle, iq, R, words, L, states, key=("tile case", case, R, C))
    assert not np.array_equal(want[0], unshifted[0])                   # the index is in the phase


def test_stride_and_nothing_outside_the_ranges(engine, oracle, built, tile):
    R, C, L, nb = 12, 9, tile + 6, 5
    n = nb * (L // 4)
    stride, tail = n + 7, 64
    words = fmbank_ref.words_for(C, seed=3)
    iq = ddc_ref.random_iq(nb * L * R, seed=4)
    states = fmbank_ref.states_for(C, seed=5)
    want_audio, want_st = fmbank_ref.expected(oracle, iq, R, words, L, states)
    sentinel = np.float32(-12345.678)
    plan = built.FmBankPlan.open(engine)
    d_iq = engine.upload(iq)
    d_in = engine.upload(states)
    d_out = engine.upload(np.full(C * STATE + tail, sentinel, dtype=np.float32))
    d_audio = engine.upload(np.full(C * stride + tail, sentinel, dtype=np.float32))
    plan.run(R, d_iq, L, nb, words, d_in, d_out, d_audio, audio_stride=stride)
    engine.sync()
    audio = engine.download(d_audio, np.float32, (C * stride + tail,))
    st = engine.download(d_out, np.float32, (C * STATE + tail,))
    body = audio[:C * stride].reshape(C, stride)
    assert np.array_equal(body[:, :n], want_audio)
    assert np.all(body[:, n:] == sentinel) and np.all(audio[C * stride:] == sentinel)
    assert np.array_equal(st[:C * STATE].reshape(C, STATE), want_st) and np.all(st[C * STATE:] == sentinel)
    assert np.array_equal(engine.download(d_in, np.float32, (C, STATE)), states)

    # with a device the refusals still hold and leave the buffers untouched
    err = built.fmbank_last_error
    assert plan.run(R, d_iq, L, nb, words, d_in, d_out, d_audio, audio_stride=n - 1, check=False) == -1 and "audio_stride" in err()
    assert plan.run(R, d_iq, L, nb, [P // 2], d_in, d_out, d_audio, audio_stride=stride, check=False) == -1 and "tuning word" in err()
    assert plan.run(R, d_iq, L, nb, words, d_in, d_out, d_audio, audio_stride=stride, first_dec_index=-1, check=False) == -1
    assert plan.run(R, d_iq, L, nb, words, d_in, d_in.ptr + 4, d_audio, audio_stride=stride, check=False) == -1 and "overlap" in err()
    assert plan.run(R, d_iq, 19, nb, words, d_in, d_out, d_audio, audio_stride=stride, check=False) == -1 and "block_len" in err()
    engine.sync()
    assert np.array_equal(engine.download(d_audio, np.float32, (C * stride + tail,)), audio)
    assert np.array_equal(engine.download(d_out, np.float32, (C * STATE + tail,)), st)

    # no blocks: the states are copied, nothing else is written
    d_out2 = engine.upload(np.full(C * STATE + tail, sentinel, dtype=np.float32))
    assert plan.run(R, None, L, 0, words, d_in, d_out2, None, audio_stride=0) == 0
    engine.sync()
    st2 = engine.download(d_out2, np.float32, (C * STATE + tail,))
    assert np.array_equal(st2[:C * STATE].reshape(C, STATE), states) and np.all(st2[C * STATE:] == sentinel)
    assert np.array_equal(engine.download(d_audio, np.float32, (C * stride + tail,)), audio)
    plan.close()
    for b in (d_iq, d_in, d_out, d_out2, d_audio):
        b.free()


def test_device_composition(engine):
    """Engine.fm_bank equals Engine.ddc followed by Engine.fm_audio_blocks per channel: the definition of
    include/rtlws_fmbank.h, on the device."""
    R, C, L, nb = 12, 2, 1030, 3
    words = [5000, -9000]
    first = 4242
    iq = ddc_ref.random_iq(nb * L * R, seed=12)
    states = fmbank_ref.states_for(C, seed=13)
    audio, st = engine.fm_bank(iq, R, words, L, states, first_dec_index=first)
    streams = engine.ddc(iq, R, words, first_dec_index=first)
    for c in range(C):
        want_audio, want_st = engine.fm_audio_blocks(streams[c], L, states[c])
        assert np.array_equal(audio[c], want_audio) and np.array_equal(st[c], want_st), c
    assert np.any(audio != 0)


def test_capture_and_replay(built, oracle, tile):
    """A run is one kernel launch: captured on a side stream as tests/test_ddc_gpu.py captures the bank, replayed
    twice, identical to an eager launch and to the expected values."""
    import torch
    dev = torch.device("cuda", 0)
    eng = built.Engine(0)
    plan = built.FmBankPlan.open(eng)
    R, C, L, nb = 8, 8, tile + 6, 3
    n = nb * (L // 4)
    words = fmbank_ref.words_for(C, seed=8)
    iq_host = ddc_ref.random_iq(nb * L * R, seed=9)
    states = fmbank_ref.states_for(C, seed=10)
    iq = torch.from_numpy(iq_host).to(dev)
    st_in = torch.from_numpy(states).to(dev)
    audio = torch.zeros((C, n), dtype=torch.float32, device=dev)
    st_out = torch.zeros((C, STATE), dtype=torch.float32, device=dev)

    def launch(a, s):
        plan.run(R, iq.data_ptr(), L, nb, words, st_in.data_ptr(), s.data_ptr(), a.data_ptr(), first_dec_index=77,
                 stream=built.torch_stream_handle())

    g = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        with torch.cuda.graph(g, stream=side):
            launch(audio, st_out)
    torch.cuda.current_stream().wait_stream(side)
    assert float(audio.abs().sum()) == 0 and float(st_out.abs().sum()) == 0      # capture enqueued nothing
    g.replay()
    torch.cuda.synchronize()
    first_audio, first_st = audio.clone(), st_out.clone()
    audio.zero_()
    st_out.zero_()
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(first_audio, audio) and torch.equal(first_st, st_out)
    eager_audio, eager_st = torch.zeros_like(audio), torch.zeros_like(st_out)
    launch(eager_audio, eager_st)
    torch.cuda.synchronize()
    assert torch.equal(first_audio, eager_audio) and torch.equal(first_st, eager_st)
    want_audio, want_st = fmbank_ref.expected(oracle, iq_host, R, words, L, states, 77)
    assert np.array_equal(audio.cpu().numpy(), want_audio) and np.array_equal(st_out.cpu().numpy(), want_st)
    plan.close()
    eng.close()

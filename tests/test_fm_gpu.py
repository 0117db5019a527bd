"""GPU suite of include/rtlws_fm.h: the FM receive chain in one launch (CIC block sums, demodulator, both
half-bands) against the reference-object-code golden and a loop of the oracle's per-block chain, at single-tile
shapes and at every block_len mod 4 over several tiles (fm_ref.tile_cases).  Every
comparison is np.array_equal: the fused path is held to equality, not to a tolerance."""
import ctypes as C

import numpy as np
import pytest

import fm_ref
from conftest import golden

pytestmark = pytest.mark.gpu

SHAPES = [(L, nb) for L in (20, 22, 23, 25, 1024) for nb in (1, 3)]
INPUTS = {"A": fm_ref.input_a, "B": fm_ref.input_b}


@pytest.fixture(scope="module")
def fm(built, engine):
    L = built.fm_lib()
    assert L.rtlws_fm_prepare(engine.h) == 0, built.fm_last_error()
    return L


def _case(kind, L, nb):
    return INPUTS[kind](L * nb, seed=1000 * nb + L), fm_ref.random_state(L + nb)


def test_golden_blocks_as_one_launch_and_as_a_chain(engine, fm):
    g = golden("audio_ref.npz")
    n = int(g["block_len"])
    nb = g["audio"].shape[0]
    assert nb == 4
    iq = np.ascontiguousarray(g["iq"][:nb * n])
    zero = np.zeros(fm_ref.STATE, dtype=np.float32)                 # the reference's start
    audio, st_all = engine.fm_audio_blocks(iq, n, zero)
    assert np.array_equal(audio, g["audio"].reshape(-1))
    st = zero
    for k in range(nb):
        a, st = engine.fm_audio_blocks(iq[k * n:(k + 1) * n], n, st)
        assert np.array_equal(a, g["audio"][k]), k
    assert np.array_equal(st, st_all)


@pytest.mark.parametrize("L,nb", SHAPES)
@pytest.mark.parametrize("kind", ["A", "B"])
def test_block_shapes_equal_the_oracle_loop(engine, fm, oracle, kind, L, nb):
    iq, st = _case(kind, L, nb)
    want, want_st = fm_ref.oracle_chain(oracle, iq, L, st)
    got, got_st = engine.fm_audio_blocks(iq, L, st)
    assert got.size == nb * (L // 4)
    assert np.array_equal(got, want)
    assert np.array_equal(got_st, want_st), np.nonzero(got_st != want_st)


@pytest.mark.parametrize("kind", ["A", "B"])
def test_inputs_reach_both_sides_of_the_limiter(oracle, kind):
    """On the ORACLE's demodulator output: at least 10 % of the samples of the cases above are clamped and at
    least 10 % are not -- an always-clamping (or never-clamping) kernel cannot pass them."""
    demod = []
    for L, nb in SHAPES:
        iq, st = _case(kind, L, nb)
        demod.append(oracle.fm_demod(iq, prev_phase=float(st[0]))[0])
    big = oracle.fm_demod(_case(kind, 1024, 3)[0])[0]
    for d in (np.concatenate(demod), big):
        clamped = np.mean(np.abs(d) == 1.0)
        print("input %s: %.1f %% of %d samples clamped" % (kind, 100 * clamped, d.size))
        assert 0.10 <= clamped <= 0.90


def test_tiles_with_block_borders_inside(engine, fm, oracle, built):
    """block_len = 4102 (2 mod 4: half = 2051 is odd, the first half-band's last output of every block is skipped);
    the audio spans at least three tiles and a partial one, and the block borders fall inside tiles."""
    L = 4102
    tile = built.fm_grid(L, 1, 0)[4]
    quarter = L // 4
    nb = -(-(3 * tile + 1) // quarter)
    if (nb * quarter) % tile == 0:
        nb += 1
    rc, blocks, threads, lds, _ = built.fm_grid(L, nb, 0)
    assert rc == 0 and blocks - 1 == -(-nb * quarter // tile) >= 4 and (nb * quarter) % tile != 0
    assert all((b * quarter) % tile != 0 for b in range(1, nb))     # borders inside tiles
    for kind in ("A", "B"):
        iq, st = _case(kind, L, nb)
        want, want_st = fm_ref.oracle_chain(oracle, iq, L, st)
        got, got_st = engine.fm_audio_blocks(iq, L, st)
        assert np.array_equal(got, want), kind
        assert np.array_equal(got_st, want_st), kind


# ---- every block shape over several tiles (fm_ref.tile_cases; tests/test_fm_cpu.py checks what the cases reach) ----

CASES = [(regime, residue) for regime in "abc" for residue in range(4)]
ODD_BLOCKS = [(regime, residue) for regime in "abc" for residue in (1, 3)]       # the stage-1 map skips


def _tile_case(built, regime, residue):
    """the case of the library's own tile, and its grid: one workgroup per tile and the one of the state"""
    tile = built.fm_grid(20, 1, 0)[4]
    case = {(c.regime, c.residue): c for c in fm_ref.tile_cases(tile)}[regime, residue]
    ntiles = case.ntiles(tile)
    for R in (0, 7, 8, 10, 12):
        rc, blocks, _, _, t = built.fm_grid(case.block_len, case.nblocks, R)
        assert rc == 0 and t == tile and blocks == ntiles + 1 >= 5, (case.id, R)
    return case


def _cu8_case(case, R):
    seed = 100 * case.block_len + R
    u8 = np.random.default_rng(seed).integers(0, 256, size=(case.block_len * case.nblocks * R, 2), dtype=np.uint8)
    return u8, fm_ref.random_state(seed + 1)


@pytest.mark.parametrize("regime,residue", CASES)
def test_tile_cases_equal_the_oracle_loop(engine, fm, oracle, built, regime, residue):
    """Dozens of tiny blocks per tile, borders just in front of tiles, long blocks: every block_len mod 4 over four
    tiles or more, from a carried state, against the loop of the reference's per-block chain."""
    case = _tile_case(built, regime, residue)
    for kind, make in INPUTS.items():
        iq, st = fm_ref.case_input(make, case)
        want, want_st = fm_ref.oracle_chain(oracle, iq, case.block_len, st)
        got, got_st = engine.fm_audio_blocks(iq, case.block_len, st)
        assert got.size == case.nblocks * (case.block_len // 4)
        bad = np.nonzero(got != want)[0]
        assert bad.size == 0, (case.id, kind, bad.size, bad[:8])
        assert np.array_equal(got_st, want_st), (case.id, kind, np.nonzero(got_st != want_st))


@pytest.mark.parametrize("R,regime,residue", [(8,) + c for c in CASES] + [(R,) + c for R in (10, 12, 7) for c in ODD_BLOCKS])
def test_tile_cases_with_the_cic_in_front(engine, fm, oracle, built, R, regime, residue):
    """The cu8 form at every loader: audio, state and every decimated sample -- those an odd block skips and those
    behind the last tile's range included."""
    case = _tile_case(built, regime, residue)
    u8, st = _cu8_case(case, R)
    rc, dec, _ = oracle.cic_decimate(R, u8)
    assert rc == 0 and dec.shape == (case.nblocks * case.block_len, 2)
    want, want_st = fm_ref.oracle_chain(oracle, dec, case.block_len, st)
    got, got_st, got_dec = engine.fm_audio_blocks_cu8(u8, R, case.block_len, st, want_dec=True)
    bad = np.nonzero(np.any(got_dec != dec, axis=1))[0]
    assert bad.size == 0, (case.id, "dec", bad.size, bad[:8])
    bad = np.nonzero(got != want)[0]
    assert got.size == want.size and bad.size == 0, (case.id, "audio", bad.size, bad[:8])
    assert np.array_equal(got_st, want_st), (case.id, np.nonzero(got_st != want_st))


@pytest.mark.parametrize("R", [8, 7])
def test_stage_2_off_over_tiles_with_skipping_maps(engine, fm, oracle, built, R):
    """run_stage2 = 0 where both maps skip and the borders lie in front of the tiles: every decimated sample is
    delivered by the tiles and the last workgroup, the state is the exhausted pool's."""
    case = _tile_case(built, "b", 3)
    u8, st = _cu8_case(case, R)
    rc, dec, _ = oracle.cic_decimate(R, u8)
    assert rc == 0
    _, want_st = fm_ref.oracle_chain(oracle, dec, case.block_len, st, run_stage2=False)
    none, got_st, got_dec = engine.fm_audio_blocks_cu8(u8, R, case.block_len, st, run_stage2=False, want_dec=True)
    assert none.size == 0
    assert np.array_equal(got_dec, dec), np.nonzero(np.any(got_dec != dec, axis=1))[0][:8]
    assert np.array_equal(got_st[11:21], st[11:21])
    assert np.array_equal(got_st, want_st), np.nonzero(got_st != want_st)


@pytest.mark.parametrize("L", [23, 1024])
def test_stage_2_off_is_the_exhausted_pool(engine, fm, oracle, built, L):
    nb = 3
    iq, st = _case("A", L, nb)
    naudio = nb * (L // 4)
    d_iq = engine.upload(iq)
    d_st = engine.upload(np.concatenate([st, np.zeros(3, np.float32), np.full(24, 9.0, np.float32)]))
    d_audio = engine.upload(np.full(naudio, -77.0, dtype=np.float32))
    assert fm.rtlws_fm_audio_blocks(engine.h, d_iq.ptr, L, nb, d_st.ptr, d_st.ptr + 96, 0, d_audio.ptr, None) == 0
    assert np.all(engine.download(d_audio, np.float32, (naudio,)) == -77.0)       # the sentinel is untouched
    mixed = engine.download(d_st, np.float32, (48,))[24:45]
    _, want_st = fm_ref.oracle_chain(oracle, iq, L, st, run_stage2=False)
    assert np.array_equal(mixed[11:21], st[11:21])
    assert np.array_equal(mixed[0:11], want_st[0:11])
    assert np.array_equal(mixed, want_st)
    # a NULL d_audio is accepted when nothing is written to it
    assert fm.rtlws_fm_audio_blocks(engine.h, d_iq.ptr, L, nb, d_st.ptr, d_st.ptr + 96, 0, None, None) == 0
    assert np.array_equal(engine.download(d_st, np.float32, (48,))[24:45], want_st)
    # the next launch, stage 2 on, from that mixed state
    iq2, _ = _case("B", L, nb)
    want, want_st2 = fm_ref.oracle_chain(oracle, iq2, L, want_st)
    got, got_st2 = engine.fm_audio_blocks(iq2, L, mixed)
    assert np.array_equal(got, want) and np.array_equal(got_st2, want_st2)
    for b in (d_iq, d_st, d_audio):
        b.free()


@pytest.mark.parametrize("R", [1, 7, 8, 10, 12, 128])
def test_cu8_form_with_the_cic_in_front(engine, fm, oracle, built, R):
    """cmplx_u8 in: oracle.cic_decimate, then the oracle's chain.  At R = 8 the audio spans four tiles and a
    partial one (block_len 4102), at the other factors one tile and a remainder (block_len 1030: half = 515 and
    the block length itself are skipped-sample shapes)."""
    tile = built.fm_grid(20, 1, R)[4]
    L, nb = (4102, 2) if R == 8 else (1030, 3)
    naudio = nb * (L // 4)
    assert naudio >= (3 * tile + 1 if R == 8 else tile + 1) and naudio % tile != 0
    rng = np.random.default_rng(R)
    u8 = rng.integers(0, 256, size=(L * nb * R, 2), dtype=np.uint8)
    st = fm_ref.random_state(R)
    rc, dec, _ = oracle.cic_decimate(R, u8)
    assert rc == 0
    want, want_st = fm_ref.oracle_chain(oracle, dec, L, st)
    got, got_st, got_dec = engine.fm_audio_blocks_cu8(u8, R, L, st, want_dec=True)
    assert np.array_equal(got_dec, dec)
    assert np.array_equal(got, want)
    assert np.array_equal(got_st, want_st)
    got, got_st = engine.fm_audio_blocks_cu8(u8, R, L, st)          # d_dec = NULL is accepted
    assert np.array_equal(got, want) and np.array_equal(got_st, want_st)
    # stage 2 off: the decimated samples are still delivered, the state as the oracle leaves it
    _, off_st = fm_ref.oracle_chain(oracle, dec, L, st, run_stage2=False)
    none, got_st, got_dec = engine.fm_audio_blocks_cu8(u8, R, L, st, run_stage2=False, want_dec=True)
    assert none.size == 0 and np.array_equal(got_dec, dec) and np.array_equal(got_st, off_st)


def test_no_blocks_copies_the_state_and_refusals_with_a_device(engine, fm, built):
    st = fm_ref.random_state(3)
    audio, out = engine.fm_audio_blocks(np.zeros((0, 2), np.int32), 20, st)
    assert audio.size == 0 and np.array_equal(out, st)
    d = engine.alloc(1 << 16)
    a, b, s1, s2 = d.ptr, d.ptr + 32768, d.ptr + 49152, d.ptr + 49152 + 96
    cs32 = lambda **kw: fm.rtlws_fm_audio_blocks(*[kw.get(k, v) for k, v in (
        ("e", engine.h), ("iq", a), ("L", 1024), ("nb", 2), ("si", s1), ("so", s2), ("run2", 1), ("audio", b), ("st", None))])
    cu8 = lambda **kw: fm.rtlws_fm_audio_blocks_cu8(*[kw.get(k, v) for k, v in (
        ("e", engine.h), ("r", 8), ("iq", a), ("L", 64), ("nb", 2), ("si", s1), ("so", s2), ("run2", 1), ("audio", b),
        ("dec", None), ("st", None))])
    for fn in (cs32, cu8):
        assert fn(L=19) == -1 and fn(nb=-1) == -1
        assert fn(iq=None) == -1 and fn(si=None) == -1 and fn(so=None) == -1 and fn(audio=None) == -1
        assert fn(so=s1) == -1 and "differ" in built.fm_last_error()
        assert fn(e=None) == -1
    assert cs32(iq=a + 4) == -1 and cu8(iq=a + 8) == -1 and cu8(dec=b + 4) == -1
    assert cu8(r=0) == -1 and cu8(r=129) == -1
    assert cs32() == 0 and cu8() == 0 and built.fm_last_error() == ""
    engine.sync()
    d.free()


def test_capture_and_replay(built, oracle):
    """After rtlws_fm_prepare a launch makes no other runtime call: captured on a side stream the way
    tests/test_graph_gpu.py captures rtlws_spectra_batch, replayed twice, identical bytes to an eager launch
    and to the oracle."""
    import torch
    dev = torch.device("cuda", 0)
    eng = built.Engine(0)
    fm = built.fm_lib()
    assert fm.rtlws_fm_prepare(eng.h) == 0
    R, L, nb = 10, 1030, 3
    rng = np.random.default_rng(21)
    u8_host = rng.integers(0, 256, size=(L * nb * R, 2), dtype=np.uint8)
    st_host = fm_ref.random_state(21)
    u8 = torch.from_numpy(u8_host).to(dev)
    st_in = torch.from_numpy(st_host).to(dev)
    st_out = torch.zeros(21, dtype=torch.float32, device=dev)
    audio = torch.zeros(nb * (L // 4), dtype=torch.float32, device=dev)
    dec = torch.zeros((L * nb, 2), dtype=torch.int32, device=dev)

    def launch(a, s, d):
        rc = fm.rtlws_fm_audio_blocks_cu8(eng.h, R, u8.data_ptr(), L, nb, st_in.data_ptr(), s.data_ptr(), 1,
                                          a.data_ptr(), d.data_ptr(), built.torch_stream_handle())
        assert rc == 0, built.fm_last_error()

    g = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        with torch.cuda.graph(g, stream=side):
            launch(audio, st_out, dec)
    torch.cuda.current_stream().wait_stream(side)
    assert float(audio.abs().sum()) == 0.0 and float(st_out.abs().sum()) == 0.0     # capture enqueued nothing
    g.replay()
    torch.cuda.synchronize()
    first = (audio.clone(), st_out.clone(), dec.clone())
    audio.zero_(), st_out.zero_(), dec.zero_()
    g.replay()
    torch.cuda.synchronize()
    assert all(torch.equal(x, y) for x, y in zip(first, (audio, st_out, dec)))     # replays are bit-identical
    eager = (torch.zeros_like(audio), torch.zeros_like(st_out), torch.zeros_like(dec))
    launch(*eager)
    torch.cuda.synchronize()
    assert all(torch.equal(x, y) for x, y in zip(first, eager))
    rc, ref_dec, _ = oracle.cic_decimate(R, u8_host)
    want, want_st = fm_ref.oracle_chain(oracle, ref_dec, L, st_host)
    assert np.array_equal(audio.cpu().numpy(), want) and np.array_equal(st_out.cpu().numpy(), want_st)
    assert np.array_equal(dec.cpu().numpy(), ref_dec)
    eng.close()

"""GPU suite of include/rtlws_sift.h (librtlws_sift.so) against its numpy restatement (tests/sift_ref.py): every word of
d_cand, of d_count and of the plane, bit for bit.  Every case runs with the outputs and the workspace preset to a pattern:
the words of d_cand behind the last candidate and the guard words behind every buffer still hold it afterwards.  The
inputs are synthetic arrays (the shapes, the tile's borders, planted ties and special values, the limits of max_cand and
of the threshold) and what Engine.pulse and rtlws_pulse_run leave, chained on the device."""
import ctypes as C

import numpy as np
import pytest

import sift_ref as ref
from test_sift_cpu import RANDOM_CASES

pytestmark = pytest.mark.gpu

FILL = np.array([0x7FC5A5A5], np.uint32).view(np.float32)[0]          # a quiet NaN with a payload: the preset pattern
FILL_BITS = np.uint32(0x7FC5A5A5)
W1 = np.array([2], np.int32)


@pytest.fixture(scope="module")
def sf(built):
    import rtlws.sift
    return rtlws.sift


def _words(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _check(sf, engine, case, thr, rt, rs, max_cand=None, name=None, rich=False):
    """one run through rtlws.sift.sift with `fill` against the restatement -> the restatement's (cand, count, score, k)"""
    peak, at, mom, widths, seg, nout = case
    want, count, score, k_of = ref.sift_ref(peak, at, mom, widths, seg, nout, thr, rt, rs)
    if rich:
        found, dropped, most = len(want), int(count[1]) - len(want), int(want[:, 6].max())
        assert found >= 8 and dropped >= 1 and most >= 3, (name, found, dropped, most)
    T, K, S = peak.shape
    room = max(len(want), 1) + 3 if max_cand is None else max_cand
    cand, cnt, sc, kk, work = sf.sift(engine, peak, at, mom, widths, seg, nout, thr, rt, rs, room, fill=FILL)
    n = min(len(want), room)
    assert cnt[:2].tolist() == count.tolist(), (name, cnt[:2], count)
    assert cand.shape == (room * 8 + sf.GUARD,) and np.array_equal(cand[:n * 8].reshape(n, 8), want[:n]), (name, n, cand[:16], want[:2])
    assert np.all(cand[n * 8:] == FILL_BITS) and np.all(_words(cnt[2:]) == FILL_BITS), name
    assert np.array_equal(_words(sc[:T * S]), _words(score).reshape(-1)), (name, "score")
    assert np.array_equal(kk[:T * S], k_of.reshape(-1)), (name, "k")
    assert np.all(_words(sc[T * S:]) == FILL_BITS) and np.all(_words(kk[T * S:]) == FILL_BITS) and np.all(work[-sf.GUARD:] == FILL_BITS), name
    return want, count, score, k_of


# ---- shapes ------------------------------------------------------------------------------------------------------------

def test_one_event(sf, engine):
    mom = ref.flat_moments(1, 64, 64)
    case = (np.full((1, 1, 1), 20.0, np.float32), np.full((1, 1, 1), 17, np.int32), mom, W1, 64, 64)
    for thr, found in ((1.0, 1), (100.0, 0), (-np.inf, 1), (np.inf, 0)):
        for rt, rs in ((0, 0), (32, 8)):
            want = _check(sf, engine, case, thr, rt, rs, name=(thr, rt, rs))[0]
            assert len(want) == found and (not found or want[0].tolist()[:4] + want[0].tolist()[6:] == [0, 0, 0, 17, 1, 0])


@pytest.mark.parametrize("T,K,S,seed,tail,step,thr,rt,rs", RANDOM_CASES, ids=["%dx%dx%d-seed%d" % c[:4] for c in RANDOM_CASES])
def test_the_random_cases(sf, engine, T, K, S, seed, tail, step, thr, rt, rs):
    """5 x 3 x 7 and 40 x 16 x 33 among them, a last segment of 17 and of 2 outputs, peaks on a grid so that scores tie"""
    case = ref.random_case(T, K, S, seed, tail=tail, step=step)
    _check(sf, engine, case, thr, rt, rs, name=(T, K, S), rich=True)
    for radii in ((0, 0), (32, 8), (32, 0), (0, 8)):
        _check(sf, engine, case, thr, *radii, name=(T, K, S, radii))


RADII = [(0, 0), (1, 1), (32, 8), (32, 0), (0, 8)]


@pytest.mark.parametrize("rt,rs", RADII, ids=["rt%d-rs%d" % r for r in RADII])
def test_planes_across_the_tile_s_borders(sf, engine, rt, rs):
    """T and S one below, at and one above the tile's extent (rtlws_sift_geometry's), and across two tiles either way"""
    rc, _, _, _, tile_t, tile_s, _ = sf.geometry(W1, 64, rt, rs, 1, 64)
    assert rc == 0 and (tile_t, tile_s) == (64, 64)
    for T in (tile_t - 1, tile_t, tile_t + 1):
        for S in (tile_s - 1, tile_s, tile_s + 1):
            case = ref.random_case(T, 2, S, 100 * T + S, blobs=25)
            _check(sf, engine, case, 2.0, rt, rs, name=(T, S, rt, rs), rich=(rt, rs) == (1, 1))
    _check(sf, engine, ref.random_case(2 * tile_t + 1, 1, 2 * tile_s + 1, 5, blobs=40, tail=3), 2.0, rt, rs, name=("2x2 tiles and one", rt, rs))


def test_a_plane_of_many_tiles(sf, engine):
    """300 tiles of one block of trials (two blocks of the list's scan), six blocks of trials in three of segments (more
    than the four row groups a workgroup adds up at once), and 3 x 100 tiles: the list is cut by max_cand inside a tile"""
    for T, S, seed in ((1, 64 * 300 - 5, 1), (64 * 5 + 1, 130, 2), (130, 64 * 100, 3)):
        case = ref.random_case(T, 1, S, seed, blobs=30)
        want = _check(sf, engine, case, 2.0, 1, 1, name=(T, S), rich=True)[0]
        assert sf.geometry(case[3], 64, 1, 1, T, case[5])[1][1] == -(-T // 64) * -(-S // 64) >= 18
        assert len(want) > 300
        _check(sf, engine, case, 2.0, 1, 1, max_cand=len(want) // 2, name=(T, S, "half"))


# ---- planted cases --------------------------------------------------------------------------------------------------

def _flat(T, S, base=6.0, seg=64, tail=None):
    """one width of 2, every segment's mean 3 and variance 4: a peak of 6 scores +0.0, equal peaks score equal bits"""
    nout = (S - 1) * seg + (seg if tail is None else tail)
    at = (np.arange(T * S, dtype=np.int32) * 7 % seg).reshape(T, 1, S) + (np.arange(S, dtype=np.int32) * seg)[None, None, :]
    return [np.full((T, 1, S), base, np.float32), at, ref.flat_moments(T, seg, nout), W1, seg, nout]


def test_every_arm_of_the_tie_rule(sf, engine):
    """equal scores at neighbouring t (the smaller t survives), at neighbouring s (the smaller s), and diagonally (the
    smaller t, though its s is the larger); across a tile's border too"""
    case = _flat(70, 70)
    pairs = [((10, 10), (11, 10)), ((20, 20), (20, 21)), ((30, 31), (31, 30)), ((63, 40), (64, 40)), ((40, 63), (40, 64)), ((63, 64), (64, 63))]
    for a, b in pairs:
        case[0][a[0], 0, a[1]] = case[0][b[0], 0, b[1]] = 20.0
    want = _check(sf, engine, case, 1.0, 1, 1, name="ties")[0]
    assert sorted((int(c[0]), int(c[1])) for c in want) == sorted(a for a, _ in pairs) and np.all(want[:, 6] == 2)
    assert len(_check(sf, engine, case, 1.0, 0, 0, name="ties, no box")[0]) == 12


def test_zeros_of_either_sign_are_equal(sf, engine):
    peak, at, mom, widths, seg, nout = _flat(8, 8, base=-1.0)
    mom[:, :, 0] = 0.0                                            # mean 0: the score of a peak of +-0.0 is +-0.0
    for (t, s), v in (((1, 1), -0.0), ((1, 2), 0.0), ((4, 4), 0.0), ((5, 4), -0.0), ((6, 1), -0.0)):
        peak[t, 0, s] = v
    want, count, score, _ = _check(sf, engine, (peak, at, mom, widths, seg, nout), 0.0, 1, 1, name="zeros")
    assert count.tolist() == [3, 5] and [(int(c[0]), int(c[1]), int(c[4])) for c in want] == [(1, 1, 0x80000000), (6, 1, 0x80000000), (4, 4, 0)]
    want = _check(sf, engine, (peak, at, mom, widths, seg, nout), -0.0, 1, 1, name="zeros, threshold -0.0")[0]
    assert len(want) == 3


def test_peaks_and_segments_that_do_not_score(sf, engine):
    """peaks of -Inf and NaN, a segment of constant samples, a last segment of one output: the score is -Inf, and where
    no width scores the event is (-Inf, 0, -1), which a threshold of -Inf keeps"""
    peak, at, mom, widths, seg, nout = ref.random_case(9, 3, 11, 21, tail=1)
    peak[2, 0, 3], peak[2, 1, 3], peak[2, 2, 3] = -np.inf, np.nan, -np.inf
    peak[4, 1, 5], peak[5, 0, 6], peak[6, 2, 2] = np.nan, -np.inf, np.inf
    mom[7, 4] = (64 * 2.5, 64 * 6.25)
    case = (peak, at, mom, widths, seg, nout)
    want, count, score, k_of = _check(sf, engine, case, 1.0, 2, 1, name="special")
    assert np.all(score[:, 10] == ref.NEG_INF) and score[2, 3] == score[7, 4] == ref.NEG_INF and score[6, 2] == np.inf and k_of[2, 3] == 0
    assert np.isfinite(score[4, 5]) and np.isfinite(score[5, 6])
    want, count, _, _ = _check(sf, engine, case, -np.inf, 0, 0, name="special, everything")
    assert count.tolist() == [99, 99]
    unscored = want[want[:, 4] == 0xFF800000]
    assert len(unscored) == 11 and np.all(unscored[:, 2] == 0) and np.all(unscored[:, 3] == 0xFFFFFFFF)
    assert _words(peak[2, 0, 3:4])[0] in unscored[:, 5]
    _check(sf, engine, case, -np.inf, 3, 2, name="special, boxes of -Inf")


def test_a_box_clipped_at_all_four_edges(sf, engine):
    case = _flat(5, 7)
    for t, s in ((0, 0), (0, 6), (4, 0), (4, 6), (2, 3)):
        case[0][t, 0, s] = 20.0 + t + s
    want = _check(sf, engine, case, 0.0, 2, 2, name="corners")[0]
    assert [(int(c[0]), int(c[1]), int(c[6]), int(c[7])) for c in want] == [(0, 0, 9, 2 << 16), (4, 0, 9, 4 << 16 | 2), (2, 3, 25, 4 << 16), (0, 6, 9, 2 << 16), (4, 6, 9, 4 << 16 | 2)]
    want = _check(sf, engine, case, 0.0, 32, 8, name="one box")[0]
    assert [(int(c[0]), int(c[1]), int(c[6]), int(c[7])) for c in want] == [(4, 6, 35, 4 << 16)]


def test_a_maximum_in_the_halo_of_a_tile(sf, engine):
    """an event above the threshold whose only better neighbour lies in the next tile, in t, in s and diagonally, at the
    reach of the radii and one beyond it"""
    case = _flat(130, 130)
    planted = {(63, 10): 20.0, (64, 10): 21.0, (10, 63): 20.0, (10, 64): 21.0, (63, 63): 20.0, (64, 64): 21.0,
               (60, 100): 20.0, (64, 100): 21.0, (100, 62): 20.0, (100, 64): 21.0, (127, 120): 20.0, (128, 122): 21.0, (59, 30): 20.0, (64, 30): 21.0}
    for (t, s), v in planted.items():
        case[0][t, 0, s] = v
    want = _check(sf, engine, case, 1.0, 4, 2, name="halo")[0]
    assert sorted((int(c[0]), int(c[1])) for c in want) == sorted([p for p, v in planted.items() if v == 21.0] + [(59, 30)])
    want = _check(sf, engine, case, 1.0, 32, 8, name="halo, the widest")[0]
    assert (59, 30) not in [(int(c[0]), int(c[1])) for c in want]


def test_max_cand_below_at_and_above_the_number_found(sf, engine):
    case = ref.random_case(40, 4, 33, 7)
    found = len(ref.sift_ref(*case, 2.0, 2, 1)[0])
    assert found >= 8
    for room in (found - 1, found, found + 1, 1):
        _check(sf, engine, case, 2.0, 2, 1, max_cand=room, name=("max_cand", room))


def test_thresholds_of_either_infinity(sf, engine):
    case = ref.random_case(12, 3, 20, 9)
    want, count, _, _ = _check(sf, engine, case, -np.inf, 1, 1, name="-Inf")
    assert count[1] == 240 and len(want) >= 8
    want, count, _, _ = _check(sf, engine, case, np.inf, 1, 1, name="+Inf")
    assert count.tolist() == [0, 0]


# ---- a run's properties ---------------------------------------------------------------------------------------------

def test_two_runs_give_the_same_bytes_and_the_plane_is_optional(sf, engine):
    case = ref.random_case(70, 5, 90, 13)
    a = sf.sift(engine, *case, 1.5, 3, 1, 4096, fill=FILL)
    b = sf.sift(engine, *case, 1.5, 3, 1, 4096, fill=FILL)
    for x, y in zip(a[:4], b[:4]):
        assert np.array_equal(_words(x), _words(y))
    want, count, score, k_of = ref.sift_ref(*case, 1.5, 3, 1)
    cand, cnt = sf.sift(engine, *case, 1.5, 3, 1, 4096)                       # NULL d_score and d_k
    assert np.array_equal(cand, want) and cnt.tolist() == count.tolist()
    cand, cnt, sc, kk = sf.sift(engine, *case, 1.5, 3, 1, 4096, want_plane=True)
    assert np.array_equal(cand, want) and np.array_equal(_words(sc), _words(score)) and np.array_equal(kk, k_of)


def _series(T, n, seed, pulses):
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((T, n)).astype(np.float32)
    for t, at, amp in pulses:
        for dt in range(-3, 4):
            if 0 <= t + dt < T:
                x[t + dt, at:at + 4] += np.float32(amp / (1 + abs(dt)))
    return x


def test_behind_engine_pulse(sf, engine):
    """what Engine.pulse gives for noise and four pulses, sifted, against the restatement over those arrays"""
    widths, seg, nout = np.array([1, 2, 4, 8, 16], np.int32), 64, 64 * 30 + 9
    x = _series(12, nout + 15, 31, [(3, 222, 18.0), (8, 990, 14.0), (5, 1502, 16.0), (11, 1886, 18.0)])
    peak, at, mom = engine.pulse(x, widths, seg, nout=nout)
    want = _check(sf, engine, (peak, at, mom, widths, seg, nout), 6.0, 4, 1, name="pulse")[0]
    assert [(int(c[0]), int(c[1])) for c in want] == [(3, 3), (8, 15), (5, 23), (11, 29)]
    assert np.all(want[:, 6] >= 3) and np.all(want[:, 3] // seg == want[:, 1]) and np.all(want[:3, 7] >> 16 > want[:3, 0]) and np.all((want[:, 7] & 0xFFFF) < want[:, 0])


def test_chained_on_the_device_with_no_copy(sf, built, engine):
    """rtlws_pulse_run and rtlws_sift_run over the same device buffers, the moments 8 bytes off a multiple of 16; the plan
    serves a second shape"""
    widths, seg = np.array([1, 3, 4], np.int32), 64
    pplan, splan = built.PulsePlan(engine, widths, seg), sf.SiftPlan(engine, widths, seg, 2, 1)
    bufs = []
    try:
        for T, nout, seed in ((7, 64 * 9 + 1, 41), (66, 64 * 70, 42)):
            S = -(-nout // seg)
            x = _series(T, nout + 3, seed, [(T // 2, 130, 9.0), (1, 64 * 5 + 7, 8.0)])
            x = np.concatenate([x, np.zeros((T, -x.shape[1] % 4), np.float32)], axis=1)
            d_x, d_peak, d_at = engine.upload(x), engine.alloc(T * 3 * S * 4), engine.alloc(T * 3 * S * 4)
            d_mom, d_work = engine.alloc(T * S * 16 + 16), engine.alloc(splan.work_bytes(T, nout))
            d_cand, d_count = engine.upload(np.full(64 * 8, FILL_BITS, np.uint32)), engine.alloc(8)
            bufs += [d_x, d_peak, d_at, d_mom, d_work, d_cand, d_count]
            assert d_mom.ptr % 16 == 0
            pplan.run(d_x, x.shape[1], T, nout, d_peak, d_at, d_mom.ptr + 8)
            splan.run(d_peak, d_at, d_mom.ptr + 8, T, nout, 5.5, 64, d_work, d_cand, d_count)
            engine.sync()
            peak, at = engine.download(d_peak, np.float32, (T, 3, S)), engine.download(d_at, np.int32, (T, 3, S))
            mom = engine.download(d_mom, np.float64, (T * S * 2 + 2,))[1:-1].reshape(T, S, 2)
            want, count, _, _ = ref.sift_ref(peak, at, mom, widths, seg, nout, 5.5, 2, 1)
            cand, cnt = engine.download(d_cand, np.uint32, (64, 8)), engine.download(d_count, np.int32, (2,))
            assert 2 <= len(want) <= 64 and cnt.tolist() == count.tolist()
            assert np.array_equal(cand[:len(want)], want) and np.all(cand[len(want):] == FILL_BITS), (T, nout)
            assert {(T // 2, 2), (1, 5)} <= {(int(c[0]), int(c[1])) for c in want}
    finally:
        for b in bufs:
            b.free()
        pplan.close()
        splan.close()


def test_capture_and_replay(sf, built):
    """tests/test_graph_gpu.py's pattern for this plan: the three launches of rtlws_sift_run captured on a side stream
    enqueue nothing; replays give the restatement's words, twice.  The process's queue settings are as they were"""
    import torch
    eng = built.Engine(0)
    case = ref.random_case(70, 3, 66, 17)
    peak, at, mom, widths, seg, nout = case
    want, count, score, _ = ref.sift_ref(*case, 2.0, 2, 2)
    dev = torch.device("cuda", 0)
    d_peak, d_at, d_mom = (torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in (peak, at, mom))
    plan = sf.SiftPlan(eng, widths, seg, 2, 2)
    work = torch.zeros(plan.work_bytes(70, nout) // 4, dtype=torch.int32, device=dev)
    cand, cnt = torch.zeros(len(want) * 8 + 8, dtype=torch.int32, device=dev), torch.zeros(2, dtype=torch.int32, device=dev)
    plane = torch.zeros(70 * 66, dtype=torch.float32, device=dev)
    g, side = torch.cuda.CUDAGraph(), torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        with torch.cuda.graph(g, stream=side):
            plan.run(d_peak.data_ptr(), d_at.data_ptr(), d_mom.data_ptr(), 70, nout, 2.0, len(want) + 1, work.data_ptr(), cand.data_ptr(), cnt.data_ptr(),
                     plane.data_ptr(), None, stream=built.torch_stream_handle())
    torch.cuda.current_stream().wait_stream(side)
    assert int(cand.abs().sum()) == 0 and int(cnt.abs().sum()) == 0 and float(plane.abs().sum()) == 0.0      # capture enqueued nothing
    for _ in range(2):
        cand.zero_(), cnt.zero_(), plane.zero_(), work.zero_()
        g.replay()
        torch.cuda.synchronize()
        got = cand.cpu().numpy().view(np.uint32)
        assert cnt.cpu().numpy().tolist() == count.tolist() and np.array_equal(got[:len(want) * 8].reshape(-1, 8), want) and not got[len(want) * 8:].any()
        assert np.array_equal(_words(plane.cpu().numpy()), _words(score).reshape(-1))
    plan.close()
    eng.close()


def test_a_run_s_refusals_behind_the_plan(sf, engine):
    """with a plan every earlier refusal still comes first, and none of them has touched the device's buffers"""
    plan = sf.SiftPlan(engine, W1, 64, 1, 1)
    d = engine.upload(np.full(64, FILL_BITS, np.uint32))
    try:
        run = lambda **kw: plan.run(*[kw.get(n, v) for n, v in (("peak", d), ("at", d), ("mom", d), ("T", 1), ("nout", 64), ("thr", 1.0), ("room", 1), ("work", d), ("cand", d),
                                                                   ("count", d))], check=False)
        for kw, text in ((dict(T=0, nout=0), "ntrials must be 1 .. 65536"), (dict(nout=0, thr=float("nan")), "nout must be 1 .. 2^30"), (dict(thr=float("nan"), room=0), "threshold must not be NaN"),
                         (dict(room=0, peak=None), "max_cand must be 1 .. 16777216"), (dict(count=None, mom=d.ptr + 4), "null pointer"),
                         (dict(mom=d.ptr + 4, work=d.ptr + 8), "d_mom must be 8-byte aligned"), (dict(work=d.ptr + 8, cand=d.ptr + 8), "d_work must be 16-byte aligned"),
                         (dict(cand=d.ptr + 8), "d_cand must be 16-byte aligned"), (dict(T=128, nout=1 << 30), "more than 2^31 - 1 events")):
            assert run(**kw) == -1 and sf.last_error().startswith("rtlws_sift_run: " + text), (kw, sf.last_error())
        assert plan.work_bytes(128, 1 << 30) == -1 and "more than 2^31 - 1 events" in sf.last_error()
        assert plan.work_bytes(5, 64 * 7) == 2 * 144 + 256 + 16
        engine.sync()
        assert np.all(engine.download(d, np.uint32, (64,)) == FILL_BITS)
    finally:
        d.free()
        plan.close()


# ---- end to end ------------------------------------------------------------------------------------------------------

def test_one_dispersed_pulse_end_to_end(sf, built, engine):
    """a pulse swept across 64 channels at trial 20 of 33 in noise: Engine.dedisp, Engine.pulse and the sift give exactly
    one candidate, at the pulse's trial and segment, with its extent in trials around it"""
    M, T, t0, row0, seg = 64, 33, 20, 700, 128
    delays = built.dedisp_delays(M, 1, 150e6, 8e6, 1e-3, T, 0.0, 0.5)
    rng = np.random.default_rng(5)
    rows = rng.standard_normal((1400 + int(delays.max()), M)).astype(np.float32)
    for w in range(3):
        rows[row0 + w + delays[t0], np.arange(M)] += np.float32(2.0)
    series = engine.dedisp(rows, delays, nout=1400)
    widths = np.array([1, 2, 4, 8], np.int32)
    nout = 1400 - 7
    peak, at, mom = engine.pulse(series, widths, seg, nout=nout)
    cand, count = sf.sift(engine, peak, at, mom, widths, seg, nout, 5.0, 32, 2, 16)
    want = ref.sift_ref(peak, at, mom, widths, seg, nout, 5.0, 32, 2)[0]
    assert np.array_equal(cand, want) and count[0] == 1 and count[1] >= 3
    t, s, k, where, _, _, members, extent = (int(v) for v in cand[0])
    assert (t, s) == (t0, row0 // seg) and abs(where - row0) <= 2 and widths[k] in (2, 4) and members == count[1]
    assert (extent & 0xFFFF) < t0 < (extent >> 16)

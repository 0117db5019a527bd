"""GPU suite of include/rtlws_cutout.h (librtlws_cutout.so) against its numpy restatement (tests/cutout_ref.py): every word
of d_ft, d_dmt and d_info, bit for bit.  Every case runs with the outputs preset to a pattern: the words behind the served
candidates and the guard words behind every buffer still hold it afterwards.  The rows are seeded noise with a few planted
dispersed pulses, the lists hand-written except where the real chain (dedispersion, pulse search, sift) is wanted."""
import numpy as np
import pytest

import cutout_ref as ref

pytestmark = pytest.mark.gpu

FILL = np.array([0x7FC5A5A5], np.uint32).view(np.float32)[0]          # a quiet NaN with a payload: the preset pattern
FILL_BITS = np.uint32(0x7FC5A5A5)
W3, B3 = np.array([1, 2, 5], np.int32), np.array([1, 3, 16], np.int32)


@pytest.fixture(scope="module")
def co(built):
    import rtlws.cutout
    return rtlws.cutout


def _words(a):
    return np.ascontiguousarray(a).view(np.uint32).reshape(-1)


class Case:
    """a waterfall, its table and mask, the series of every trial, and the planes' extents"""

    def __init__(self, nchan, ntrials, nsamp, seed, nx=8, nf=1, rq=1, dq=1, widths=W3, bins=B3, dmax=9, delays=None, mask=None, series="noise"):
        rng = np.random.default_rng(seed)
        self.delays = rng.integers(0, dmax + 1, (ntrials, nchan)).astype(np.int32) if delays is None else np.asarray(delays, np.int32)
        self.mask = mask
        kept = self.delays if mask is None else self.delays[:, np.asarray(mask) != 0]
        self.rows = ref.waterfall(nsamp + (int(kept.max()) if kept.size else 0), nchan, seed + 1000)
        # the series are D of the header where that is what the case is about; else noise of their own, which is a series too
        self.series = ref.dedisp(self.rows, self.delays, mask, nsamp) if series == "dedisp" else ref.waterfall(ntrials, nsamp, seed + 2000)
        self.nchan, self.ntrials, self.nsamp, self.nx, self.nf, self.rq, self.dq, self.widths, self.bins = nchan, ntrials, nsamp, nx, nf, rq, dq, widths, bins

    def args(self):
        return self.delays, self.mask, self.widths, self.bins, self.nx, self.nf, self.rq, self.dq


def _check(co, engine, c, entries, count=None, max_cand=None, want_ft=True, want_dmt=True, name=None):
    """one run through rtlws.cutout.cutout with `fill` against the restatement -> the restatement's (F, G, info)"""
    count = [len(entries) if count is None else count, 12345]
    room = max(len(entries), 1) + 2 if max_cand is None else max_cand
    cand = ref.list_of(entries, room)                             # max_cand long, as the sift's d_cand is
    F, G, info = ref.cutout_ref(c.rows if want_ft else None, c.series if want_dmt else None, cand, count, *c.args(), c.nsamp, room)
    ft, dmt, inf = co.cutout(engine, c.rows if want_ft else None, c.series if want_dmt else None, cand, count, *c.args(), nsamp=c.nsamp, max_cand=room,
                             want_ft=want_ft, want_dmt=want_dmt, fill=FILL)
    m, ndm = len(info), 2 * c.rq + 1
    assert m == min(max(count[0], 0), room)
    assert ft.shape == (room * c.nf * c.nx + co.GUARD,) and dmt.shape == (room * ndm * c.nx + co.GUARD,) and inf.shape == (room * 4 + co.GUARD,), name
    assert np.array_equal(inf[:m * 4].reshape(m, 4), info), (name, inf[:m * 4].reshape(m, 4), info)
    assert np.all(_words(inf[m * 4:]) == FILL_BITS), (name, "behind the info")
    for got, want, per, what in ((ft, F, c.nf * c.nx, "band-time"), (dmt, G, ndm * c.nx, "DM-time")):
        if want is None:
            assert np.all(_words(got) == FILL_BITS), (name, what, "a NULL output was touched")
            continue
        bad = np.flatnonzero(_words(got[:m * per]) != _words(want))
        assert bad.size == 0, (name, what, "%d words differ, the first at (i, row, x) = %s: %r against %r"
                               % (bad.size, np.unravel_index(bad[0], want.shape), got[bad[0]], want.reshape(-1)[bad[0]]))
        assert np.all(_words(got[m * per:]) == FILL_BITS), (name, what, "behind the served candidates")
    return F, G, info


# ---- the layout in channels ----------------------------------------------------------------------------------------------

# (nchan, nf): cpb = 1 at every nchan; one subband of the whole band below, at and above the tile's 256 channels (the chunk
# walk and its carried sums: 260 = 256 + 4, 1028 = 4 * 256 + 4, and 257 = 256 + 1 four times); cpb 2, 3, 4, 65 (three
# subbands a workgroup, 61 lanes idle) and 128 (two)
CHANNELS = [(4, 4), (12, 12), (64, 64), (256, 256), (260, 260), (1028, 1028), (260, 1), (1028, 1), (256, 1), (1028, 4), (12, 6), (12, 4), (64, 16), (260, 4), (256, 2)]


@pytest.mark.parametrize("nchan,nf", CHANNELS, ids=["%d-in-%d" % c for c in CHANNELS])
def test_the_layout_in_channels(co, engine, nchan, nf):
    c = Case(nchan, 3, 60, nchan * 7 + nf, nx=8, nf=nf, dmax=5)
    per = 256 // (nchan // nf) if nchan // nf <= 256 else 1
    assert co.geometry(*c.args(), 2)[1][0] == 2 * -(-nf // per)
    F, G, info = _check(co, engine, c, [(1, 0, 30), (2, 1, 7), (0, 2, 58)], name=(nchan, nf))
    assert info[:, 2].tolist() == [1, 1, 1] and F.any() and np.all(np.isfinite(F))
    if nf == nchan:                                               # cpb = 1: F is R, the rows of a bin of one channel
        assert F[0, nchan - 1, 3] == c.rows[30 - 4 + 3 + c.delays[1, nchan - 1], nchan - 1]


def test_the_channel_sum_is_in_ascending_channel(co, engine):
    """values that any other order adds to other bits: 2^24 first, then ones that it swallows one by one, in one subband of
    one workgroup (cpb 64), across the lanes of a chunk and across two chunks (cpb 260)"""
    for nchan, nf in ((64, 1), (260, 1), (128, 2)):
        c = Case(nchan, 1, 20, 5, nx=4, nf=nf, dmax=0, bins=[1, 1, 1])
        c.rows[:] = np.float32(1.0)
        c.rows[:, 0] = np.float32(2.0 ** 24)
        c.rows[:, nchan - 1] = np.float32(-(2.0 ** 24))
        F, _, _ = _check(co, engine, c, [(0, 0, 10)], want_dmt=False, name=("order", nchan, nf))
        assert F[0, 0, 0] == (0.0 if nf == 1 else 2.0 ** 24) and F[0, nf - 1, 0] == (0.0 if nf == 1 else 63.0 - 2.0 ** 24)


# ---- the layout in time -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("nx", [4, 32, 36, 256])
def test_the_layout_in_time(co, engine, nx):
    """nx below, at and across the group of 32 bins, bins of 1, 3 and 16 rows for the three widths of one list"""
    c = Case(12, 3, 16 * nx + 50, nx, nx=nx, nf=3, rq=1)
    mid = c.nsamp // 2
    entries = [(0, 0, mid), (1, 1, mid + 1), (2, 2, mid - 3), (1, 2, 5), (0, 1, c.nsamp - 1)]
    F, G, info = _check(co, engine, c, entries, name=("nx", nx))
    assert info[:, 1].tolist() == [1, 3, 16, 16, 3] and info[2, 3] == 16 * nx and info[0].tolist() == [mid - nx // 2, 1, 1, nx]
    assert co.geometry(*c.args(), 5)[1] == (5 * -(-nx // 32), 5 * 3) and co.geometry(*c.args(), 5)[2] == (256, -(-nx // 64) * 64)


# ---- windows ------------------------------------------------------------------------------------------------------------------

def test_windows_over_the_borders(co, engine):
    """hanging over row 0, over nsamp, over both (nsamp < nx b), lying behind the series altogether; info's count of rows"""
    widths, bins = np.array([1, 4, 9, 200], np.int32), np.array([1, 2, 5, 1], np.int32)
    c = Case(16, 4, 70, 11, nx=36, nf=4, rq=2, widths=widths, bins=bins, series="dedisp")
    entries = [(0, 0, 0), (1, 0, 69), (2, 1, 3), (3, 1, 66), (1, 2, 35), (0, 2, 0), (3, 2, 69), (2, 3, 60), (2, 0, 35)]
    F, G, info = _check(co, engine, c, entries, name="borders")
    want = [ref.window(at, int(widths[k]), int(bins[k]), 36, 70) for _, k, at in entries]
    assert info[:, 0].tolist() == [w[0] for w in want] and info[:, 3].tolist() == [w[1] for w in want]
    assert info[:, 3].tolist() == [18, 19, 41, 38, 70, 70, 70, 0, 36] and info[7].tolist() == [142, 1, 1, 0]
    assert not F[7].view(np.uint32).any() and not G[7].view(np.uint32).any()      # valid, and nothing of it inside
    assert not F[0, :, :18].view(np.uint32).any() and F[0, :, 18:].all() and not F[1, :, 19:].view(np.uint32).any() and F[1, :, :19].all()
    small = Case(8, 2, 5, 12, nx=4, nf=2, rq=1, bins=[1, 3, 16])          # a series shorter than one bin
    _, _, info = _check(co, engine, small, [(0, 2, 2), (1, 1, 4), (0, 0, 0)], name="nsamp 5")
    assert info[:, 3].tolist() == [5, 5, 2]


# ---- tables ----------------------------------------------------------------------------------------------------------------

def test_a_dispersion_sweep(co, built, engine):
    M, T = 64, 9
    delays = built.dedisp_delays(M, 1, 150e6, 8e6, 1e-3, T, 0.0, 2.0)
    assert delays.max() > 100
    c = Case(M, T, 300, 13, nx=32, nf=8, rq=2, dq=2, delays=delays)
    for w in range(2):                                            # rows 151 and 152 of trial 4: bin 16 of the window of width 2 at 150
        c.rows[151 + w + delays[4], np.arange(M)] += np.float32(30.0)
    c.series = ref.dedisp(c.rows, delays, None, 300)
    F, G, info = _check(co, engine, c, [(4, 1, 150), (0, 0, 150), (8, 2, 150)], name="sweep")
    assert np.all(F[0].argmax(axis=1) == 16) and G[0, 2].argmax() == 16 and G[0, 2].max() > G[0, 0].max()      # broadband, and the bow tie's knot


def test_a_random_table_with_the_largest_delays(co, engine):
    rng = np.random.default_rng(14)
    delays = rng.integers(0, 65536, (3, 8)).astype(np.int32)
    delays[1, 5], delays[2, 0] = 65535, 0
    c = Case(8, 3, 10, 15, nx=12, nf=2, delays=delays)
    assert co.geometry(*c.args())[-1] == 65535 and c.rows.shape[0] == 10 + 65535
    _check(co, engine, c, [(1, 0, 9), (2, 0, 0), (0, 1, 5)], name="65535")


def test_masks(co, engine):
    """one channel out, a whole subband out (its plane is +0.0), all out; a masked channel's rows are not there to read: the
    waterfall ends where the kept channels' delays end"""
    for which in ("one", "subband", "all"):
        mask = np.ones(16, np.uint8)
        mask[{"one": slice(5, 6), "subband": slice(4, 8), "all": slice(0, 16)}[which]] = 0
        delays = np.random.default_rng(16).integers(0, 6, (3, 16)).astype(np.int32)
        delays[:, mask == 0] = 40000                              # rows that do not exist
        c = Case(16, 3, 50, 17, nx=8, nf=4, delays=delays, mask=mask)
        assert c.rows.shape[0] <= 55 and co.geometry(*c.args())[-1] == (0 if which == "all" else 5)
        F, _, info = _check(co, engine, c, [(0, 0, 25), (2, 1, 49)], name=("mask", which))
        assert not F[:, 1].view(np.uint32).any() if which != "one" else F[0, 1].all()
        assert F.any() == (which != "all") and info[:, 2].tolist() == [1, 1]


# ---- the list ---------------------------------------------------------------------------------------------------------------

def test_the_count_and_max_cand(co, engine):
    """d_count[0] = 0 (nothing is written at all), 1, max_cand and above it, a negative count; max_cand = 1"""
    c = Case(12, 4, 80, 18, nx=8, nf=3)
    entries = [(t % 4, t % 3, 10 + 9 * t) for t in range(6)]
    for count, room in ((0, 6), (1, 6), (6, 6), (6, 4), (4096, 5), (6, 1), (-1, 6), (1, 1), (3, 4096)):
        _, _, info = _check(co, engine, c, entries, count=count, max_cand=room, name=("count", count, room))
        assert len(info) == max(min(count, room), 0)


def test_invalid_candidates(co, engine):
    """t, k and at below and above their ranges (-1 among them): zero planes, zero info, the valid ones between them served"""
    c = Case(12, 4, 80, 19, nx=8, nf=3)
    entries = [(-1, 0, 40), (1, 0, 40), (4, 0, 40), (1, -1, 40), (1, 3, 40), (1, 2, 40), (1, 0, -1), (1, 0, 80), (1, 0, 79), (-(1 << 31), 0, 0), (0, 1 << 30, 0),
               (0, 0, (1 << 31) - 1)]
    F, G, info = _check(co, engine, c, entries, name="invalid")
    assert info[:, 2].tolist() == [0, 1, 0, 0, 0, 1, 0, 0, 1, 0, 0, 0]
    for i in np.flatnonzero(info[:, 2] == 0):
        assert not F[i].view(np.uint32).any() and not G[i].view(np.uint32).any() and not info[i].any()


# ---- the DM-time plane -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("rq,dq", [(0, 1), (2, 1), (2, 7), (64, 1), (64, 7)])
def test_the_dm_time_plane(co, engine, rq, dq):
    """the rows at trials t + (r - rq) dq; those below 0 and above ntrials - 1 are +0.0"""
    c = Case(8, 40, 90, 20 + rq + dq, nx=12, nf=2, rq=rq, dq=dq)
    entries = [(0, 0, 45), (39, 1, 45), (20, 2, 45), (13, 0, 2)]
    _, G, _ = _check(co, engine, c, entries, name=("rq", rq, dq))
    for i, (t, _, _) in enumerate(entries):
        q = t + (np.arange(2 * rq + 1) - rq) * dq
        inside = (q >= 0) & (q < 40)
        assert not G[i, ~inside].view(np.uint32).any() and np.all(G[i, inside].any(axis=1)) and G[i, rq].any()


def test_null_outputs(co, engine):
    """d_ft or d_dmt NULL (and what only it reads with it): the other plane is what it was, the NULL one untouched"""
    c = Case(64, 5, 80, 23, nx=36, nf=8, rq=2)
    entries = [(2, 0, 40), (4, 2, 70), (9, 0, 1)]
    F, G, info = _check(co, engine, c, entries, name="both")
    F1, G1, info1 = _check(co, engine, c, entries, want_dmt=False, name="no d_dmt")
    F2, G2, info2 = _check(co, engine, c, entries, want_ft=False, name="no d_ft")
    assert G1 is None and F2 is None and np.array_equal(_words(F1), _words(F)) and np.array_equal(_words(G2), _words(G))
    assert np.array_equal(info1, info) and np.array_equal(info2, info)


# ---- the two ties to rtlws_dedisp_run -----------------------------------------------------------------------------------------

def test_the_ties_to_the_dedispersion(co, engine):
    """nf = 1 and b = 1: F[i][0][x] is D[t][n0 + x] of rtlws_dedisp_run bit for bit inside the series; b = 1: G[i][rq][x] is
    that value too, -0.0 turned into +0.0 -- at 64 channels and across the chunks of 260"""
    for nchan in (64, 260):
        c = Case(nchan, 5, 120, 24 + nchan, nx=32, nf=1, rq=1, bins=[1, 1, 1])
        mask = np.ones(nchan, np.uint8)
        mask[3] = 0
        c.mask = mask
        D = engine.dedisp(c.rows, c.delays, mask, nout=120)
        assert np.array_equal(_words(D), _words(ref.dedisp(c.rows, c.delays, mask, 120)))
        c.series = D.copy()
        c.series[2, 61] = np.float32(-0.0)
        entries = [(2, 0, 60), (0, 1, 3), (4, 2, 119)]
        F, G, info = _check(co, engine, c, entries, name=("ties", nchan))
        for i, (t, _, _) in enumerate(entries):
            n = info[i, 0] + np.arange(32)
            ok = (n >= 0) & (n < 120)
            assert np.array_equal(_words(F[i, 0, ok]), _words(D[t, n[ok]])) and 10 < ok.sum() <= 32
            assert np.array_equal(_words(G[i, 1, ok]), _words(c.series[t, n[ok]] + np.float32(0.0)))
        assert np.signbit(c.series[2, 61]) and G[0, 1, 61 - info[0, 0]] == 0.0 and not np.signbit(G[0, 1, 61 - info[0, 0]])


# ---- the real chain --------------------------------------------------------------------------------------------------------------

def test_the_chain_on_the_device(co, built, engine):
    """rtlws_dedisp_run, rtlws_pulse_run, rtlws_sift_run and rtlws_cutout_run over the same device buffers: the list and its
    count are read where the sift left them.  The planted pulse is the brightest bin of row rq of G, and of the band summed over its subbands"""
    import rtlws.sift as sf
    M, T, t0, row0, seg, N = 64, 33, 20, 700, 128, 1400
    delays = built.dedisp_delays(M, 1, 150e6, 8e6, 1e-3, T, 0.0, 0.5)
    rows = np.random.default_rng(5).standard_normal((N + int(delays.max()), M)).astype(np.float32)
    for w in range(3):
        rows[row0 + w + delays[t0], np.arange(M)] += np.float32(2.0)
    widths, bins, nx, nf, rq, room = np.array([1, 2, 4, 8], np.int32), np.array([1, 1, 2, 4], np.int32), 32, 8, 4, 16
    nout = N - 7
    S = -(-nout // seg)
    dplan, pplan = built.DedispPlan(engine, delays), built.PulsePlan(engine, widths, seg)
    splan, cplan = sf.SiftPlan(engine, widths, seg, 32, 2), co.CutoutPlan(engine, delays, None, widths, bins, nx, nf, rq, 3)
    bufs = []
    try:
        d_rows, d_series = engine.upload(rows), engine.alloc(T * N * 4)
        d_peak, d_at, d_mom = engine.alloc(T * 4 * S * 4), engine.alloc(T * 4 * S * 4), engine.alloc(T * S * 16)
        d_work, d_cand, d_count = engine.alloc(splan.work_bytes(T, nout)), engine.upload(np.full(room * 8, FILL_BITS, np.uint32)), engine.alloc(8)
        d_ft, d_dmt = engine.upload(np.full(room * nf * nx, FILL, np.float32)), engine.upload(np.full(room * 9 * nx, FILL, np.float32))
        d_info = engine.upload(np.full(room * 4, FILL_BITS, np.uint32))
        bufs += [d_rows, d_series, d_peak, d_at, d_mom, d_work, d_cand, d_count, d_ft, d_dmt, d_info]
        dplan.run(d_rows, N, d_series, M, N)
        pplan.run(d_series, N, T, nout, d_peak, d_at, d_mom)
        splan.run(d_peak, d_at, d_mom, T, nout, 5.0, room, d_work, d_cand, d_count)
        cplan.run(d_rows, M, d_series, N, N, d_cand, d_count, room, d_ft, d_dmt, d_info)
        engine.sync()
        cand, count = engine.download(d_cand, np.uint32, (room, 8)), engine.download(d_count, np.int32, (2,))
        series = engine.download(d_series, np.float32, (T, N))
        ft, dmt = engine.download(d_ft, np.float32, (room, nf, nx)), engine.download(d_dmt, np.float32, (room, 9, nx))
        info = engine.download(d_info, np.int32, (room, 4))
        assert count[0] == 1 and cand[0, 0] == t0 and abs(int(cand[0, 3]) - row0) <= 2
        F, G, winfo = ref.cutout_ref(rows, series, cand, count, delays, None, widths, bins, nx, nf, rq, 3, N, room)
        assert np.array_equal(_words(ft[:1]), _words(F)) and np.array_equal(_words(dmt[:1]), _words(G)) and np.array_equal(info[:1], winfo)
        assert np.all(_words(ft[1:]) == FILL_BITS) and np.all(_words(dmt[1:]) == FILL_BITS) and np.all(_words(info[1:]) == FILL_BITS)
        n0, b = int(info[0, 0]), int(info[0, 1])
        lit = sorted({(row0 + w - n0) // b for w in range(3)})
        assert int(dmt[0, rq].argmax()) in lit and int(ft[0].sum(axis=0).argmax()) in lit
    finally:
        for buf in bufs:
            buf.free()
        for plan in (dplan, pplan, splan, cplan):
            plan.close()


# ---- non-finite samples, reproducibility, capture -------------------------------------------------------------------------------

def test_non_finite_samples_reach_their_bin_alone(co, engine):
    c = Case(16, 3, 100, 26, nx=12, nf=4, rq=1, bins=[1, 3, 16], dmax=3)
    c.rows[50 + c.delays[1, 6], 6] = np.nan                       # n = 50 of channel 6 under trial 1
    c.rows[53 + c.delays[1, 9], 9] = np.inf
    c.series[1, 50], c.series[1, 53], c.series[2, 50] = np.nan, -np.inf, np.inf
    F, G, info = _check(co, engine, c, [(1, 1, 50)], name="non-finite")
    n0 = int(info[0, 0])
    xa, xb = (50 - n0) // 3, (53 - n0) // 3
    assert xa != xb and np.isnan(F[0, 1, xa]) and np.isinf(F[0, 2, xb])
    F[0, 1, xa] = F[0, 2, xb] = 0.0
    assert np.all(np.isfinite(F))
    assert np.isnan(G[0, 1, xa]) and G[0, 1, xb] == -np.inf and G[0, 2, xa] == np.inf and np.isfinite(G).sum() == G.size - 3


def test_two_runs_give_the_same_bytes(co, engine):
    c = Case(260, 6, 200, 27, nx=36, nf=4, rq=2, dq=2)
    entries = [(t % 6, t % 3, 3 + 17 * t) for t in range(11)]
    cand, count = ref.list_of(entries, 12), [11, 0]
    a = co.cutout(engine, c.rows, c.series, cand, count, *c.args(), nsamp=200, max_cand=12, fill=FILL)
    b = co.cutout(engine, c.rows, c.series, cand, count, *c.args(), nsamp=200, max_cand=12, fill=FILL)
    for x, y in zip(a, b):
        assert np.array_equal(_words(x), _words(y))
    F, G, info = ref.cutout_ref(c.rows, c.series, cand, count, *c.args(), 200, 12)
    ft, dmt, inf = co.cutout(engine, c.rows, c.series, cand, count, *c.args(), nsamp=200, max_cand=12)       # without fill: the served planes, shaped
    assert np.array_equal(_words(ft), _words(F)) and np.array_equal(_words(dmt), _words(G)) and np.array_equal(inf, info)
    assert ft.shape == (11, 4, 36) and dmt.shape == (11, 5, 36) and inf.shape == (11, 4)


def test_capture_and_replay_with_another_count(co, built):
    """tests/test_graph_gpu.py's pattern for this plan: the two launches captured on a side stream enqueue nothing; a replay
    serves d_count[0] as it stands then: 2 candidates, then 5 of the same list with nothing captured again"""
    import torch
    eng = built.Engine(0)
    c = Case(64, 4, 150, 28, nx=36, nf=8, rq=1)
    entries = [(t % 4, t % 3, 20 + 21 * t) for t in range(6)]
    cand = ref.list_of(entries)
    dev = torch.device("cuda", 0)
    d_rows, d_series = torch.from_numpy(c.rows).to(dev), torch.from_numpy(np.ascontiguousarray(c.series)).to(dev)
    d_cand, d_count = torch.from_numpy(cand.view(np.int32)).to(dev), torch.zeros(2, dtype=torch.int32, device=dev)
    plan = co.CutoutPlan(eng, *c.args())
    ft, dmt = torch.zeros(6 * 8 * 36, dtype=torch.float32, device=dev), torch.zeros(6 * 3 * 36, dtype=torch.float32, device=dev)
    info = torch.zeros(6 * 4, dtype=torch.int32, device=dev)
    d_count[0] = 6
    g, side = torch.cuda.CUDAGraph(), torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        with torch.cuda.graph(g, stream=side):
            plan.run(d_rows.data_ptr(), 64, d_series.data_ptr(), 150, 150, d_cand.data_ptr(), d_count.data_ptr(), 6, ft.data_ptr(), dmt.data_ptr(), info.data_ptr(),
                     stream=built.torch_stream_handle())
    torch.cuda.current_stream().wait_stream(side)
    assert float(ft.abs().sum()) == 0.0 and float(dmt.abs().sum()) == 0.0 and int(info.abs().sum()) == 0      # capture enqueued nothing
    for served in (2, 5):
        ft.zero_(), dmt.zero_(), info.zero_()
        d_count[0] = served
        g.replay()
        torch.cuda.synchronize()
        F, G, winfo = ref.cutout_ref(c.rows, c.series, cand, [served, 0], *c.args(), 150, 6)
        got_f, got_g, got_i = ft.cpu().numpy().reshape(6, 8, 36), dmt.cpu().numpy().reshape(6, 3, 36), info.cpu().numpy().reshape(6, 4)
        assert np.array_equal(_words(got_f[:served]), _words(F)) and np.array_equal(_words(got_g[:served]), _words(G)) and np.array_equal(got_i[:served], winfo)
        assert not _words(got_f[served:]).any() and not _words(got_g[served:]).any() and not got_i[served:].any()
    plan.close()
    eng.close()


def test_a_run_s_refusals_behind_the_plan(co, engine):
    """with a plan every earlier refusal still comes first, in_stride below nchan is the plan's to refuse, and none of them
    has touched the device's buffers"""
    plan = co.CutoutPlan(engine, np.zeros((2, 8), np.int32), None, W3, B3, 4, 2, 1, 1)
    d = engine.upload(np.full(64, FILL_BITS, np.uint32))
    try:
        run = lambda **kw: plan.run(*[kw.get(n, v) for n, v in (("rows", d), ("in_stride", 8), ("series", d), ("stride", 8), ("nsamp", 8), ("cand", d), ("count", d),
                                                                   ("room", 1), ("ft", d), ("dmt", d), ("info", d))], check=False)
        for kw, text in ((dict(nsamp=0, room=0), "nsamp must be 1 .. 2^30"), (dict(room=0, in_stride=2), "max_cand must be 1 .. 4096"),
                         (dict(in_stride=6, stride=4), "in_stride must be >= 4 and a multiple of 4"), (dict(stride=7, ft=None, dmt=None), "series_stride must be >= nsamp"),
                         (dict(ft=None, dmt=None, cand=None), "d_ft and d_dmt must not both be NULL"), (dict(cand=None, rows=d.ptr + 8), "null pointer"),
                         (dict(dmt=None, series=None, rows=None), "null pointer"), (dict(rows=d.ptr + 8, cand=d.ptr + 8), "d_rows must be 16-byte aligned"),
                         (dict(cand=d.ptr + 8, in_stride=4), "d_cand must be 16-byte aligned"), (dict(in_stride=4), "in_stride must be >= nchan")):
            assert run(**kw) == -1 and co.last_error().startswith("rtlws_cutout_run: " + text), (kw, co.last_error())
        assert plan.rows_needed(8) == 8 and plan.rows_needed(0) == -1
        engine.sync()
        assert np.all(engine.download(d, np.uint32, (64,)) == FILL_BITS)
    finally:
        d.free()
        plan.close()

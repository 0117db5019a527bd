"""GPU suite of include/rtlws_fold.h (librtlws_fold.so) against its numpy restatement (tests/fold_ref.py): profiles on
uint32 views with NaN by place, hits exactly; NaN in the stride's padding and behind nsamp, a preset pattern behind both
outputs; signed data with exponents over 2^-6 .. 2^6.  Every block shape at every border of the tile and the
sub-integration, special steps and phases, planted samples, zeros, subnormals, NaN and infinities, the trial counts up
to the limit, a NULL d_hits, a run from a later sub-integration, one plan many times and beside another, graph capture,
and the chain spectrometer -> dedispersion -> folding (with the pulse search's moments) on the device."""
import numpy as np
import pytest

import dedisp_ref
import fold_ref
import pulse_ref

pytestmark = pytest.mark.gpu

FILL = np.float32(-12345.678)
T = fold_ref.TILE
NBINS = (2, 3, 64, 65, 128, 129, 255, 256)
NPERIODS = (1, 63, 64, 65, 129)
NSAMPS = ("1", "T-1", "T", "T+1", "2T+5")
SUBS = ("64", "68", "T", "T+4", "2T+4", ">nsamp")
SIZES = {"1": 1, "T-1": T - 1, "T": T, "T+1": T + 1, "2T+5": 2 * T + 5, "64": 64, "68": 68, "T+4": T + 4, "2T+4": 2 * T + 4}
M64 = 1 << 64


def _size(code, nsamp=None):
    if code == ">nsamp":
        return max(64, (nsamp + 4 + 3) // 4 * 4)
    return SIZES[code]


def _same_bits(got, want, what=None):
    """bit for bit on uint32 views, NaN by place (the default NaN of the host's additions and the device's may differ)"""
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape)
    nan = np.isnan(want) if got.dtype.kind == "f" else np.zeros(want.shape, bool)
    gnan = np.isnan(got) if got.dtype.kind == "f" else nan
    bad = (gnan != nan) | (~nan & (got.view(np.uint32) != want.view(np.uint32)))
    assert not bad.any(), (what, np.argwhere(bad)[:5], got[bad][:5], want[bad][:5])


def _run(built, engine, x, steps, phases, nbins, sub, nsamp=None, want_hits=True, name=None):
    """x float32 [ntrials, >= nsamp] through Engine.fold with NaN in the padding and behind nsamp and preset guards behind
    the outputs, against the restatement; -> (prof, hits) of the device"""
    ntrials, nper = x.shape[0], len(steps)
    nsamp = x.shape[1] if nsamp is None else nsamp
    nsub = fold_ref.subints(nsamp, sub)
    stride = (nsamp + 3) // 4 * 4 + 4
    padded = np.full((ntrials, stride), np.nan, np.float32)
    padded[:, :nsamp] = x[:, :nsamp]
    prof, hits = engine.fold(padded, steps, phases, nbins, sub, nsamp=nsamp, in_stride=stride, want_hits=want_hits, fill=FILL)
    n1, n2, guard = ntrials * nper * nsub * nbins, nper * nsub * nbins, built.FOLD_GUARD
    assert prof.shape == (n1 + guard,) and hits.shape == (n2 + guard,) and hits.dtype == np.uint32
    assert np.all(prof[n1:].view(np.uint32) == FILL.view(np.uint32)) and np.all(hits[n2:] == FILL.view(np.uint32)), name
    prof, hits = prof[:n1].reshape(ntrials, nper, nsub, nbins), hits[:n2].reshape(nper, nsub, nbins)
    want_prof, want = fold_ref.fold_ref(x, steps, phases, nbins, sub, nsamp)
    _same_bits(prof, want_prof, (name, "prof"))
    if want_hits:
        assert np.array_equal(hits, want), (name, np.argwhere(hits != want)[:5])
        lens = np.minimum(sub, nsamp - sub * np.arange(nsub))
        assert np.all(hits.sum(axis=2) == lens[None, :]), name
    else:
        assert np.all(hits == FILL.view(np.uint32)), name
    return prof, hits


def test_the_cases_cover_the_borders(built):
    """The shapes of test_every_block_shape_at_every_border: all three waves_per_block, a wavefront with idle lanes and a
    whole idle wavefront, tiles of one sample and of `tile`, a last sub-integration of one sample, and sub above nsamp"""
    shapes = set()
    for nbins in NBINS:
        rc, _, threads, lds, tile, wpb, _ = built.fold_geometry(1, nbins, 64)
        assert rc == 0 and tile == T and threads == 64 * wpb and lds == wpb * nbins * 256 <= 65536
        shapes.add(wpb)
    assert shapes == {4, 2, 1}
    assert any(n % 64 for n in NPERIODS) and any(n % 64 == 0 for n in NPERIODS)           # idle lanes, and none
    assert any(-(-n // 64) % 4 for n in NPERIODS)                                        # a workgroup with a whole wavefront behind the table
    assert _size("T+1") % _size("T") == 1 and _size("2T+5") % _size("68") == 65        # a last sub-integration of one sample; one of a tile and one
    assert _size(">nsamp", 5) > 5 and _size(">nsamp", 2 * T + 5) > 2 * T + 5 and _size(">nsamp", 2 * T + 5) % 4 == 0
    assert all(_size(s, 1) % 4 == 0 and _size(s, 1) >= 64 for s in SUBS)


@pytest.mark.parametrize("nperiods", NPERIODS)
@pytest.mark.parametrize("nbins", NBINS)
def test_every_block_shape_at_every_border(built, engine, nbins, nperiods):
    seed = NBINS.index(nbins) * 10 + NPERIODS.index(nperiods)
    steps, phases = fold_ref.table(nperiods, seed)
    x = fold_ref.signed_series(2, 2 * T + 5, seed)
    for nsamp_code in NSAMPS:
        nsamp = _size(nsamp_code)
        for sub_code in SUBS:
            sub = _size(sub_code, nsamp)
            rc, blocks, threads, lds, tile, wpb, nsub = built.fold_geometry(nperiods, nbins, sub, 2, nsamp)
            assert rc == 0 and (blocks, threads, lds, tile, wpb, nsub) == fold_ref.plan(nperiods, nbins, sub, 2, nsamp)
            _run(built, engine, x, steps, phases, nbins, sub, nsamp, name=(nbins, nperiods, nsamp_code, sub_code))


def test_special_steps_and_phases(built, engine):
    """step 0 (everything in bin(phi0)), 2^63, 2^64 - 1, a period of exactly nbins samples, a phase that wraps exactly at
    a tile border and at a sub-integration border, two equal entries"""
    nbins, sub, nsamp = 16, 2 * T + 4, 3 * (2 * T + 4) + 9
    any_step = fold_ref.step_of(37.3)
    steps = [0, 0, 1 << 63, 1 << 63, M64 - 1, M64 - 1, M64 // nbins, M64 // nbins, any_step, any_step, any_step, 12345, any_step]
    phases = [0, (11 << 60) + 5, 0, (1 << 63) - 1, 0, 77, 0, (1 << 60) - 1, (-T * any_step) % M64, (-sub * any_step) % M64,
              (-(sub + T) * any_step) % M64, M64 - 12345 * sub, (-T * any_step) % M64]
    x = fold_ref.signed_series(2, nsamp, seed=3)
    prof, hits = _run(built, engine, x, steps, phases, nbins, sub, name="special steps")
    lens = np.minimum(sub, nsamp - sub * np.arange(4))
    assert np.all(hits[0, :, 0] == lens) and np.all(hits[1, :, 11] == lens)              # step 0: one bin holds everything
    assert np.all(hits[2, :, 0] + hits[2, :, 8] == lens) and np.all(hits[2, :, 0] == (lens + 1) // 2)
    assert np.all(hits[6, 0] == sub // nbins + (np.arange(16) < sub % nbins))            # a period of nbins samples: bin = n mod 16
    assert fold_ref.bins_of(any_step, phases[8], nbins, T - 1, T + 1).tolist() == [15, 0]  # the wrap between two tiles
    assert fold_ref.bins_of(any_step, phases[9], nbins, sub - 1, sub + 1).tolist() == [15, 0]
    assert fold_ref.bins_of(12345, phases[11], nbins, sub - 1, sub + 1).tolist() == [15, 0]
    _same_bits(prof[:, 8], prof[:, 12], "equal entries")
    assert np.array_equal(hits[8], hits[12])


@pytest.mark.parametrize("nbins", [5, 200])
def test_planted_samples(built, engine, nbins):
    """A sample of 3.0e6 at the first and last n of a sub-integration and of a tile: it lands in the bin the restatement
    says, in the right sub-integration, and nowhere else"""
    sub = 2 * T + 4
    nsamp = 3 * sub
    steps, phases = fold_ref.table(5, seed=11)
    for which, n in enumerate((0, sub - 1, sub, 2 * sub - 1, T - 1, T, sub + T - 1, sub + T, 2 * T + 3, nsamp - 1)):
        x = fold_ref.signed_series(1, nsamp, seed=100 + which)
        x[0, n] = np.float32(3.0e6)
        prof, _ = _run(built, engine, x, steps, phases, nbins, sub, name=(nbins, n))
        big = np.abs(prof[0]) > 1.0e6
        for p in range(5):
            b = int(fold_ref.bins_of(steps[p], phases[p], nbins, n, n + 1)[0])
            assert np.argwhere(big[p]).tolist() == [[n // sub, b]], (n, p)


def test_zeros_subnormals_nan_and_infinities(built, engine):
    nbins, sub, nsamp = 7, 68, 300
    steps, phases = fold_ref.table(4, seed=21)
    x = fold_ref.signed_series(6, nsamp, seed=22)
    x[0, :] = -0.0                                               # every sum is +0.0 + -0.0 .. = +0.0
    x[1, :] = np.float32(2.0 ** -149) * np.arange(1, nsamp + 1).astype(np.float32)       # subnormals only: their sums stay subnormal, and exact
    x[2, :] = x[2] * np.float32(2.0 ** -130)                   # 2^-136 .. 2^-124: subnormals among small normals, sums on both sides of 2^-126
    x[3, 70], x[3, 200] = np.nan, np.inf                         # each spoils exactly one bin per period
    x[4, :] = -np.inf
    x[5, 3::2] = 0.0                                             # zeros among the samples
    assert (np.abs(x[2]) < 2.0 ** -126).sum() > 50 and (np.abs(x[2]) >= 2.0 ** -126).sum() > 50
    prof, hits = _run(built, engine, x, steps, phases, nbins, sub, name="special values")
    assert not prof[0].view(np.uint32).any()
    occupied = hits > 0                                          # subnormal results are kept, not flushed
    assert np.all(prof[1][occupied] != 0) and np.all(np.abs(prof[1][occupied]) < 2.0 ** -126)
    assert ((prof[2] != 0) & (np.abs(prof[2]) < 2.0 ** -126)).sum() > 20 and (np.abs(prof[2]) >= 2.0 ** -126).sum() > 20
    assert np.all(np.isnan(prof[3]).sum(axis=2) == (np.arange(5) == 1)[None, :])
    assert np.all(np.isinf(prof[3]).sum(axis=2) == (np.arange(5) == 2)[None, :]) and np.all(prof[3][np.isinf(prof[3])] > 0)
    assert np.all(prof[4][hits > 0] == -np.inf) and not prof[4][hits == 0].view(np.uint32).any()


@pytest.mark.parametrize("ntrials", [1, 2, 4096, 65536])
def test_trial_counts(built, engine, ntrials):
    steps, phases = fold_ref.table(3, seed=31)
    x = fold_ref.signed_series(ntrials, 64, seed=ntrials)
    assert built.fold_geometry(3, 4, 64, ntrials, 64)[1] == ntrials
    _run(built, engine, x, steps, phases, 4, 64, name=ntrials)


def test_hits_options(built, engine):
    """d_hits NULL: the same profiles, the hits buffer untouched; the hits do not depend on the number of trials"""
    nbins, sub, nsamp = 9, 68, 700
    steps, phases = fold_ref.table(70, seed=41)
    x = fold_ref.signed_series(3, nsamp, seed=42)
    with_hits = _run(built, engine, x, steps, phases, nbins, sub)
    without = _run(built, engine, x, steps, phases, nbins, sub, want_hits=False)
    _same_bits(with_hits[0], without[0])
    one = _run(built, engine, x[:1], steps, phases, nbins, sub)
    assert np.array_equal(one[1], with_hits[1])
    _same_bits(one[0], with_hits[0][:1])


def _on_device(torch, host):
    return torch.from_numpy(np.ascontiguousarray(host)).to(torch.device("cuda", 0))


def _outputs(torch, ntrials, nper, nsub, nbins):
    return (_on_device(torch, np.full(ntrials * nper * nsub * nbins + 8, FILL, np.float32)),
            _on_device(torch, np.full(nper * nsub * nbins + 8, 0xDEADBEEF, np.uint32).view(np.int32)))


def _check_outputs(outs, want, what=None):
    prof, hits = outs[0].cpu().numpy(), outs[1].cpu().numpy().view(np.uint32)
    n1, n2 = want[0].size, want[1].size
    assert prof.size == n1 + 8 and hits.size == n2 + 8
    assert np.all(prof[n1:] == FILL) and np.all(hits[n2:] == 0xDEADBEEF), what
    _same_bits(prof[:n1].reshape(want[0].shape), want[0], (what, "prof"))
    assert np.array_equal(hits[:n2].reshape(want[1].shape), want[1]), what


def test_a_run_from_a_later_subintegration(built, engine):
    """The run over the samples from 3 sub on with every phi0 replaced by rtlws_fold_phase_at: the whole run's
    sub-integrations from 3 on, bit for bit"""
    import torch
    nbins, sub, ntrials = 33, T + 4, 2
    nsamp = 5 * sub + 9
    steps, phases = fold_ref.table(70, seed=51)
    steps[5], steps[6] = 0, M64 - 1
    stride = (nsamp + 3) // 4 * 4
    host = np.full((ntrials, stride), np.nan, np.float32)
    host[:, :nsamp] = fold_ref.signed_series(ntrials, nsamp, seed=52)
    whole = fold_ref.fold_ref(host, steps, phases, nbins, sub, nsamp)
    series = _on_device(torch, host)
    for first in (0, 3):
        later = [built.fold_phase_at(st, ph, first * sub) for st, ph in zip(steps, phases)]
        assert later == [fold_ref.phase_at(st, ph, first * sub) for st, ph in zip(steps, phases)]
        plan = built.FoldPlan(engine, steps, later, nbins, sub)
        assert plan.subints(nsamp) == 6
        outs = _outputs(torch, ntrials, 70, 6 - first, nbins)
        plan.run(series.data_ptr() + 4 * first * sub, stride, ntrials, nsamp - first * sub, outs[0].data_ptr(), outs[1].data_ptr(),
                 stream=built.torch_stream_handle())
        torch.cuda.synchronize()
        _check_outputs(outs, (whole[0][:, :, first:], whole[1][:, first:]), first)
        plan.close()


def test_one_plan_many_runs_and_two_plans(built, engine):
    """One plan at three nsamp in turn into preset buffers; then beside a second plan of another table, nbins and sub,
    their runs interleaved on two streams"""
    import torch
    handle = built.torch_stream_handle
    shapes = ((fold_ref.table(70, seed=61), 16, 64), (fold_ref.table(5, seed=62), 200, 132))
    nsamps = (1, T, 2 * T + 5)
    ntrials = 3
    hosts = [fold_ref.signed_series(ntrials, (nsamps[-1] + 3) // 4 * 4, seed=63 + j) for j in range(2)]
    series = [_on_device(torch, h) for h in hosts]
    plans = [built.FoldPlan(engine, st, ph, nbins, sub) for (st, ph), nbins, sub in shapes]
    (st, ph), nbins, sub = shapes[0]
    for nsamp in nsamps:
        outs = _outputs(torch, ntrials, len(st), plans[0].subints(nsamp), nbins)
        plans[0].run(series[0].data_ptr(), hosts[0].shape[1], ntrials, nsamp, outs[0].data_ptr(), outs[1].data_ptr(), stream=handle())
        torch.cuda.synchronize()
        _check_outputs(outs, fold_ref.fold_ref(hosts[0], st, ph, nbins, sub, nsamp), nsamp)
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    for s in streams:
        s.wait_stream(torch.cuda.current_stream())
    nsamp, reps = nsamps[-1], 3
    outs = [[_outputs(torch, ntrials, len(sh[0][0]), plans[j].subints(nsamp), sh[1]) for _ in range(reps)] for j, sh in enumerate(shapes)]
    for rep in range(reps):
        for j in (0, 1):
            o = outs[j][rep]
            plans[j].run(series[j].data_ptr(), hosts[j].shape[1], ntrials, nsamp, o[0].data_ptr(), o[1].data_ptr(), stream=handle(streams[j]))
    torch.cuda.synchronize()
    for j, ((st, ph), nbins, sub) in enumerate(shapes):
        want = fold_ref.fold_ref(hosts[j], st, ph, nbins, sub, nsamp)
        for rep in range(reps):
            _check_outputs(outs[j][rep], want, (j, rep))
    for plan in plans:
        plan.close()


def test_capture_and_replay(built):
    """tests/test_graph_gpu.py's pattern for this plan: rtlws_fold_run captured on a side stream enqueues nothing, replays
    give the eager launch's bits and the restatement's, twice"""
    import torch
    eng = built.Engine(0)
    nbins, sub, ntrials = 100, 68, 3
    nsamp = 2 * T + 5
    steps, phases = fold_ref.table(130, seed=71)
    host = fold_ref.signed_series(ntrials, (nsamp + 3) // 4 * 4, seed=72)
    series = _on_device(torch, host)
    plan = built.FoldPlan(eng, steps, phases, nbins, sub)
    nsub = plan.subints(nsamp)
    outs = _outputs(torch, ntrials, 130, nsub, nbins)
    before = [o.clone() for o in outs]
    g = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        with torch.cuda.graph(g, stream=side):
            plan.run(series.data_ptr(), host.shape[1], ntrials, nsamp, outs[0].data_ptr(), outs[1].data_ptr(), stream=built.torch_stream_handle())
    torch.cuda.current_stream().wait_stream(side)
    assert all(torch.equal(o, b) for o, b in zip(outs, before))              # capture enqueued nothing
    want = fold_ref.fold_ref(host, steps, phases, nbins, sub, nsamp)
    for _ in range(2):
        for o, b in zip(outs, before):
            o.copy_(b)
        g.replay()
        torch.cuda.synchronize()
        _check_outputs(outs, want, "replay")
    eager = _outputs(torch, ntrials, 130, nsub, nbins)
    plan.run(series.data_ptr(), host.shape[1], ntrials, nsamp, eager[0].data_ptr(), eager[1].data_ptr(), stream=built.torch_stream_handle())
    torch.cuda.synchronize()
    assert torch.equal(eager[0].view(torch.int32), outs[0].view(torch.int32)) and torch.equal(eager[1], outs[1])
    plan.close()
    eng.close()


# ---- the chain on the device -------------------------------------------------------------------------------------

P0 = 37.5                                        # the injected period in dedispersed samples (spectrometer rows)
CHAIN_PERIODS = tuple(P0 + 0.15 * (i - 32) for i in range(64))
CHAIN_NBINS, CHAIN_NSAMP, CHAIN_TRIAL, CHAIN_ROWS_WIDE, CHAIN_AMPLITUDE = 16, 600, 20, 2, 0.8


def periodic_capture(built, t0, nsamp, amplitude=CHAIN_AMPLITUDE, rows_wide=CHAIN_ROWS_WIDE, first_row=10):
    """A capture of noise with a burst of rows_wide rows every P0 rows, dispersed as trial t0 of the third table of
    dedisp_ref.DELAY_SETS: channel i's burst of turn j from where row first_row + floor(j P0) + d[t0][i] of the
    spectrometer (k = 6, 4 taps, K = 4, hop 32, shifted) is formed"""
    k, taps, K, hop = 6, 4, 4, 32
    M = 1 << k
    delays = dedisp_ref.delays(*dedisp_ref.DELAY_SETS[2])
    nrows = dedisp_ref.rows_needed(delays, None, nsamp)
    nsamples = (nrows * K - 1) * hop + taps * M
    b = dedisp_ref.hashed_ints(2 * nsamples, 255, seed=43).reshape(nsamples, 2).astype(np.float64)
    x = (b[:, 0] - 127.5) / 16.0 + 1j * (b[:, 1] - 127.5) / 16.0
    s = np.arange(rows_wide * K * hop)
    turn = 0
    while first_row + int(turn * P0) + rows_wide <= nsamp:
        for i in range(M):
            c = (i + M // 2) % M
            at = (first_row + int(turn * P0) + int(delays[t0, i])) * K * hop + taps * M // 2
            x[at:at + s.size] += amplitude * np.exp(2j * np.pi * c * (at + s) / M)
        turn += 1
    iq = np.clip(np.rint(np.stack([x.real, x.imag], axis=1) + 128.0), 0, 255).astype(np.uint8)
    return iq, built.pfb_design(k, taps), delays, nrows, turn


def chain_statistics(prof, hits, mom, nsamp, chi2=fold_ref.chi2):
    """chi2 [ntrials, nperiods] of one-sub-integration profiles, a trial's noise from all its segments' moments"""
    out = np.zeros(prof.shape[:2])
    for t in range(prof.shape[0]):
        sum1, sum2 = mom[t, :, 0].sum(), mom[t, :, 1].sum()
        for p in range(prof.shape[1]):
            out[t, p] = chi2(prof[t, p, 0], hits[p, 0], sum1, sum2, nsamp)
    return out


def margin_of(stat, t0, p0):
    """the statistic at (t0, p0) over the largest at any entry other than that one and its two neighbours in the table"""
    rest = stat.copy()
    rest[t0, max(p0 - 1, 0):p0 + 2] = -np.inf
    return stat[t0, p0] / rest.max()


def test_end_to_end_on_the_device(built, engine):
    """pfbspec -> dedisp -> fold, and rtlws_pulse_run for the moments, with no copy in between: the spectrometer's rows and
    the dedispersed series stay on the device; profiles, hits and moments bit for bit the restatements' chain over the
    downloaded rows; the largest rtlws_fold_chi2 at the injected trial and at P0.

    The burst's amplitude (0.8 per channel over noise of about 4.6 per component, 2 rows wide, 16 turns in 600 samples)
    is a condition fixed ahead on the CPU, with the spectrometer restated in numpy f64: there the restatements' chain gave
    chi2 429.1 at (trial 20, P0), 227.9 and 240.7 at P0's two neighbours in the table, and 2.68 times the largest of every
    other entry (160.2, two entries from P0 in trial 20; the condition: at least 2); the median entry has 15.4.  Stronger
    bursts do worse, not better: the noise estimate holds the bursts, so chi2 at the injected pair saturates near 480
    while the neighbouring trials' smeared bursts keep growing (1.2: 2.08 times, 1.5: 1.52 times)."""
    t0, p0, nsamp, nbins = CHAIN_TRIAL, 32, CHAIN_NSAMP, CHAIN_NBINS
    iq, taps, delays, nrows, turns = periodic_capture(built, t0, nsamp)
    assert turns == 16 and CHAIN_PERIODS[p0] == P0
    ntrials, M = delays.shape
    steps = [built.fold_step(p) for p in CHAIN_PERIODS]
    assert steps == [fold_ref.step_of(p) for p in CHAIN_PERIODS]
    phases = [0] * len(steps)
    stride = (nsamp + 3) // 4 * 4 + 4
    sub, seg = 600, 64
    spec, dd = built.PfbSpecPlan(engine, 6, taps), built.DedispPlan(engine, delays)
    ff, pp = built.FoldPlan(engine, steps, phases, nbins, sub), built.PulsePlan(engine, (1,), seg)
    assert ff.subints(nsamp) == 1 and pp.samples_needed(nsamp) == nsamp and dd.rows_needed(nsamp) == nrows
    nseg, nper = pp.segments(nsamp), len(steps)
    bufs = [engine.upload(iq), engine.alloc(nrows * M * 4), engine.upload(np.full((ntrials, stride), np.nan, np.float32)),
            engine.alloc(ntrials * nper * nbins * 4), engine.alloc(nper * nbins * 4),
            engine.alloc(ntrials * nseg * 4), engine.alloc(ntrials * nseg * 4), engine.alloc(ntrials * nseg * 16)]
    try:
        spec.run(bufs[0], nrows, 4, bufs[1], hop=32, shifted=True)
        dd.run(bufs[1], nsamp, bufs[2], in_stride=M, out_stride=stride)
        ff.run(bufs[2], stride, ntrials, nsamp, bufs[3], bufs[4])
        pp.run(bufs[2], stride, ntrials, nsamp, bufs[5], bufs[6], bufs[7])
        engine.sync()
        rows = engine.download(bufs[1], np.float32, (nrows, M))
        prof = engine.download(bufs[3], np.float32, (ntrials, nper, 1, nbins))
        hits = engine.download(bufs[4], np.uint32, (nper, 1, nbins))
        mom = engine.download(bufs[7], np.float64, (ntrials, nseg, 2))
    finally:
        for plan in (spec, dd, ff, pp):
            plan.close()
        for b in bufs:
            b.free()
    series = dedisp_ref.dedisp_ref(rows, delays, None, nsamp)
    want_prof, want_hits = fold_ref.fold_ref(series, steps, phases, nbins, sub, nsamp)
    want_mom = pulse_ref.pulse_ref(series, (1,), seg, nsamp)[2]
    _same_bits(prof, want_prof, "prof")
    assert np.array_equal(hits, want_hits)
    assert np.array_equal(mom.view(np.uint64), want_mom.view(np.uint64))
    # the condition, on the restatements' chain alone
    stat = chain_statistics(want_prof, want_hits, want_mom, nsamp)
    assert np.unravel_index(np.argmax(stat), stat.shape) == (t0, p0) and margin_of(stat, t0, p0) >= 2.0, (np.argmax(stat), margin_of(stat, t0, p0))
    # the library's statistic over the device's outputs
    got = chain_statistics(prof, hits, mom, nsamp, chi2=built.fold_chi2)
    assert np.allclose(got, stat, rtol=1e-12, atol=0)
    print("largest chi2 %.1f at trial %d, period %.2f; its neighbours %.1f and %.1f; %.2f times the largest elsewhere (median %.1f)"
          % (got.max(), t0, CHAIN_PERIODS[p0], got[t0, p0 - 1], got[t0, p0 + 1], margin_of(got, t0, p0), np.median(got)))
    assert np.unravel_index(np.argmax(got), got.shape) == (t0, p0)

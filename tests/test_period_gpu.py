"""GPU suite of include/rtlws_period.h (librtlws_period.so) against its numpy restatement (tests/period_ref.py).

Stage 1 (the power spectrum) within the derived bound period_ref.bound(log2n) of the f64 spectrum, per trial, the worst
ratio printed; exact-bin tones.  Stages 2 - 4 bit for bit on uint32 views, NaN by place: the whitened row from the
device's own power row, the peaks from the device's own whitened row, and the peaks with both optional rows NULL.  NaN
in the stride's padding and behind nsamp, a preset pattern behind every output.  Every frame length (every radix
decomposition), nsamp at the borders, the whitening blocks inside a thread, a wavefront and across wavefronts, segments
of one chunk and of several, klo at the borders of a segment, the trial counts; crafted trials (all zero, an impulse
whose spectrum is flat: equal maxima, tones at the first and last bin of a segment and at klo); a NaN and an Inf trial
beside finite ones; one plan many times and beside another, graph capture; and the chain spectrometer -> dedispersion
-> periodicity search -> folding on the device.

Worst observed stage-1 error over this file's cases, as a share of the bound (measured on one MI355X; printed by
test_every_frame_length): 0.0108, 0.0095, 0.0088, 0.0097, 0.0099, 0.0096 at log2n 10 .. 15 (bounds 1.47e-5 .. 2.15e-5).
Every trial's every bin is held to period_ref.bound_bin as well (period_family.check_stage1), the tones' leakage bins
included.  Worst per-bin share of `bound_bin`, measured on one MI355X (printed by test_every_frame_length): 0.0217,
0.0154, 0.0214, 0.0189, 0.0173, 0.0180 at log2n 10 .. 15 (b1 6.09e-6 .. 8.90e-6)."""
import numpy as np
import pytest

import dedisp_ref
import fold_ref
import period_ref
import pulse_ref
from period_family import FILL, check_bare, check_behind, check_stage1, noise, padded, unpack
from period_family import same_bits as _same_bits
from test_fold_gpu import CHAIN_NSAMP, CHAIN_TRIAL, P0, periodic_capture

pytestmark = pytest.mark.gpu

WORST, WORST_BIN = {}, {}


def _noise(ntrials, nsamp, seed, mean=10.0):
    return noise(ntrials, nsamp, seed, mean, draw=np.float64)


def _reference(log2n):
    """the f64 spectrum of a trial's samples; the premises of the bound hold for them"""
    def reference(xs, name):
        ref = period_ref.power(xs, log2n)
        if xs.size > 1:
            x64 = xs.astype(np.float64)
            assert period_ref.nyquist_power(xs, log2n) <= ref.sum() and (x64.std() == 0 or abs(x64.mean()) <= 256 * x64.std()), name
        return ref
    return reference


def _check_stage1(power, x, log2n, nsamp, name, finite=None):
    """per trial sum |P^ - P| <= c sum P against the f64 spectrum, the premises of that bound hold for x; and every bin
    within period_ref.bound_bin"""
    return check_stage1(power, x, nsamp, period_ref.bound(log2n), period_ref.bound_bin(log2n), _reference(log2n), WORST, WORST_BIN, log2n, name, finite)


def _run(built, engine, x, log2n, levels, norm, seg, klo, nsamp=None, wide=False, name=None, stage1=True, finite=None):
    """x float32 [ntrials, >= nsamp] through Engine.period with NaN in the padding and behind nsamp and preset guards
    behind the outputs; stage 1 against the f64 spectrum, stages 2 - 4 against the restatement over the device's own
    rows; the run with NULL rows gives the same peaks and leaves the rows' buffers alone -> (best, at, power, white)"""
    ntrials = x.shape[0]
    nsamp = x.shape[1] if nsamp is None else nsamp
    m = 1 << (log2n - 1)
    rows, stride = padded(x, nsamp, wide)
    outs = engine.period(rows, log2n, levels, norm, seg, klo, nsamp=nsamp, in_stride=stride, fill=FILL)
    bare = engine.period(rows, log2n, levels, norm, seg, klo, nsamp=nsamp, in_stride=stride, want_rows=False, fill=FILL)
    best, at, power, white = unpack(outs, ntrials, levels, m // seg, m, built.PERIOD_GUARD, name)
    check_bare(bare, best, at, name)
    if stage1:
        _check_stage1(power, x, log2n, nsamp, name, finite)
    check_behind(power, white, best, at, levels, norm, seg, klo, name)
    return best, at, power, white


def _plans(log2n):
    """(levels, norm, seg, klo): norm 16 (inside a thread), 1024 (a wavefront), 2048 (two), M; seg 64, 1024 (one chunk),
    2048 (two chunks), M; klo 1, seg - 1, seg, M - 1; levels 1 and 5"""
    m = 1 << (log2n - 1)
    norms = sorted({16, min(1024, m), min(2048, m), m})
    segs = sorted({64, min(1024, m), min(2048, m), m})
    out = []
    for i, seg in enumerate(segs):
        for j, klo in enumerate((1, seg - 1, seg if seg < m else m - 1, m - 1)):
            out.append((5 if (i + j) % 3 else 1, norms[(i + j) % len(norms)], seg, klo))
    for norm in norms:                                           # every norm with every seg at least once more, levels 5
        out.append((5, norm, segs[len(out) % len(segs)], 1))
    return out


def test_the_cases_cover_the_paths(built):
    for log2n in range(10, 16):
        m = 1 << (log2n - 1)
        plans = _plans(log2n)
        assert all(built.period_supported(log2n, *p) == 1 for p in plans), log2n
        assert {p[0] for p in plans} == {1, 5} and {16, m} <= {p[1] for p in plans} and {64, m} <= {p[2] for p in plans}
        assert {1, m - 1} <= {p[3] for p in plans} and any(p[3] == p[2] - 1 for p in plans) and any(p[3] == p[2] for p in plans)
        rc, blocks, threads, lds, nseg = built.period_geometry(log2n, 5, 16, 64, 1, 257)
        assert (rc, blocks, threads, lds, nseg) == (0,) + period_ref.geometry(log2n, 64, 257)
    assert 257 > 256                                             # more trials than the device has compute units


@pytest.mark.parametrize("log2n", range(10, 16))
def test_every_frame_length(built, engine, log2n):
    """every radix decomposition: nsamp at its borders with tight and wide strides, every plan of _plans at nsamp N"""
    n = 1 << log2n
    x = _noise(2, n, seed=log2n)
    x[1] += (3.0 * np.cos(2.0 * np.pi * np.arange(n) / 37.5)).astype(np.float32)
    for i, nsamp in enumerate((1, 5, n - 4, n - 1, n)):
        levels, norm, seg, klo = _plans(log2n)[i]
        for wide in (False, True):
            _run(built, engine, x, log2n, levels, norm, seg, klo, nsamp=nsamp, wide=wide, name=(log2n, nsamp, wide))
    for plan in _plans(log2n):
        best, at, _, _ = _run(built, engine, x, log2n, *plan, name=(log2n, plan))
        levels, norm, seg, klo = plan
        assert np.all(at[:, :, : klo // seg] == -1) and np.all(np.isneginf(best[:, :, : klo // seg]))
        assert np.all(at[:, :, klo // seg:] >= klo)
    print("log2n %d: worst stage-1 error %.3g of the bound %.3g; worst bin %.3g of bound_bin %.3g"
          % (log2n, WORST[log2n], period_ref.bound(log2n), WORST_BIN[log2n], period_ref.bound_bin(log2n)))


@pytest.mark.parametrize("ntrials", [1, 2, 257, 4096])
def test_trial_counts(built, engine, ntrials):
    x = _noise(ntrials, 600, seed=ntrials)
    assert built.period_geometry(10, 5, 64, 64, 8, ntrials)[1] == ntrials
    _run(built, engine, x, 10, 5, 64, 64, 8, name=ntrials)
    if ntrials == 257:
        _run(built, engine, _noise(ntrials, 4096, seed=5), 12, 5, 64, 256, 8, name=(12, ntrials))


@pytest.mark.parametrize("log2n", range(10, 16))
def test_exact_bin_tones(built, engine, log2n):
    """amplitude A at bins 1, M / 2 and M - 1: P[k0] within c (A N / 2)^2 of (A N / 2)^2, and every bin, the tone's and
    the leakage bins, within bound_bin of the f64 spectrum of the f32 series (_run's check_stage1; the leakage of the
    rounded cosine is the reference's too); a permutation fault of the transform shows here on its own"""
    n, m = 1 << log2n, 1 << (log2n - 1)
    amp = 3.0
    bins = (1, m // 2, m - 1)
    x = np.stack([amp * np.cos(2.0 * np.pi * k0 * np.arange(n) / n + 0.3) for k0 in bins]).astype(np.float32)
    _, _, power, _ = _run(built, engine, x, log2n, 1, 16, 64, 1, name=("tones", log2n))
    full, c = (amp * n / 2.0) ** 2, period_ref.bound(log2n)
    for t, k0 in enumerate(bins):
        p = power[t].astype(np.float64)
        assert abs(p[k0] - full) <= c * full, (log2n, k0, p[k0], full)
        p[k0] = 0.0
        assert p.max() <= c * full, (log2n, k0, p.argmax(), p.max(), c * full)          # what bound_bin holds far tighter


def test_crafted_trials(built, engine):
    """an all-zero trial (0 / 0: NaN rows, every peak (-Inf, -1)); an impulse, whose spectrum is flat: whole segments of
    equal maxima, taken at their first k or at klo; tones at the first and the last bin of a segment and at klo; rows with
    exponents over 2^-6 .. 2^6"""
    log2n, seg = 11, 64
    n, m = 1 << log2n, 1 << (log2n - 1)
    t = np.arange(n)
    rng = np.random.default_rng(7)
    x = np.zeros((6, n), np.float32)
    x[1, 0] = 1.0
    tone = lambda k0: 5.0 * np.cos(2.0 * np.pi * k0 * t / n)
    x[2] = (tone(3 * seg) + 0.01 * rng.standard_normal(n) + 2.0).astype(np.float32)             # the first k of segment 3
    x[3] = (tone(4 * seg - 1) + 0.01 * rng.standard_normal(n) + 2.0).astype(np.float32)         # the last k of segment 3
    x[4] = (tone(200) + 0.01 * rng.standard_normal(n) + 2.0).astype(np.float32)                 # klo itself
    x[5] = period_ref.signed_exponent_series(1, n, log2n, seed=8)[0]
    for klo in (1, 200):
        best, at, power, white = _run(built, engine, x, log2n, 5, 64, seg, klo, name=("crafted", klo))
        assert not power[0].any() and np.isnan(white[0]).all() and np.all(at[0] == -1) and np.all(np.isneginf(best[0]))
        # the impulse: segments of equal maxima at level 0
        s0 = -(-klo // seg) + 1
        ties = (white[1].reshape(-1, seg) == white[1].reshape(-1, seg).max(axis=1, keepdims=True)).sum(axis=1)
        assert ties[s0:].min() >= 2, ties
        assert np.array_equal(at[1, 0, s0:], seg * np.arange(s0, m // seg))
        assert at[3, 0, 3] == 4 * seg - 1 and at[4, 0, 3] == 200
        if klo == 1:
            assert at[2, 0, 3] == 3 * seg
        else:
            assert at[1, 0, 3] == 200 and np.all(at[:, :, :3] == -1) and np.all(np.isneginf(best[:, :, :3]))
    expo = np.frexp(power[5][power[5] > 0])[1]
    assert expo.max() - expo.min() >= 12


def test_bad_trials_leave_the_others_alone(built, engine):
    """one trial with a NaN and one with +Inf beside finite trials: the finite trials' outputs keep their bits"""
    log2n, plan = 12, (5, 64, 256, 8)
    x = _noise(5, 4096, seed=21)
    clean = _run(built, engine, x, log2n, *plan, name="clean")
    bad = x.copy()
    bad[1, 1234], bad[3, 7] = np.nan, np.inf
    finite = np.array([True, False, True, False, True])
    got = _run(built, engine, bad, log2n, *plan, name="bad", finite=finite)
    for a, b in zip(got, clean):
        _same_bits(a[finite], b[finite], "finite trials")
    assert np.isnan(got[2][1]).all()


def _on_device(torch, host):
    return torch.from_numpy(np.ascontiguousarray(host)).to(torch.device("cuda", 0))


def _outputs(torch, ntrials, levels, nseg, m):
    return (_on_device(torch, np.full(ntrials * levels * nseg + 8, FILL, np.float32)),
            _on_device(torch, np.full(ntrials * levels * nseg + 8, 0x5EADBEEF, np.int32)),
            _on_device(torch, np.full(ntrials * m + 8, FILL, np.float32)), _on_device(torch, np.full(ntrials * m + 8, FILL, np.float32)))


def _check_outputs(outs, x, log2n, levels, norm, seg, klo, nsamp, what=None):
    best, at, power, white = [o.cpu().numpy() for o in outs]
    ntrials, m = x.shape[0], 1 << (log2n - 1)
    n1, n2 = ntrials * levels * (m // seg), ntrials * m
    assert np.all(best[n1:] == FILL) and np.all(at[n1:] == 0x5EADBEEF) and np.all(power[n2:] == FILL) and np.all(white[n2:] == FILL), what
    power, white = power[:n2].reshape(ntrials, m), white[:n2].reshape(ntrials, m)
    _check_stage1(power, x, log2n, nsamp, what)
    _same_bits(white, period_ref.whiten(power, norm), (what, "white"))
    want_best, want_at = period_ref.peaks(period_ref.sums(white, levels), seg, klo)
    _same_bits(best[:n1].reshape(want_best.shape), want_best, (what, "best"))
    assert np.array_equal(at[:n1].reshape(want_at.shape), want_at), what
    return best, at, power, white


def test_one_plan_many_runs_and_two_plans(built, engine):
    """One plan at three nsamp in turn into preset buffers (nsamp above its N refused); then beside a second plan of
    another frame length, their runs interleaved on two streams"""
    import torch
    handle = built.torch_stream_handle
    shapes = ((10, 5, 64, 64, 8), (13, 3, 2048, 2048, 100))
    ntrials = 3
    hosts = [_noise(ntrials, 1 << sh[0], seed=31 + j) for j, sh in enumerate(shapes)]
    series = [_on_device(torch, h) for h in hosts]
    plans = [built.PeriodPlan(engine, *sh) for sh in shapes]
    log2n, levels, norm, seg, klo = shapes[0]
    for nsamp in (1, 600, 1024):
        outs = _outputs(torch, ntrials, levels, 512 // seg, 512)
        plans[0].run(series[0].data_ptr(), 1024, ntrials, nsamp, *[o.data_ptr() for o in outs], stream=handle())
        torch.cuda.synchronize()
        _check_outputs(outs, hosts[0], *shapes[0], nsamp, nsamp)
    outs = _outputs(torch, ntrials, levels, 512 // seg, 512)
    rc = plans[0].run(series[0].data_ptr(), 1028, 1, 1025, *[o.data_ptr() for o in outs], stream=handle(), check=False)
    assert rc == -1 and "nsamp must be at most the plan's N" in built.period_last_error()
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    for s in streams:
        s.wait_stream(torch.cuda.current_stream())
    reps = 3
    outs = [[_outputs(torch, ntrials, sh[1], (1 << (sh[0] - 1)) // sh[3], 1 << (sh[0] - 1)) for _ in range(reps)] for sh in shapes]
    for rep in range(reps):
        for j, sh in enumerate(shapes):
            plans[j].run(series[j].data_ptr(), 1 << sh[0], ntrials, 1 << sh[0], *[o.data_ptr() for o in outs[j][rep]], stream=handle(streams[j]))
    torch.cuda.synchronize()
    for j, sh in enumerate(shapes):
        first = _check_outputs(outs[j][0], hosts[j], *sh, 1 << sh[0], (j, 0))
        for rep in range(1, reps):
            for a, b in zip(first, [o.cpu().numpy() for o in outs[j][rep]]):
                assert np.array_equal(a.reshape(-1).view(np.uint32), b[:a.size].view(np.uint32)), (j, rep)
    for plan in plans:
        plan.close()


def test_capture_and_replay(built):
    """tests/test_graph_gpu.py's pattern for this plan: rtlws_period_run captured on a side stream enqueues nothing,
    replays give the eager launch's bits and the restatement's, twice"""
    import torch
    eng = built.Engine(0)
    shape, ntrials, nsamp = (14, 5, 64, 256, 8), 3, 16000
    m = 1 << (shape[0] - 1)
    host = _noise(ntrials, 16000, seed=41)
    series = _on_device(torch, host)
    plan = built.PeriodPlan(eng, *shape)
    outs = _outputs(torch, ntrials, shape[1], m // shape[3], m)
    before = [o.clone() for o in outs]
    g = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        with torch.cuda.graph(g, stream=side):
            plan.run(series.data_ptr(), 16000, ntrials, nsamp, *[o.data_ptr() for o in outs], stream=built.torch_stream_handle())
    torch.cuda.current_stream().wait_stream(side)
    assert all(torch.equal(o, b) for o, b in zip(outs, before))              # capture enqueued nothing
    for _ in range(2):
        for o, b in zip(outs, before):
            o.copy_(b)
        g.replay()
        torch.cuda.synchronize()
        _check_outputs(outs, host, *shape, nsamp, "replay")
    eager = _outputs(torch, ntrials, shape[1], m // shape[3], m)
    plan.run(series.data_ptr(), 16000, ntrials, nsamp, *[o.data_ptr() for o in eager], stream=built.torch_stream_handle())
    torch.cuda.synchronize()
    assert all(torch.equal(e.view(torch.int32), o.view(torch.int32)) for e, o in zip(eager, outs))
    plan.close()
    eng.close()


# ---- the chain on the device -------------------------------------------------------------------------------------

def chain_lnq(best, at, lnq):
    """lnq [ntrials, levels, nseg] of the peaks (0 where nothing was taken)"""
    out = np.zeros(best.shape)
    for idx in np.ndindex(*best.shape):
        if at[idx] >= 0:
            out[idx] = lnq(float(best[idx]), 1 << idx[1])
    return out


def chain_conditions(lnq, at, t0, samples):
    """the first three conditions of the chain: the smallest lnq lies at trial t0, its period is within one
    fundamental bin (P0^2 / 1024 samples) of P0, and it is at least 5 below every trial more than one DM step away
    -> (the period, its lnq, the smallest lnq elsewhere)"""
    idx = np.unravel_index(np.argmin(lnq), lnq.shape)
    period = samples(10, idx[1], int(at[idx]))
    per_trial = lnq.reshape(lnq.shape[0], -1).min(axis=1)
    others = min(per_trial[t] for t in range(lnq.shape[0]) if abs(t - t0) > 1)
    assert idx[0] == t0, idx
    assert abs(period - P0) <= P0 * P0 / 1024.0, period
    assert lnq[idx] <= others - 5.0, (lnq[idx], others)
    return period, lnq[idx], others


def test_end_to_end_on_the_device(built, engine):
    """pfbspec -> dedisp -> period -> fold, and rtlws_pulse_run for the moments, with no copy in between: tests/
    test_fold_gpu.py's scene (16 dispersed bursts 37.5 rows apart in 600 dedispersed samples at trial 20, amplitude 0.8)
    at log2n 10, levels 5, norm 64, seg 64, klo 8.

    The conditions were fixed ahead on the CPU with the restatements' chain (the spectrometer restated in numpy f64,
    dedisp_ref, period_ref.power rounded to f32 and stages 2 - 4, fold_ref, pulse_ref): there the smallest lnq, -122.1,
    lies at trial 20, level 4, bin 437: 16384 / 437 = 37.49 samples (one fundamental bin is 1.37); the smallest lnq of
    every trial more than one DM step away is -22.9 (99 above; the condition: at least 5), trials 19 and 21 have -15.3 and
    -14.1; folding every trial at rtlws_fold_step(37.49) gives chi2 429 at trial 20 against 102 at the next.  The test
    recomputes them from the restatements over the device's rows before it looks at the device's peaks."""
    t0, nsamp = CHAIN_TRIAL, CHAIN_NSAMP
    log2n, levels, norm, seg, klo, nbins = 10, 5, 64, 64, 8, 16
    iq, taps, delays, nrows, turns = periodic_capture(built, t0, nsamp)
    assert turns == 16
    ntrials, M = delays.shape
    m, nseg = 512, 512 // seg
    stride = (nsamp + 3) // 4 * 4 + 4
    spec, dd = built.PfbSpecPlan(engine, 6, taps), built.DedispPlan(engine, delays)
    pp, per = built.PulsePlan(engine, (1,), 64), built.PeriodPlan(engine, log2n, levels, norm, seg, klo)
    pseg = pp.segments(nsamp)
    bufs = [engine.upload(iq), engine.alloc(nrows * M * 4), engine.upload(np.full((ntrials, stride), np.nan, np.float32)),
            engine.alloc(ntrials * levels * nseg * 4), engine.alloc(ntrials * levels * nseg * 4), engine.alloc(ntrials * m * 4),
            engine.alloc(ntrials * m * 4), engine.alloc(ntrials * pseg * 4), engine.alloc(ntrials * pseg * 4), engine.alloc(ntrials * pseg * 16),
            engine.alloc(ntrials * nbins * 4), engine.alloc(nbins * 4)]
    ff = None
    try:
        spec.run(bufs[0], nrows, 4, bufs[1], hop=32, shifted=True)
        dd.run(bufs[1], nsamp, bufs[2], in_stride=M, out_stride=stride)
        per.run(bufs[2], stride, ntrials, nsamp, bufs[3], bufs[4], bufs[5], bufs[6])
        pp.run(bufs[2], stride, ntrials, nsamp, bufs[7], bufs[8], bufs[9])
        engine.sync()
        best = engine.download(bufs[3], np.float32, (ntrials, levels, nseg))
        at = engine.download(bufs[4], np.int32, (ntrials, levels, nseg))
        # the candidate goes back to the device as one period: the series never left it
        got_lnq = chain_lnq(best, at, built.period_lnq)
        period, low, others = chain_conditions(got_lnq, at, t0, built.period_samples)
        step = built.fold_step(period)
        ff = built.FoldPlan(engine, [step], [0], nbins, 600)
        ff.run(bufs[2], stride, ntrials, nsamp, bufs[10], bufs[11])
        engine.sync()
        rows = engine.download(bufs[1], np.float32, (nrows, M))
        power = engine.download(bufs[5], np.float32, (ntrials, m))
        white = engine.download(bufs[6], np.float32, (ntrials, m))
        mom = engine.download(bufs[9], np.float64, (ntrials, pseg, 2))
        prof = engine.download(bufs[10], np.float32, (ntrials, 1, 1, nbins))
        hits = engine.download(bufs[11], np.uint32, (1, 1, nbins))
    finally:
        for plan in (spec, dd, pp, per, ff):
            if plan is not None:
                plan.close()
        for b in bufs:
            b.free()
    # the restatements' chain over the device's rows meets the conditions by itself
    series = dedisp_ref.dedisp_ref(rows, delays, None, nsamp)
    ref_power = np.stack([period_ref.power(series[t], log2n) for t in range(ntrials)]).astype(np.float32)
    _, ref_best, ref_at = period_ref.period_ref(ref_power, levels, norm, seg, klo)
    ref_period, ref_low, ref_others = chain_conditions(chain_lnq(ref_best, ref_at, period_ref.lnq), ref_at, t0, period_ref.samples)
    ref_prof, ref_hits = fold_ref.fold_ref(series, [fold_ref.step_of(ref_period)], [0], nbins, 600, nsamp)
    ref_mom = pulse_ref.pulse_ref(series, (1,), 64, nsamp)[2]
    ref_chi = [fold_ref.chi2(ref_prof[t, 0, 0], ref_hits[0, 0], ref_mom[t, :, 0].sum(), ref_mom[t, :, 1].sum(), nsamp) for t in range(ntrials)]
    assert int(np.argmax(ref_chi)) == t0
    # the device: stage 1 within its bound of the restatement's, stages 2 - 4 bit for bit from its own rows
    _check_stage1(power, series, log2n, nsamp, "chain")
    _same_bits(white, period_ref.whiten(power, norm), "white")
    want_best, want_at = period_ref.peaks(period_ref.sums(white, levels), seg, klo)
    _same_bits(best, want_best, "best")
    assert np.array_equal(at, want_at)
    assert period == ref_period and step == fold_ref.step_of(period)
    _same_bits(prof, ref_prof, "prof")
    assert np.array_equal(hits, ref_hits) and np.array_equal(mom.view(np.uint64), ref_mom.view(np.uint64))
    chi = [built.fold_chi2(prof[t, 0, 0], hits[0, 0], mom[t, :, 0].sum(), mom[t, :, 1].sum(), nsamp) for t in range(ntrials)]
    print("smallest lnq %.1f at trial %d: %.3f samples (the restatements: %.1f, %.3f); %.1f elsewhere; chi2 there %.0f, next %.0f"
          % (low, t0, period, ref_low, ref_period, others, max(chi), sorted(chi)[-2]))
    assert int(np.argmax(chi)) == t0

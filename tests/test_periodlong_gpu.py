"""GPU suite of include/rtlws_periodlong.h (librtlws_periodlong.so) against its numpy restatements (tests/periodlong_ref.py
for stage 1, tests/period_ref.py for stages 2 - 4, unchanged).

Stage 1 (the power spectrum) within the derived bound periodlong_ref.bound(log2n) of the f64 spectrum, per trial, the
worst ratio printed; exact-bin tones at the ends of the axis and on each side of every border of the decomposition
M = M1 M2; impulses.  Stages 2 - 4 bit for bit on uint32 views, NaN by place: the whitened row from the device's own
power row, the peaks from the device's own whitened row, and the peaks with both optional rows NULL and with one of
them.  NaN in the stride's padding and behind nsamp, a preset pattern behind every output.  Every frame length, nsamp at
the borders, the whitening blocks inside a thread, a wavefront and a workgroup, segments of one chunk and of sixteen, klo
at the borders of a segment, the trial counts and the border between two groups of trials in flight; crafted trials; a
NaN and an Inf trial beside finite ones; one plan many times and beside another, graph capture; and the chain
dedispersion -> periodicity search -> folding on the device.

Worst observed stage-1 error over this file's cases, as a share of the bound (measured on one MI355X; printed by
test_every_frame_length): 0.0077, 0.0075, 0.0065, 0.0063, 0.0060, 0.0096, 0.0062 at log2n 16 .. 22 (bounds 2.40e-5 ..
3.22e-5).  Every trial's every bin is held to periodlong_ref.bound_bin as well (period_family.check_stage1), the tones'
leakage bins and the impulses' flat bins included.  Worst per-bin share of `bound_bin`, measured on one MI355X (printed
by test_every_frame_length): 0.0137, 0.0164, 0.0229, 0.0228, 0.0131, 0.0186, 0.0165 at log2n 16 .. 22 (b1 9.90e-6 ..
1.33e-5)."""
import numpy as np
import pytest

import dedisp_ref
import fold_ref
import period_ref
import periodlong_ref
from period_family import FILL, check_bare, check_stage1, padded, unpack
from period_family import check_behind as _check_behind, noise as _noise, same_bits as _same_bits

pytestmark = pytest.mark.gpu

WORST, WORST_BIN = {}, {}
LOG2NS = range(16, 23)


def _reference(log2n):
    """the f64 spectrum of a trial's samples; both premises of the bound hold for them"""
    def reference(xs, name):
        ref, nyquist_small, mean_small = periodlong_ref.power_and_premises(xs, log2n)
        if xs.size > 1 and ref.sum() > 0:
            assert nyquist_small and mean_small, name
        return ref
    return reference


def _check_stage1(power, x, log2n, nsamp, name, finite=None):
    """per trial sum |P^ - P| <= c sum P against the f64 spectrum, both premises of that bound hold for x; and every bin
    within periodlong_ref.bound_bin"""
    return check_stage1(power, x, nsamp, periodlong_ref.bound(log2n), periodlong_ref.bound_bin(log2n), _reference(log2n), WORST, WORST_BIN,
                        log2n, name, finite)


def _run(built, engine, x, log2n, levels, norm, seg, klo, nsamp=None, wide=False, name=None, stage1=True, finite=None, bare=True, max_trials=None):
    """x float32 [ntrials, >= nsamp] through Engine.periodlong with NaN in the padding and behind nsamp and preset guards
    behind the outputs; stage 1 against the f64 spectrum, stages 2 - 4 against the restatement over the device's own
    rows; with `bare` the run with NULL rows gives the same peaks and leaves the rows' buffers alone -> (best, at,
    power, white)"""
    ntrials = x.shape[0]
    nsamp = x.shape[1] if nsamp is None else nsamp
    m = 1 << (log2n - 1)
    rows, stride = padded(x, nsamp, wide)
    outs = engine.periodlong(rows, log2n, levels, norm, seg, klo, nsamp=nsamp, in_stride=stride, fill=FILL, max_trials=max_trials)
    best, at, power, white = unpack(outs, ntrials, levels, m // seg, m, built.PERIOD_GUARD, name)
    if bare:
        none = engine.periodlong(rows, log2n, levels, norm, seg, klo, nsamp=nsamp, in_stride=stride, want_rows=False, fill=FILL, max_trials=max_trials)
        check_bare(none, best, at, name)
    if stage1:
        _check_stage1(power, x, log2n, nsamp, name, finite)
    _check_behind(power, white, best, at, levels, norm, seg, klo, name)
    return best, at, power, white


def _plans(log2n):
    """(levels, norm, seg, klo): levels 1 and 5; norm 16 (inside a thread), 1024 (a wavefront), 16384 (a workgroup); seg 64,
    1024 (one chunk), 16384 (sixteen chunks); klo 1, seg - 1, seg, M - 1"""
    m = 1 << (log2n - 1)
    norms, segs = (16, 1024, 16384), (64, 1024, 16384)
    out = []
    for i, seg in enumerate(segs):
        for j, klo in enumerate((1, seg - 1, seg, m - 1)):
            out.append((5 if (i + j) % 3 else 1, norms[(i + j) % 3], seg, klo))
    return out


def test_the_cases_cover_the_paths(built):
    for log2n in LOG2NS:
        m = 1 << (log2n - 1)
        plans = _plans(log2n)
        assert all(built.periodlong_supported(log2n, *p) == 1 for p in plans), log2n
        assert {p[0] for p in plans} == {1, 5} and {p[1] for p in plans} == {16, 1024, 16384} and {p[2] for p in plans} == {64, 1024, 16384}
        assert {1, m - 1} <= {p[3] for p in plans} and any(p[3] == p[2] - 1 for p in plans) and any(p[3] == p[2] for p in plans)
        # every norm meets every seg
        assert {(p[1], p[2]) for p in plans} == {(a, b) for a in (16, 1024, 16384) for b in (64, 1024, 16384)}
        got = built.periodlong_geometry(log2n, 5, 16, 64, 1, 257)
        assert got == (0,) + periodlong_ref.geometry(log2n, 64, 257)


@pytest.mark.parametrize("log2n", LOG2NS)
def test_every_frame_length(built, engine, log2n):
    """nsamp at its borders with tight and wide strides, every plan of _plans at nsamp N; two trials up to log2n 19, one
    above"""
    n = 1 << log2n
    ntrials = 2 if log2n <= 19 else 1
    x = _noise(ntrials, n, seed=log2n)
    x[-1] += (3.0 * np.cos(2.0 * np.pi * np.arange(n) / 37.5)).astype(np.float32)
    plans = _plans(log2n)
    for i, nsamp in enumerate((1, 5, n - 4, n - 1, n)):
        levels, norm, seg, klo = plans[i]
        for wide in (False, True):
            _run(built, engine, x, log2n, levels, norm, seg, klo, nsamp=nsamp, wide=wide, name=(log2n, nsamp, wide),
                 bare=log2n <= 19 or (nsamp >= n - 1 and wide), stage1=log2n <= 19 or not wide or nsamp >= n - 1)
    # the long frames: three of the plans that nsamp's borders have not taken, all seven of them over log2n 20 .. 22
    for i, plan in enumerate([plans[5 + (3 * log2n + j) % 7] for j in range(3)] if log2n > 19 else plans):
        best, at, _, _ = _run(built, engine, x, log2n, *plan, name=(log2n, plan), bare=log2n <= 19 or i == 0, stage1=i == 0)
        levels, norm, seg, klo = plan
        assert np.all(at[:, :, : klo // seg] == -1) and np.all(np.isneginf(best[:, :, : klo // seg]))
        assert np.all(at[:, :, klo // seg:] >= klo)
    print("log2n %d: worst stage-1 error %.3g of the bound %.3g; worst bin %.3g of bound_bin %.3g"
          % (log2n, WORST[log2n], periodlong_ref.bound(log2n), WORST_BIN[log2n], periodlong_ref.bound_bin(log2n)))


def test_one_optional_row_alone(built, engine):
    """the peaks and the row that is asked for have the same bits whichever optional rows are given"""
    log2n, plan = 16, (5, 64, 256, 8)
    x = _noise(2, 50000, seed=3)
    best, at, power, white = engine.periodlong(x, log2n, *plan)
    for want_power, want_white in ((True, False), (False, True), (False, False)):
        b, a, p, w = engine.periodlong(x, log2n, *plan, want_power=want_power, want_white=want_white)
        _same_bits(b, best, "best")
        assert np.array_equal(a, at) and (p is None) == (not want_power) and (w is None) == (not want_white)
        if want_power:
            _same_bits(p, power, "power alone")
        if want_white:
            _same_bits(w, white, "white alone")


@pytest.mark.parametrize("ntrials", [1, 2, 257])
def test_trial_counts(built, engine, ntrials):
    x = _noise(ntrials, 40000, seed=ntrials)
    assert built.periodlong_geometry(16, 5, 64, 64, 8, ntrials)[1][2] == 16 * ntrials
    _run(built, engine, x, 16, 5 if ntrials < 257 else 2, 64, 256, 8, name=ntrials)


@pytest.mark.parametrize("log2n,max_trials", [(16, 3), (20, 1)])
def test_group_border(built, engine, log2n, max_trials):
    """a plan opened for max_trials in flight runs one trial more: the trials on either side of the border between two
    groups compare equal to a run of each alone"""
    ntrials, nsamp, plan = max_trials + 1, (1 << log2n) - 3, (5, 1024, 1024, 8)
    assert periodlong_ref.in_flight(log2n, max_trials) == max_trials
    x = _noise(ntrials, nsamp, seed=50 + log2n)
    p = built.PeriodLongPlan(engine, log2n, *plan, max_trials=max_trials)
    assert p.workspace_bytes() == max_trials * periodlong_ref.trial_bytes(log2n)
    p.close()
    got = _run(built, engine, x, log2n, *plan, name=("groups", log2n), max_trials=max_trials, bare=False)
    for t in (max_trials - 1, max_trials):
        alone = _run(built, engine, x[t:t + 1], log2n, *plan, name=("alone", t), max_trials=1, bare=False, stage1=False)
        for a, b in zip(got, alone):
            _same_bits(a[t:t + 1], b, ("trial", t))


def _tone_bins(log2n):
    l1, l2 = periodlong_ref.split(log2n)
    m, m1, m2 = 1 << (log2n - 1), 1 << l1, 1 << l2
    return (1, m // 2, m - 1, m1 - 1, m1, m2 - 1, m2, m - m1)


@pytest.mark.parametrize("log2n", LOG2NS)
def test_exact_bin_tones(built, engine, log2n):
    """amplitude A at bins 1, M / 2 and M - 1 and on each side of every border of M = M1 M2 (M1 - 1, M1, M2 - 1, M2, M -
    M1): P[k0] within c (A N / 2)^2 of (A N / 2)^2, and every bin, the tone's and the leakage bins, within bound_bin of
    the f64 spectrum of the f32 series (_run's check_stage1); a permutation fault of the transform shows here on its own.
    The long frames take the tones two at a time."""
    n = 1 << log2n
    amp = 3.0
    bins = _tone_bins(log2n)
    assert len(set(bins)) == 8
    full, c = (amp * n / 2.0) ** 2, periodlong_ref.bound(log2n)
    per = 8 if log2n <= 18 else 2
    for first in range(0, 8, per):
        ks = bins[first:first + per]
        x = np.stack([amp * np.cos((k0 * np.arange(n, dtype=np.int64) % n) * (2.0 * np.pi / n) + 0.3) for k0 in ks]).astype(np.float32)
        _, _, power, _ = _run(built, engine, x, log2n, 1, 16, 64, 1, name=("tones", log2n), bare=False)
        for t, k0 in enumerate(ks):
            p = power[t].astype(np.float64)
            assert abs(p[k0] - full) <= c * full, (log2n, k0, p[k0], full)
            p[k0] = 0.0
            assert p.max() <= c * full, (log2n, k0, p.argmax(), p.max(), c * full)      # what bound_bin holds far tighter


@pytest.mark.parametrize("log2n", [16, 20])
def test_impulses(built, engine, log2n):
    """an impulse at n = 0 and at an odd n: the spectrum of a - a / nsamp at one sample and - a / nsamp elsewhere is flat
    but for the mean's term, which the f64 spectrum carries too; every flat bin within bound_bin of it (_run's
    check_stage1), and the sum over the trial as before"""
    n, m = 1 << log2n, 1 << (log2n - 1)
    x = np.zeros((2, n), np.float32)
    x[0, 0], x[1, 4097] = 1.0, 1.0
    _, _, power, _ = _run(built, engine, x, log2n, 5, 64, 64, 1, name=("impulse", log2n), bare=False)
    c = periodlong_ref.bound(log2n)
    for t in range(2):
        p = power[t].astype(np.float64)
        assert p[0] + np.abs(p[1:] - 1.0).sum() <= c * (m - 1), (t, p[:3], np.abs(p[1:] - 1.0).sum())     # sum P = M - 1


def test_crafted_trials(built, engine):
    """an all-zero trial (0 / 0: NaN rows, every peak (-Inf, -1)); an impulse, whose spectrum is flat: whole segments of
    equal maxima, taken at their first k or at klo; tones at the first and the last bin of a segment and at klo; rows with
    exponents over 2^-6 .. 2^6"""
    log2n, seg = 16, 64
    n, m = 1 << log2n, 1 << (log2n - 1)
    t = np.arange(n)
    rng = np.random.default_rng(7)
    x = np.zeros((6, n), np.float32)
    x[1, 0] = 1.0
    tone = lambda k0: 5.0 * np.cos(2.0 * np.pi * k0 * t / n)
    x[2] = (tone(3 * seg) + 0.01 * rng.standard_normal(n) + 2.0).astype(np.float32)             # the first k of segment 3
    x[3] = (tone(4 * seg - 1) + 0.01 * rng.standard_normal(n) + 2.0).astype(np.float32)         # the last k of segment 3
    x[4] = (tone(200) + 0.01 * rng.standard_normal(n) + 2.0).astype(np.float32)                 # klo itself
    x[5] = (period_ref.signed_exponent_series(1, n, log2n, seed=8)[0].astype(np.float64) * 64.0).astype(np.float32)
    for klo in (1, 200):
        best, at, power, white = _run(built, engine, x, log2n, 5, 64, seg, klo, name=("crafted", klo), bare=klo == 1)
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
    log2n, plan = 17, (5, 64, 256, 8)
    x = _noise(5, 100000, seed=21)
    clean = _run(built, engine, x, log2n, *plan, name="clean", bare=False)
    bad = x.copy()
    bad[1, 1234], bad[3, 7] = np.nan, np.inf
    finite = np.array([True, False, True, False, True])
    got = _run(built, engine, bad, log2n, *plan, name="bad", finite=finite, bare=False)
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
    shape = (ntrials, levels, m // seg)
    _check_behind(power, white, best[:n1].reshape(shape), at[:n1].reshape(shape), levels, norm, seg, klo, what)
    return best, at, power, white


def test_one_plan_many_runs_and_two_plans(built, engine):
    """One plan at three nsamp in turn into preset buffers (nsamp above its N refused); then beside a second plan of
    another frame length, their runs interleaved on two streams, each plan's runs ordered on its own"""
    import torch
    handle = built.torch_stream_handle
    shapes = ((16, 5, 64, 64, 8), (20, 3, 2048, 2048, 100))
    ntrials = 2
    hosts = [_noise(ntrials, 1 << sh[0], seed=31 + j) for j, sh in enumerate(shapes)]
    series = [_on_device(torch, h) for h in hosts]
    plans = [built.PeriodLongPlan(engine, *sh, max_trials=ntrials) for sh in shapes]
    log2n, levels, norm, seg, klo = shapes[0]
    n, m = 1 << log2n, 1 << (log2n - 1)
    for nsamp in (1, 50000, n):
        outs = _outputs(torch, ntrials, levels, m // seg, m)
        plans[0].run(series[0].data_ptr(), n, ntrials, nsamp, *[o.data_ptr() for o in outs], stream=handle())
        torch.cuda.synchronize()
        _check_outputs(outs, hosts[0], *shapes[0], nsamp, nsamp)
    outs = _outputs(torch, ntrials, levels, m // seg, m)
    rc = plans[0].run(series[0].data_ptr(), n + 4, 1, n + 1, *[o.data_ptr() for o in outs], stream=handle(), check=False)
    assert rc == -1 and "nsamp must be at most the plan's N" in built.periodlong_last_error()
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    for s in streams:
        s.wait_stream(torch.cuda.current_stream())
    reps = 2
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
    """tests/test_graph_gpu.py's pattern for this plan: rtlws_periodlong_run captured on a side stream enqueues nothing,
    replays give the eager launch's bits and the restatement's, twice; three trials through a workspace of two, so that
    the graph holds two groups"""
    import torch
    eng = built.Engine(0)
    shape, ntrials, nsamp = (17, 5, 64, 256, 8), 3, 100000
    m = 1 << (shape[0] - 1)
    host = _noise(ntrials, nsamp, seed=41)
    series = _on_device(torch, host)
    plan = built.PeriodLongPlan(eng, *shape, max_trials=2)
    outs = _outputs(torch, ntrials, shape[1], m // shape[3], m)
    before = [o.clone() for o in outs]
    g = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        with torch.cuda.graph(g, stream=side):
            plan.run(series.data_ptr(), nsamp, ntrials, nsamp, *[o.data_ptr() for o in outs], stream=built.torch_stream_handle())
    torch.cuda.current_stream().wait_stream(side)
    assert all(torch.equal(o, b) for o, b in zip(outs, before))              # capture enqueued nothing
    for _ in range(2):
        for o, b in zip(outs, before):
            o.copy_(b)
        g.replay()
        torch.cuda.synchronize()
        _check_outputs(outs, host, *shape, nsamp, "replay")
    eager = _outputs(torch, ntrials, shape[1], m // shape[3], m)
    plan.run(series.data_ptr(), nsamp, ntrials, nsamp, *[o.data_ptr() for o in eager], stream=built.torch_stream_handle())
    torch.cuda.synchronize()
    assert all(torch.equal(e.view(torch.int32), o.view(torch.int32)) for e, o in zip(eager, outs))
    plan.close()
    eng.close()


# ---- the chain on the device -------------------------------------------------------------------------------------

CHAIN_LOG2N, CHAIN_NSAMP, CHAIN_NCHAN, CHAIN_NTRIALS, CHAIN_TRIAL, CHAIN_P0 = 16, 50000, 16, 9, 4, 137.3
CHAIN_PLAN = (5, 64, 256, 8)                                 # levels, norm, seg, klo


def chain_scene():
    """(rows float32 [nrows, 16], delays int32 [9, 16]): noise of mean 4 and deviation 1 in every channel, and a train of
    pulses 137.3 rows apart (a Gaussian of deviation 1.2 rows, amplitude 0.5) that arrives in channel i (15 - i) *
    CHAIN_TRIAL rows late: trial t removes (15 - i) t rows, one row per channel and DM step"""
    delays = (np.arange(CHAIN_NTRIALS)[:, None] * (CHAIN_NCHAN - 1 - np.arange(CHAIN_NCHAN))[None, :]).astype(np.int32)
    nrows = CHAIN_NSAMP + int(delays.max())
    rng = np.random.default_rng(2024)
    rows = 4.0 + rng.standard_normal((nrows, CHAIN_NCHAN))
    r = np.arange(nrows, dtype=np.float64)
    for i in range(CHAIN_NCHAN):
        phase = (r - delays[CHAIN_TRIAL, i] - 20.0) / CHAIN_P0
        d = (phase - np.rint(phase)) * CHAIN_P0
        rows[:, i] += 0.5 * np.exp(-0.5 * (d / 1.2) ** 2)
    return rows.astype(np.float32), delays


def chain_lnq(best, at, lnq):
    """lnq [ntrials, levels, nseg] of the peaks (0 where nothing was taken)"""
    out = np.zeros(best.shape)
    for idx in np.ndindex(*best.shape):
        if at[idx] >= 0:
            out[idx] = lnq(float(best[idx]), 1 << idx[1])
    return out


def chain_conditions(lnq, at, samples):
    """the smallest lnq lies at the injected trial, its period is within one fundamental bin (P0^2 / N samples) of P0,
    and it is at least 5 below every trial more than one DM step away -> (the period, its lnq, the smallest lnq
    elsewhere)"""
    idx = np.unravel_index(np.argmin(lnq), lnq.shape)
    period = samples(CHAIN_LOG2N, idx[1], int(at[idx]))
    per_trial = lnq.reshape(lnq.shape[0], -1).min(axis=1)
    others = min(per_trial[t] for t in range(lnq.shape[0]) if abs(t - CHAIN_TRIAL) > 1)
    assert idx[0] == CHAIN_TRIAL, idx
    assert abs(period - CHAIN_P0) <= CHAIN_P0 * CHAIN_P0 / (1 << CHAIN_LOG2N), period
    assert lnq[idx] <= others - 5.0, (lnq[idx], others)
    return period, lnq[idx], others


def chain_chi2(chi2, prof, hits, series, nsamp):
    x = series[:, :nsamp].astype(np.float64)
    return [chi2(prof[t, 0, 0], hits[0, 0], x[t].sum(), (x[t] * x[t]).sum(), nsamp) for t in range(series.shape[0])]


def test_end_to_end_on_the_device(built, engine):
    """dedisp -> periodlong -> fold with no copy in between: chain_scene's waterfall (16 channels, 364 dispersed pulses
    137.3 rows apart, 50 000 dedispersed samples, nine trial DMs, the pulses' own at trial 4) at log2n 16, levels 5,
    norm 64, seg 256, klo 8.

    The conditions were fixed ahead on the CPU with the restatements' chain (dedisp_ref, periodlong_ref.power rounded to
    f32, period_ref's stages 2 - 4, fold_ref): there the smallest lnq, -337.9, lies at trial 4, level 4, bin 7637:
    2^20 / 7637 = 137.302 samples (one fundamental bin is 0.288); the smallest lnq of every trial more than one DM step
    away is -53.8 (284 above; the condition: at least 5), trials 3 and 5 have -93.5 and -94.9; folding every trial at
    rtlws_fold_step(137.302) into 16 bins gives chi2 1317 at trial 4 against 517 at the next.  The test recomputes them
    from the restatements before it looks at the device's peaks."""
    log2n, nsamp, t0 = CHAIN_LOG2N, CHAIN_NSAMP, CHAIN_TRIAL
    levels, norm, seg, klo = CHAIN_PLAN
    nbins = 16
    rows, delays = chain_scene()
    nrows, nchan = rows.shape
    ntrials = delays.shape[0]
    m = 1 << (log2n - 1)
    nseg = m // seg
    stride = (nsamp + 3) // 4 * 4 + 4
    # the restatements' chain meets the conditions by itself
    series = dedisp_ref.dedisp_ref(rows, delays, None, nsamp)
    ref_power = np.stack([periodlong_ref.power(series[t], log2n) for t in range(ntrials)]).astype(np.float32)
    _, ref_best, ref_at = period_ref.period_ref(ref_power, levels, norm, seg, klo)
    ref_period, ref_low, ref_others = chain_conditions(chain_lnq(ref_best, ref_at, period_ref.lnq), ref_at, periodlong_ref.samples)
    ref_prof, ref_hits = fold_ref.fold_ref(series, [fold_ref.step_of(ref_period)], [0], nbins, 65536, nsamp)
    ref_chi = chain_chi2(fold_ref.chi2, ref_prof, ref_hits, series, nsamp)
    assert int(np.argmax(ref_chi)) == t0

    dd, per = built.DedispPlan(engine, delays), built.PeriodLongPlan(engine, log2n, levels, norm, seg, klo, max_trials=ntrials)
    bufs = [engine.upload(rows), engine.upload(np.full((ntrials, stride), np.nan, np.float32)),
            engine.alloc(ntrials * levels * nseg * 4), engine.alloc(ntrials * levels * nseg * 4), engine.alloc(ntrials * m * 4),
            engine.alloc(ntrials * m * 4), engine.alloc(ntrials * nbins * 4), engine.alloc(nbins * 4)]
    ff = None
    try:
        dd.run(bufs[0], nsamp, bufs[1], in_stride=nchan, out_stride=stride)
        per.run(bufs[1], stride, ntrials, nsamp, bufs[2], bufs[3], bufs[4], bufs[5])
        engine.sync()
        best = engine.download(bufs[2], np.float32, (ntrials, levels, nseg))
        at = engine.download(bufs[3], np.int32, (ntrials, levels, nseg))
        # the candidate goes back to the device as one period: the series never left it
        got_lnq = chain_lnq(best, at, built.period_lnq)
        period, low, others = chain_conditions(got_lnq, at, built.periodlong_samples)
        step = built.fold_step(period)
        ff = built.FoldPlan(engine, [step], [0], nbins, 65536)
        ff.run(bufs[1], stride, ntrials, nsamp, bufs[6], bufs[7])
        engine.sync()
        dev_series = engine.download(bufs[1], np.float32, (ntrials, stride))
        power = engine.download(bufs[4], np.float32, (ntrials, m))
        white = engine.download(bufs[5], np.float32, (ntrials, m))
        prof = engine.download(bufs[6], np.float32, (ntrials, 1, 1, nbins))
        hits = engine.download(bufs[7], np.uint32, (1, 1, nbins))
    finally:
        for plan in (dd, per, ff):
            if plan is not None:
                plan.close()
        for b in bufs:
            b.free()
    _same_bits(dev_series[:, :nsamp], series, "series")
    assert np.isnan(dev_series[:, nsamp:]).all()
    # the device: stage 1 within its bound of the restatement's, stages 2 - 4 bit for bit from its own rows
    _check_stage1(power, series, log2n, nsamp, "chain")
    _check_behind(power, white, best, at, levels, norm, seg, klo, "chain")
    assert period == ref_period and step == fold_ref.step_of(period)
    _same_bits(prof, ref_prof, "prof")
    assert np.array_equal(hits, ref_hits)
    chi = chain_chi2(built.fold_chi2, prof, hits, series, nsamp)
    print("smallest lnq %.1f at trial %d: %.3f samples (the restatements: %.1f, %.3f); %.1f elsewhere; chi2 there %.0f, next %.0f"
          % (low, t0, period, ref_low, ref_period, others, max(chi), sorted(chi)[-2]))
    assert int(np.argmax(chi)) == t0

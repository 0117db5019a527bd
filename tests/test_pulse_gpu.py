"""GPU suite of include/rtlws_pulse.h (librtlws_pulse.so) against its numpy restatement (tests/pulse_ref.py): peaks on
uint32 views, places exactly, moments on uint64 views; NaN in the stride's padding and behind samples_needed, a preset
pattern behind every output array; signed data with exponents over 2^-6 .. 2^6.  Every plan form at every border of the
tile and the segment, planted maxima and ties, zeros of both signs, NaN and infinities, the trial counts up to the
limit, a NULL d_mom, a run from a later segment, one plan many times and beside another, graph capture, the f64 bound
on every case, and the chain spectrometer -> dedispersion -> pulse search on the device."""
import numpy as np
import pytest

import dedisp_ref
import pulse_ref
from pulse_ref import LADDER, MIXED16

pytestmark = pytest.mark.gpu

FILL = np.float32(-12345.678)
FIRST_PLANS = {"w1": (1,), "w2": (2,), "w3": (3,), "w257": (257,), "w258": (258,), "w1023": (1023,), "w1024": (1024,), "ladder": LADDER,
               "mixed16": MIXED16}
# ... and the least width whose eight rows of a 1024-output tile pass 32 KiB: pulse_kernel<16384, 4>, the one instantiation
# of the launch table that none of the tables above (nor any other test's) takes (tests/search_family_matrix.py)
PLANS = dict(FIRST_PLANS, w151=(151,))
NOUTS = ("1", "T-1", "T", "T+1", "2T+5")
SEGS = ("64", "68", "T", "T+4", "2T+4", ">nout")
WORST = {}


SIZES = {"1": lambda t: 1, "T-1": lambda t: t - 1, "T": lambda t: t, "T+1": lambda t: t + 1, "2T+5": lambda t: 2 * t + 5,
         "64": lambda t: 64, "68": lambda t: 68, "T+4": lambda t: t + 4, "2T+4": lambda t: 2 * t + 4}


def _size(code, tile, nout=None):
    if code == ">nout":
        return max(64, (nout + 4 + 3) // 4 * 4)
    return SIZES[code](tile)


def _same_bits(got, want, what=None):
    """bit for bit on integer views, NaN by place (the default NaN of the host's additions and the device's may differ)"""
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape)
    view = {4: np.uint32, 8: np.uint64}[got.dtype.itemsize]
    nan = np.isnan(want) if got.dtype.kind == "f" else np.zeros(want.shape, bool)
    gnan = np.isnan(got) if got.dtype.kind == "f" else nan
    bad = (gnan != nan) | (~nan & (got.view(view) != want.view(view)))
    assert not bad.any(), (what, np.argwhere(bad)[:5], got[bad][:5], want[bad][:5])


def _run(built, engine, x, widths, seg, nout, want_moments=True, name=None):
    """x float32 [ntrials, >= samples_needed] through Engine.pulse with NaN in the padding and behind samples_needed and
    preset guards behind the outputs, against the restatement; -> (peak, at, mom) of the device"""
    ntrials, nw = x.shape[0], len(widths)
    need, nseg = pulse_ref.samples_needed(widths, nout), pulse_ref.segments(nout, seg)
    stride = (need + 3) // 4 * 4 + 4
    padded = np.full((ntrials, stride), np.nan, np.float32)
    padded[:, :need] = x[:, :need]
    peak, at, mom = engine.pulse(padded, widths, seg, nout=nout, in_stride=stride, want_moments=want_moments, fill=FILL)
    n1, n2, guard = ntrials * nw * nseg, ntrials * nseg * 2, built.PULSE_GUARD
    assert peak.shape == at.shape == (n1 + guard,) and mom.shape == (n2 + guard,)
    assert np.all(peak[n1:].view(np.uint32) == FILL.view(np.uint32)) and np.all(at[n1:] == FILL.view(np.int32)) and np.all(mom[n2:] == np.float64(FILL))
    peak, at, mom = peak[:n1].reshape(ntrials, nw, nseg), at[:n1].reshape(ntrials, nw, nseg), mom[:n2].reshape(ntrials, nseg, 2)
    want_peak, want_at, want_mom = pulse_ref.pulse_ref(x, widths, seg, nout)
    assert not np.isnan(peak).any()
    _same_bits(peak, want_peak, (name, "peak"))
    assert np.array_equal(at, want_at), (name, np.argwhere(at != want_at)[:5])
    if want_moments:
        _same_bits(mom, want_mom, (name, "mom"))
    else:
        assert np.all(mom == np.float64(FILL)), name
    # the device's own peaks against the f64 sum of their windows: within depth 2^-24 sum|terms|
    x64, rows = x[:, :need].astype(np.float64), np.arange(ntrials)[:, None]
    with np.errstate(invalid="ignore", over="ignore"):
        for k, w in enumerate(widths):
            b64, lim, where = pulse_ref.boxcar(x64, w), pulse_ref.bound(x[:, :need], w), np.maximum(at[:, k], 0)
            ok = (at[:, k] >= 0) & np.isfinite(b64[rows, where]) & np.isfinite(lim[rows, where])
            err = np.abs(peak[:, k].astype(np.float64) - b64[rows, where])
            assert np.all(err[ok] <= lim[rows, where][ok]), (name, w)
    return peak, at, mom


def test_the_cases_cover_the_borders(built):
    """The shapes of test_every_plan_at_every_border: every tile size, every LDS size, tiles of one output and of
    tile_out, a last segment of one output, seg above nout, halos one and two past a multiple of 256"""
    tiles, sizes, both = set(), set(), set()
    for name, widths in PLANS.items():
        rc, _, threads, lds, tile, kept, _ = built.pulse_geometry(widths, 64)
        assert rc == 0 and threads == 256 and (tile, lds, kept) == pulse_ref.plan(widths)[:3]
        tiles.add(tile)
        sizes.add(lds)
        both.add((tile, lds))
    assert tiles == {1024, 512, 256} and sizes == {16384, 32768, 65536}
    assert both == {(1024, 16384), (1024, 32768), (1024, 65536), (512, 65536), (256, 65536)}          # the five entries of pulse.hip's launch table
    assert (1024 + 257 - 1) % 256 == 0 and (1024 + 258 - 1) % 256 == 1            # level 0 of a full tile, in lanes
    t = 1024
    assert _size("T+1", t) % _size("T", t) == 1                                   # a last segment of one output
    assert _size(">nout", t, 5) > 5 and _size(">nout", t, 2 * t + 5) > 2 * t + 5 and _size(">nout", t, 2 * t + 5) % 4 == 0


@pytest.mark.parametrize("nout_code", NOUTS)
@pytest.mark.parametrize("plan", list(PLANS))
def test_every_plan_at_every_border(built, engine, plan, nout_code):
    widths = PLANS[plan]
    tile = built.pulse_geometry(widths, 64)[4]
    nout = _size(nout_code, tile)
    seed = list(PLANS).index(plan) * 10 + NOUTS.index(nout_code)
    x = pulse_ref.signed_series(2, pulse_ref.samples_needed(widths, nout), seed)
    for seg_code in SEGS:
        seg = _size(seg_code, tile, nout)
        rc, blocks, _, _, _, _, nseg = built.pulse_geometry(widths, seg, 2, nout)
        assert rc == 0 and nseg == -(-nout // seg) and blocks == 2 * nseg
        _run(built, engine, x, widths, seg, nout, name=(plan, nout_code, seg_code))
    ratio = pulse_ref.worst_ratio(x, widths, nout)
    WORST[(plan, nout_code)] = ratio
    assert ratio <= 1.0
    print("%s nout %s: |B - B64| at most %.4f of depth 2^-24 sum|terms|; the worst of the %d cases so far %.4f"
          % (plan, nout_code, ratio, len(WORST), max(WORST.values())))


def _planted(tile, seg, nout, places, widths, seed, value=np.float32(3.0e6)):
    x = pulse_ref.signed_series(1, pulse_ref.samples_needed(widths, nout), seed)
    for p in places:
        x[0, p] = value
    return x


@pytest.mark.parametrize("plan", ["w1+", "mixed16"])
def test_planted_maxima_and_ties(built, engine, plan):
    """A maximum at the first and at the last n of a segment and of a tile; equal maxima in two tiles and in two lanes of
    one tile: the smaller n wins.  Width 1 is in both tables: its place is the planted sample itself"""
    widths = (1, 3, 8, 100) if plan == "w1+" else MIXED16
    tile = built.pulse_geometry(widths, 64)[4]
    seg, nout = 2 * tile + 4, 3 * (2 * tile + 4)
    for which, places in enumerate(([0], [seg - 1], [seg], [2 * seg - 1], [tile - 1], [tile], [seg + tile - 1], [seg + tile], [2 * tile + 3],
                                    [5, tile + 5], [seg + 7, seg + tile + 7], [tile + 9, tile + 14], [2 * seg + 2 * tile + 1, 2 * seg + 2 * tile + 3],
                                    [63, 64], [255, 256])):
        x = _planted(tile, seg, nout, places, widths, seed=100 + which)
        peak, at, _ = _run(built, engine, x, widths, seg, nout, name=(plan, places))
        s = places[0] // seg
        assert at[0, 0, s] == places[0] and peak[0, 0, s] == np.float32(3.0e6), (places, at[0, 0])


def test_zeros_nan_and_infinities(built, engine):
    widths, seg, nout = (1, 2, 3, 8, 100), 64, 64 * 6
    need = pulse_ref.samples_needed(widths, nout)
    x = pulse_ref.signed_series(4, need, seed=7)
    x[0, 64:64 + 64 + 99] = 0.0                                  # a segment whose every window holds zeros only, of both signs
    x[0, 70:200:3] = -0.0
    x[0, 256:256 + 64 + 99] = -0.0                               # ... and one of -0.0 only: B is -0.0 or +0.0 by the additions
    x[1, 128:128 + 64 + 99] = np.nan                             # an all-NaN segment (and NaN in its neighbours' last windows)
    x[2, :] = -np.inf                                            # an all -Inf trial
    x[3, 100] = np.inf                                           # +Inf wins wherever a window holds it
    x[3, 300] = np.nan                                           # one NaN sample: exactly the windows that hold it lose
    peak, at, mom = _run(built, engine, x, widths, seg, nout, name="special")
    assert np.all(at[0, :, 1] == 64) and np.all(peak[0, :, 1] == 0.0) and np.all(at[0, :, 4] == 256) and np.all(peak[0, :, 4] == 0.0)
    assert peak[0, 0, 1].view(np.uint32) == 0 and peak[0, 0, 4].view(np.uint32) == 0x80000000      # width 1: the sample's own bits
    assert np.all(at[1, :, 2] == -1) and np.all(peak[1, :, 2].view(np.uint32) == 0xFF800000)
    assert np.all(at[2] == -1) and np.all(peak[2].view(np.uint32) == 0xFF800000) and np.all(mom[2, :, 0] == -np.inf) and np.all(mom[2, :, 1] == np.inf)
    for k, w in enumerate(widths):
        assert peak[3, k, 1] == np.inf and at[3, k, 1] == max(64, 100 - w + 1), (w, at[3, k, 1])
        if w > 100 - 64 + 1:
            assert peak[3, k, 0] == np.inf and at[3, k, 0] == 100 - w + 1
        assert not (300 - w + 1 <= at[3, k, 4] <= 300) and np.isfinite(peak[3, k, 4]), (w, at[3, k, 4])
    assert np.isnan(mom[3, 4]).all() and np.isnan(mom[1, 2]).all() and np.isfinite(mom[3, 0]).all()


@pytest.mark.parametrize("ntrials", [1, 2, 4096, 65536])
def test_trial_counts(built, engine, ntrials):
    widths, seg, nout = (1, 3, 8), 64, 64
    x = pulse_ref.signed_series(ntrials, pulse_ref.samples_needed(widths, nout), seed=ntrials)
    assert built.pulse_geometry(widths, seg, ntrials, nout)[1] == ntrials
    _run(built, engine, x, widths, seg, nout, name=ntrials)


def test_null_moments(built, engine):
    widths, seg, nout = (1, 3, 8, 100), 68, 700
    x = pulse_ref.signed_series(2, pulse_ref.samples_needed(widths, nout), seed=11)
    with_mom = _run(built, engine, x, widths, seg, nout)
    without = _run(built, engine, x, widths, seg, nout, want_moments=False)
    _same_bits(with_mom[0], without[0])
    assert np.array_equal(with_mom[1], without[1])


def _on_device(torch, host):
    return torch.from_numpy(np.ascontiguousarray(host)).to(torch.device("cuda", 0))


def _outputs(torch, ntrials, nw, nseg):
    return (_on_device(torch, np.full(ntrials * nw * nseg + 8, FILL, np.float32)), _on_device(torch, np.full(ntrials * nw * nseg + 8, -7, np.int32)),
            _on_device(torch, np.full(ntrials * nseg * 2 + 8, np.float64(FILL), np.float64)))


def _check_outputs(outs, want, ntrials, nw, nseg, what=None):
    peak, at, mom = (o.cpu().numpy() for o in outs)
    n1, n2 = ntrials * nw * nseg, ntrials * nseg * 2
    assert np.all(peak[n1:] == FILL) and np.all(at[n1:] == -7) and np.all(mom[n2:] == np.float64(FILL)), what
    _same_bits(peak[:n1].reshape(ntrials, nw, nseg), want[0], (what, "peak"))
    assert np.array_equal(at[:n1].reshape(ntrials, nw, nseg), want[1]), what
    _same_bits(mom[:n2].reshape(ntrials, nseg, 2), want[2], (what, "mom"))


def test_a_run_from_a_later_segment(built, engine):
    """The run over the samples from 3 seg on: the whole run's peaks and moments from segment 3 on, `at` shifted"""
    import torch
    widths = MIXED16
    tile = built.pulse_geometry(widths, 64)[4]
    seg, ntrials = tile + 4, 2
    nout = 5 * seg + 9
    need = pulse_ref.samples_needed(widths, nout)
    stride = (need + 3) // 4 * 4
    host = np.full((ntrials, stride), np.nan, np.float32)
    host[:, :need] = pulse_ref.signed_series(ntrials, need, seed=13)
    whole = pulse_ref.pulse_ref(host, widths, seg, nout)
    series = _on_device(torch, host)
    plan = built.PulsePlan(engine, widths, seg)
    assert plan.samples_needed(nout) == need and plan.segments(nout) == 6
    for first in (0, 3):
        nseg = 6 - first
        outs = _outputs(torch, ntrials, len(widths), nseg)
        plan.run(series.data_ptr() + 4 * first * seg, stride, ntrials, nout - first * seg, outs[0].data_ptr(), outs[1].data_ptr(), outs[2].data_ptr(),
                 stream=built.torch_stream_handle())
        torch.cuda.synchronize()
        want = (whole[0][:, :, first:], whole[1][:, :, first:] - first * seg, whole[2][:, first:])
        _check_outputs(outs, want, ntrials, len(widths), nseg, first)
    plan.close()


def test_one_plan_many_runs_and_two_plans(built, engine):
    """One plan at three nout in turn into preset buffers; then beside a second plan of another table and seg, their runs
    interleaved on two streams"""
    import torch
    handle = built.torch_stream_handle
    tables = ((LADDER, 64), ((3, 258), 1028))
    tile = built.pulse_geometry(LADDER, 64)[4]
    nouts = (1, tile, 2 * tile + 5)
    ntrials = 3
    hosts, series, plans = [], [], []
    for j, (widths, seg) in enumerate(tables):
        need = pulse_ref.samples_needed(widths, nouts[-1])
        hosts.append(pulse_ref.signed_series(ntrials, (need + 3) // 4 * 4, seed=20 + j))
        series.append(_on_device(torch, hosts[-1]))
        plans.append(built.PulsePlan(engine, widths, seg))
    for nout in nouts:
        widths, seg = tables[0]
        nseg = plans[0].segments(nout)
        outs = _outputs(torch, ntrials, len(widths), nseg)
        plans[0].run(series[0].data_ptr(), hosts[0].shape[1], ntrials, nout, outs[0].data_ptr(), outs[1].data_ptr(), outs[2].data_ptr(), stream=handle())
        torch.cuda.synchronize()
        _check_outputs(outs, pulse_ref.pulse_ref(hosts[0], widths, seg, nout), ntrials, len(widths), nseg, nout)
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    for s in streams:
        s.wait_stream(torch.cuda.current_stream())
    nout, reps = nouts[-1], 3
    outs = [[_outputs(torch, ntrials, len(w), plans[j].segments(nout)) for _ in range(reps)] for j, (w, _) in enumerate(tables)]
    for rep in range(reps):
        for j in (0, 1):
            o = outs[j][rep]
            plans[j].run(series[j].data_ptr(), hosts[j].shape[1], ntrials, nout, o[0].data_ptr(), o[1].data_ptr(), o[2].data_ptr(),
                         stream=handle(streams[j]))
    torch.cuda.synchronize()
    for j, (widths, seg) in enumerate(tables):
        want = pulse_ref.pulse_ref(hosts[j], widths, seg, nout)
        for rep in range(reps):
            _check_outputs(outs[j][rep], want, ntrials, len(widths), plans[j].segments(nout), (j, rep))
    for plan in plans:
        plan.close()


def test_capture_and_replay(built):
    """tests/test_graph_gpu.py's pattern for this plan: rtlws_pulse_run captured on a side stream enqueues nothing, replays
    give the eager launch's bits and the restatement's, twice"""
    import torch
    eng = built.Engine(0)
    widths, seg, ntrials = MIXED16, 260, 3
    tile = built.pulse_geometry(widths, seg)[4]
    nout = 2 * tile + 5
    need = pulse_ref.samples_needed(widths, nout)
    host = pulse_ref.signed_series(ntrials, (need + 3) // 4 * 4, seed=31)
    series = _on_device(torch, host)
    plan = built.PulsePlan(eng, widths, seg)
    nseg = plan.segments(nout)
    outs = _outputs(torch, ntrials, len(widths), nseg)
    before = [o.clone() for o in outs]
    g = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        with torch.cuda.graph(g, stream=side):
            plan.run(series.data_ptr(), host.shape[1], ntrials, nout, outs[0].data_ptr(), outs[1].data_ptr(), outs[2].data_ptr(),
                     stream=built.torch_stream_handle())
    torch.cuda.current_stream().wait_stream(side)
    assert all(torch.equal(o, b) for o, b in zip(outs, before))              # capture enqueued nothing
    want = pulse_ref.pulse_ref(host, widths, seg, nout)
    for _ in range(2):
        for o, b in zip(outs, before):
            o.copy_(b)
        g.replay()
        torch.cuda.synchronize()
        _check_outputs(outs, want, ntrials, len(widths), nseg, "replay")
    eager = _outputs(torch, ntrials, len(widths), nseg)
    plan.run(series.data_ptr(), host.shape[1], ntrials, nout, eager[0].data_ptr(), eager[1].data_ptr(), eager[2].data_ptr(),
             stream=built.torch_stream_handle())
    torch.cuda.synchronize()
    assert torch.equal(eager[0].view(torch.int32), outs[0].view(torch.int32)) and torch.equal(eager[1], outs[1])
    assert torch.equal(eager[2].view(torch.int64), outs[2].view(torch.int64))
    plan.close()
    eng.close()


# ---- the chain on the device -------------------------------------------------------------------------------------

PULSE_ROWS = 8                                   # the injected pulse lasts this many spectrometer rows
CHAIN_WIDTHS = (1, 2, 4, 8, 16, 32)


def dispersed_capture(built, t0, n0, nout, rows_wide=PULSE_ROWS):
    """A capture of noise with a burst per channel rows_wide rows long, channel i's from where row n0 + d[t0][i] of the
    spectrometer (k = 6, 4 taps, K = 4, hop 32, shifted) is formed, d the third table of dedisp_ref.DELAY_SETS"""
    k, T, K, hop = 6, 4, 4, 32
    M = 1 << k
    delays = dedisp_ref.delays(*dedisp_ref.DELAY_SETS[2])
    nrows = dedisp_ref.rows_needed(delays, None, nout)
    nsamples = (nrows * K - 1) * hop + T * M
    b = dedisp_ref.hashed_ints(2 * nsamples, 255, seed=41).reshape(nsamples, 2).astype(np.float64)
    x = (b[:, 0] - 127.5) / 16.0 + 1j * (b[:, 1] - 127.5) / 16.0
    s = np.arange(rows_wide * K * hop)
    for i in range(M):
        c = (i + M // 2) % M
        at = (n0 + int(delays[t0, i])) * K * hop + T * M // 2
        x[at:at + s.size] += 3.0 * np.exp(2j * np.pi * c * (at + s) / M)
    iq = np.clip(np.rint(np.stack([x.real, x.imag], axis=1) + 128.0), 0, 255).astype(np.uint8)
    return iq, built.pfb_design(k, T), delays, nrows


def strongest(peak, at, mom, widths, seg, nout):
    """(snr, t, k, s) of the largest rtlws_pulse_snr's expression, the noise of a trial from all its segments' moments"""
    best = (-np.inf, -1, -1, -1)
    for t in range(peak.shape[0]):
        sum1, sum2 = mom[t, :, 0].sum(), mom[t, :, 1].sum()
        for k, w in enumerate(widths):
            for s in range(peak.shape[2]):
                v = pulse_ref.snr(peak[t, k, s], w, sum1, sum2, nout)
                if v > best[0]:
                    best = (float(v), t, k, s)
    return best


def test_end_to_end_on_the_device(built, engine):
    """pfbspec -> dedisp -> pulse with no copy in between: the spectrometer's rows and the dedispersed series stay on the
    device; bit for bit the restatements' chain over the downloaded rows; the largest rtlws_pulse_snr at the injected
    trial and segment, at a width within a factor of two of the injected one, `at` within that width of the injected row"""
    t0, n0, seg = 20, 100, 64
    nout_d = 300                                                 # dedispersed samples per trial
    nout = nout_d - CHAIN_WIDTHS[-1] + 1                         # boxcar outputs: every window inside the series
    iq, taps, delays, nrows = dispersed_capture(built, t0, n0, nout_d)
    ntrials, M = delays.shape
    stride = (nout_d + 3) // 4 * 4 + 4
    spec, dd, pp = built.PfbSpecPlan(engine, 6, taps), built.DedispPlan(engine, delays), built.PulsePlan(engine, CHAIN_WIDTHS, seg)
    assert pp.samples_needed(nout) == nout_d and dd.rows_needed(nout_d) == nrows
    nseg, nw = pp.segments(nout), len(CHAIN_WIDTHS)
    bufs = [engine.upload(iq), engine.alloc(nrows * M * 4), engine.upload(np.full((ntrials, stride), np.nan, np.float32)),
            engine.alloc(ntrials * nw * nseg * 4), engine.alloc(ntrials * nw * nseg * 4), engine.alloc(ntrials * nseg * 16)]
    try:
        spec.run(bufs[0], nrows, 4, bufs[1], hop=32, shifted=True)
        dd.run(bufs[1], nout_d, bufs[2], in_stride=M, out_stride=stride)
        pp.run(bufs[2], stride, ntrials, nout, bufs[3], bufs[4], bufs[5])
        engine.sync()
        rows = engine.download(bufs[1], np.float32, (nrows, M))
        peak = engine.download(bufs[3], np.float32, (ntrials, nw, nseg))
        at = engine.download(bufs[4], np.int32, (ntrials, nw, nseg))
        mom = engine.download(bufs[5], np.float64, (ntrials, nseg, 2))
    finally:
        for plan in (spec, dd, pp):
            plan.close()
        for b in bufs:
            b.free()
    series = dedisp_ref.dedisp_ref(rows, delays, None, nout_d)
    want = pulse_ref.pulse_ref(series, CHAIN_WIDTHS, seg, nout)
    _same_bits(peak, want[0], "peak")
    assert np.array_equal(at, want[1])
    _same_bits(mom, want[2], "mom")
    snr, t, k, s = strongest(peak, at, mom, CHAIN_WIDTHS, seg, nout)
    assert np.isclose(snr, built.pulse_snr(peak[t, k, s], CHAIN_WIDTHS[k], mom[t, :, 0].sum(), mom[t, :, 1].sum(), nout), rtol=1e-12)
    print("largest snr %.1f at trial %d, width %d, segment %d, n = %d (injected: trial %d, %d rows from row %d)"
          % (snr, t, CHAIN_WIDTHS[k], s, at[t, k, s], t0, PULSE_ROWS, n0))
    assert (t, s) == (t0, n0 // seg) and PULSE_ROWS // 2 <= CHAIN_WIDTHS[k] <= 2 * PULSE_ROWS
    assert abs(int(at[t, k, s]) - n0) <= CHAIN_WIDTHS[k]

"""GPU suite of include/rtlws_accel.h (librtlws_accel.so) against tests/accel_ref.py and against the composition the
header holds the fused search to.

rtlws_accel_resample bit for bit on uint32 views against accel_ref.resample: nsamp at its borders (and at two lengths
where +-2^40 and 2^39 meet exact ties of the map), tight and wide strides on both sides, NaN in the input's padding and
behind nsamp, a preset pattern behind every output row and in its padding; every (a_first, a_count) of a table of three.
rtlws_accel_search word for word against rtlws_periodlong_run over the device's own resampled series, all four outputs,
with both optional rows, one and none; coefficient 0 against rtlws_periodlong_run on the source; stage 1 of every
virtual trial within periodlong_ref.bound of accel_ref, the bound's premises asserted on every resampled series; every
frame-length path (log2n 16, 19 for rows of 2^14, 20 for the 256-point columns, 22 once); 86 x 3 virtual trials; a group
border inside a trial's accelerations; a NaN trial beside finite ones; graph capture; two plans on two streams; and the
scene of DESIGN.md 4.24 with the chain dedispersion -> search -> resampling of the winner -> folding on the device.

The scene as first worded has nine coefficients (a - 2) * coef_from_shift(10, 60 000), a = 0 .. 8; the ninth,
1 229 823 932 034, is above the library's limit 2^40 = 1 099 511 627 776 (at 60 000 samples 2^40 is a mid-frame shift of
53.6 samples) and rtlws_accel_supported refuses the table.  The scene here keeps a = 0 .. 7, the matched one a = 6 among
them; test_the_scene asserts the refusal of the ninth.

Every virtual trial's every bin is held to accel_ref.bound_bin as well (period_family.check_stage1).  Worst per-bin share
of `bound_bin`, measured on one MI355X (printed by test_the_longer_frames): 0.0011, 0.0030, 0.0029 at log2n 19, 20, 22
(dense noise: ||y||_1 is large; tests/test_period_bins_gpu.py has the sparse series, 0.0199 at log2n 16)."""
import numpy as np
import pytest

import accel_ref
import dedisp_ref
import fold_ref
import period_ref
import periodlong_ref
from period_family import FILL, FILL_BITS, check_stage1, same_bits
from period_family import noise as _noise, padded as _padded

pytestmark = pytest.mark.gpu

TOP = 1 << 40
N16 = 1 << 16


def _same_bits(got, want, what=None):
    """device against device: a NaN's bits count too"""
    same_bits(got, want, what, nan_by_place=False)


def _seeded(seed, count):
    return [int(c) for c in np.random.default_rng(seed).integers(-TOP, TOP + 1, count)]


def _ceil4(n):
    return (n + 3) // 4 * 4


def _resample(built, engine, x, log2n, coefs, nsamp, wide_in=False, wide_out=False, a_first=0, a_count=None, name=None):
    """Engine.accel_resample into a preset buffer: the rows bit for bit accel_ref.resample's, everything else of the
    buffer as it was -> (device rows float32 [ntrials * a_count, out_stride], the restatement [ntrials, a_count, nsamp])"""
    ntrials = x.shape[0]
    a_count = len(coefs) - a_first if a_count is None else a_count
    padded, stride = _padded(x, nsamp, wide_in)
    ostride = _ceil4(nsamp) + (8 if wide_out else 0)
    flat = engine.accel_resample(padded, log2n, coefs, a_first, a_count, nsamp=nsamp, in_stride=stride, out_stride=ostride, fill=FILL)
    n = ntrials * a_count * ostride
    assert flat.shape == (n + built.PERIOD_GUARD,) and np.all(flat[n:].view(np.uint32) == FILL_BITS), name
    rows = flat[:n].reshape(ntrials * a_count, ostride)
    want = accel_ref.resample(x, coefs[a_first:a_first + a_count], nsamp)
    assert not np.isnan(want).any()
    _same_bits(rows[:, :nsamp], want.reshape(ntrials * a_count, nsamp), (name, "resampled"))
    assert np.all(rows[:, nsamp:].view(np.uint32) == FILL_BITS), (name, "padding")
    return rows, want


WORST, WORST_BIN = {}, {}


def _reference(log2n):
    """the f64 spectrum of a resampled series, whose two premises hold"""
    def reference(xs, name):
        ref, nyquist_small, mean_small = periodlong_ref.power_and_premises(xs, log2n)
        if xs.size > 1 and ref.sum() > 0:
            assert nyquist_small and mean_small, name
        return ref
    return reference


def _check_stage1(power, resampled, log2n, nsamp, name):
    """period_family.check_stage1 with a trial's accelerations as its trials: per virtual trial sum |P^ - P| <= c sum P
    and every bin within accel_ref.bound_bin of the f64 spectrum of the resampled series"""
    for t in range(resampled.shape[0]):
        check_stage1(power[t], resampled[t], nsamp, accel_ref.bound(log2n), accel_ref.bound_bin(log2n), _reference(log2n), WORST, WORST_BIN,
                     log2n, (name, t))


def _fused_and_composed(built, engine, x, log2n, plan, coefs, nsamp=None, wide=False, want=(True, True), max_trials=None, name=None, stage1=True):
    """the contract: every word rtlws_accel_search writes (guards included) against rtlws_periodlong_run over the series
    rtlws_accel_resample gives -> (best, at, power, white) of the fused run with a leading [ntrials, naccel]"""
    ntrials, naccel = x.shape[0], len(coefs)
    nsamp = x.shape[1] if nsamp is None else nsamp
    levels, norm, seg, klo = plan
    m = 1 << (log2n - 1)
    rows, want_r = _resample(built, engine, x, log2n, coefs, nsamp, wide_in=wide, wide_out=not wide, name=name)
    rows = rows.copy()
    rows[:, nsamp:] = np.nan
    kw = dict(nsamp=nsamp, fill=FILL, want_power=want[0], want_white=want[1])
    composed = engine.periodlong(rows, log2n, levels, norm, seg, klo, in_stride=rows.shape[1], **kw)
    padded, stride = _padded(x, nsamp, wide)
    fused = engine.accel_search(padded, log2n, levels, norm, seg, klo, coefs, in_stride=stride, max_trials=max_trials, **kw)
    nv = ntrials * naccel
    n1, n2 = nv * levels * (m // seg), nv * m
    for what, f, c, n in zip(("best", "at", "power", "white"), fused, composed, (n1, n1, n2, n2)):
        _same_bits(f, c, (name, what))
        assert f.shape == (n + built.PERIOD_GUARD,) and np.all(f[n:].view(np.uint32) == FILL_BITS), (name, what)
    for f, asked in zip(fused[2:], want):
        assert asked or np.all(f.view(np.uint32) == FILL_BITS), name
    shape = (ntrials, naccel, levels, m // seg)
    best, at = fused[0][:n1].reshape(shape), fused[1][:n1].reshape(shape)
    power, white = fused[2][:n2].reshape(ntrials, naccel, m), fused[3][:n2].reshape(ntrials, naccel, m)
    assert at.dtype == np.int32
    if stage1 and want[0]:
        _check_stage1(power, want_r, log2n, nsamp, name)
    return best, at, power, white


# ---- rtlws_accel_resample ---------------------------------------------------------------------------------------

RESAMPLE_NSAMPS = (1, 2, 5, N16 - 4, N16 - 1, N16)
TIE_NSAMPS = (65281, 65025)                      # L = 2^15 + 2^8 * 127 and 2^15 + 2^9 * 63: ties at c = 2^40, and at 2^39 too


def _tied(nsamp):
    """the smallest coefficient with an exact tie somewhere in a series of nsamp samples"""
    return min(c for c, _ in accel_ref.ties(nsamp, want=16))


def test_resample_is_the_map(built, engine):
    """nsamp at its borders and at the two lengths with exact ties, tight and wide strides on both sides; tables of one
    and of three: 0, +-1, +-2^40, the tied coefficients of both signs, seeded ones"""
    x = _noise(2, N16, seed=1)
    seeded = _seeded(2, 4)
    for nsamp in RESAMPLE_NSAMPS + TIE_NSAMPS:
        tables = [[0], [TOP], [1, -1, seeded[0]], [-TOP, seeded[1], TOP]]
        if nsamp in TIE_NSAMPS:
            pairs = accel_ref.ties(nsamp, want=16)
            assert pairs and all((c * n * (nsamp - 1 - n)) % (1 << 64) == 1 << 63 for c, n in pairs)
            c = _tied(nsamp)
            assert c == (TOP if nsamp == 65281 else TOP // 2)
            tables = [[c, -c, seeded[2]], [-c]]
        for i, coefs in enumerate(tables):
            for wide_in, wide_out in ((False, False), (True, True)) if i % 2 == 0 else ((True, False), (False, True)):
                _resample(built, engine, x, 16, coefs, nsamp, wide_in, wide_out, name=(nsamp, coefs, wide_in, wide_out))


def test_resample_every_window_of_the_table(built, engine):
    """every (a_first, a_count) of a table of three; the same bits whichever window an acceleration is asked through"""
    x = _noise(2, 50000, seed=3)
    coefs = [_seeded(4, 1)[0], -TOP, 7]
    whole, _ = _resample(built, engine, x, 16, coefs, 50000, name="whole")
    whole = whole.reshape(2, 3, -1)
    for a_first in range(3):
        for a_count in range(1, 3 - a_first + 1):
            rows, _ = _resample(built, engine, x, 16, coefs, 50000, wide_out=bool(a_first % 2), a_first=a_first, a_count=a_count, name=(a_first, a_count))
            _same_bits(rows.reshape(2, a_count, -1)[:, :, :50000], whole[:, a_first:a_first + a_count, :50000], (a_first, a_count))
    plan = built.AccelPlan(engine, 16, 1, 16, 64, 1, coefs)
    buf = engine.alloc(64)
    for first, count, word in ((0, 4, "a_first + a_count must be at most naccel"), (3, 1, "at most naccel"), (2, 2, "at most naccel")):
        assert plan.resample(buf, 4, 1, 1, first, count, buf, 4, check=False) == -1 and word in built.accel_last_error()
    assert plan.resample(buf, N16 + 4, 1, N16 + 1, 0, 1, buf, N16 + 4, check=False) == -1 and "nsamp must be at most the plan's N" in built.accel_last_error()
    assert plan.search(buf, N16 + 4, 1, N16 + 1, buf, buf, check=False) == -1 and "nsamp must be at most the plan's N" in built.accel_last_error()
    assert plan.search(buf, 4, 21846, 1, buf, buf, check=False) == -1 and "ntrials * naccel must be at most 65536" in built.accel_last_error()
    plan.close()
    buf.free()


# ---- rtlws_accel_search against the composition -----------------------------------------------------------------

def _plans16():
    """(levels, norm, seg, klo) at log2n 16: levels 1 and 5, norm 16 and 16384, seg 64 and 16384, klo 1 and M - 1"""
    m = N16 // 2
    return ((5, 16, 64, 1), (1, 16384, 16384, m - 1), (5, 16384, 64, m - 1), (1, 16, 16384, 1), (5, 64, 256, 8), (5, 1024, 1024, 8))


SEARCH_TABLES = ([0, TOP, -TOP], [1], [-1, _seeded(5, 1)[0], 1], [TOP], [_seeded(6, 1)[0]], [-TOP, 0, _seeded(7, 1)[0]])


@pytest.mark.parametrize("case", range(6))
def test_search_is_the_composition(built, engine, case):
    """log2n 16: the resampling suite's nsamp and coefficient sets, a plan of _plans16 each, tight and wide strides; the
    optional rows both, one and none; one and two trials"""
    nsamp = RESAMPLE_NSAMPS[case]
    plan, coefs = _plans16()[case], SEARCH_TABLES[case]
    ntrials = 1 + case % 2
    x = _noise(ntrials, N16, seed=60 + case)          # seeds whose two- and five-sample series meet the bound's premises
    full = _fused_and_composed(built, engine, x, 16, plan, coefs, nsamp, wide=bool(case % 2), name=("both", case))
    for want in ((True, False), (False, True), (False, False)):
        got = _fused_and_composed(built, engine, x, 16, plan, coefs, nsamp, wide=bool(case % 2), want=want, name=(want, case))
        _same_bits(got[0], full[0], (case, want, "best"))
        _same_bits(got[1], full[1], (case, want, "at"))
    assert built.accel_geometry(16, *plan, coefs, ntrials)[1:] == accel_ref.geometry(16, plan[2], ntrials, len(coefs))


@pytest.mark.parametrize("nsamp", TIE_NSAMPS)
def test_search_at_the_ties(built, engine, nsamp):
    c = _tied(nsamp)
    _fused_and_composed(built, engine, _noise(1, nsamp, seed=nsamp), 16, (5, 64, 256, 8), [c, -c], name=("ties", nsamp))


@pytest.mark.parametrize("log2n,plan", [(19, (5, 16384, 16384, 100)), (20, (5, 1024, 1024, 8)), (22, (5, 64, 256, 8))])
def test_the_longer_frames(built, engine, log2n, plan):
    """19: rows of 2^14 points; 20: the 256-point columns; 22 once: one trial and two coefficients each"""
    n = 1 << log2n
    nsamp = n - (1 if log2n == 20 else 0)
    x = _noise(1, nsamp, seed=log2n)
    x[0] += (3.0 * np.cos(2.0 * np.pi * np.arange(nsamp) / 37.5)).astype(np.float32)
    coefs = [TOP, -_seeded(log2n, 1)[0] // 2]
    _fused_and_composed(built, engine, x, log2n, plan, coefs, name=("long", log2n))
    print("log2n %d: worst stage-1 error %.3g of the bound, worst bin %.3g of bound_bin %.3g" % (log2n, WORST[log2n], WORST_BIN[log2n], accel_ref.bound_bin(log2n)))


def test_many_virtual_trials(built, engine):
    """86 trials of three accelerations: 258 virtual trials, more than one launch row of 256"""
    x = _noise(86, 30000, seed=86)
    best, at, _, _ = _fused_and_composed(built, engine, x, 16, (2, 64, 256, 8), [TOP, 0, -TOP], name="86 x 3")
    assert best.shape == (86, 3, 2, 128)


def test_coefficient_zero_is_the_plain_search(built, engine):
    """against code this library does not hold: rtlws_periodlong_run on the source itself"""
    plan = (5, 64, 256, 8)
    x = _noise(2, 50000, seed=20)
    got = engine.accel_search(x, 16, *plan, [0])
    want = engine.periodlong(x, 16, *plan)
    for g, w, what in zip(got, want, ("best", "at", "power", "white")):
        _same_bits(g[:, 0], w, what)
    # and as one of three, in the middle
    got = engine.accel_search(x, 16, *plan, [TOP, 0, 12345])
    for g, w, what in zip(got, want, ("best", "at", "power", "white")):
        _same_bits(g[:, 1], w, what)
    assert np.any(got[2][:, 0] != got[2][:, 1])


def test_group_border_inside_a_trial(built, engine):
    """max_trials 4 under three accelerations and three trials: groups of virtual trials 0 - 3, 4 - 7 and 8, the first
    border between accelerations 0 and 1 of trial 1; the virtual trials on either side equal a run of each alone"""
    plan, coefs = (5, 1024, 1024, 8), [_seeded(30, 1)[0], -TOP, TOP]
    x = _noise(3, N16 - 3, seed=31)
    p = built.AccelPlan(engine, 16, *plan, coefs, max_trials=4)
    assert p.workspace_bytes() == 4 * periodlong_ref.trial_bytes(16)
    p.close()
    got = _fused_and_composed(built, engine, x, 16, plan, coefs, max_trials=4, name="groups")
    whole = _fused_and_composed(built, engine, x, 16, plan, coefs, name="one group", stage1=False)
    for g, w in zip(got, whole):
        _same_bits(g, w, "groups of four against one group")
    for v in (3, 4, 7, 8):
        t, a = divmod(v, 3)
        alone = engine.accel_search(x[t:t + 1], 16, *plan, coefs[a:a + 1], max_trials=1)
        for g, w in zip(got, alone):
            _same_bits(g[t, a], w[0, 0], ("virtual trial", v))


def test_a_nan_trial_leaves_the_others_alone(built, engine):
    plan, coefs = (5, 64, 256, 8), [TOP, 0, -TOP]
    x = _noise(3, 60000, seed=40)
    clean = engine.accel_search(x, 16, *plan, coefs)
    bad = x.copy()
    bad[1, 30000] = np.nan
    got = engine.accel_search(bad, 16, *plan, coefs)
    for g, c, what in zip(got, clean, ("best", "at", "power", "white")):
        _same_bits(g[[0, 2]], c[[0, 2]], what)
    assert np.isnan(got[2][1]).all() and np.isnan(got[3][1]).all()


def _on_device(torch, host):
    return torch.from_numpy(np.ascontiguousarray(host)).to(torch.device("cuda", 0))


def _outputs(torch, nv, levels, nseg, m):
    return (_on_device(torch, np.full(nv * levels * nseg + 8, FILL, np.float32)), _on_device(torch, np.full(nv * levels * nseg + 8, 0x5EADBEEF, np.int32)),
            _on_device(torch, np.full(nv * m + 8, FILL, np.float32)), _on_device(torch, np.full(nv * m + 8, FILL, np.float32)))


def _equal_outputs(torch, a, b):
    return all(torch.equal(p.view(torch.int32), q.view(torch.int32)) for p, q in zip(a, b))


def test_capture_and_replay(built):
    """rtlws_accel_search captured on a side stream enqueues nothing; two replays give the eager run's bits, which are
    the composition's; three trials of three accelerations through a workspace of four, so that the graph holds three
    groups"""
    import torch
    eng = built.Engine(0)
    shape, coefs, ntrials, nsamp = (17, 5, 64, 256, 8), [TOP, -5, -TOP], 3, 100000
    m = 1 << (shape[0] - 1)
    nv = ntrials * len(coefs)
    host = _noise(ntrials, nsamp, seed=41)
    series = _on_device(torch, host)
    plan = built.AccelPlan(eng, *shape, coefs, max_trials=4)
    outs = _outputs(torch, nv, shape[1], m // shape[3], m)
    before = [o.clone() for o in outs]
    g = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        with torch.cuda.graph(g, stream=side):
            plan.search(series.data_ptr(), nsamp, ntrials, nsamp, *[o.data_ptr() for o in outs], stream=built.torch_stream_handle())
    torch.cuda.current_stream().wait_stream(side)
    assert _equal_outputs(torch, outs, before)                               # capture enqueued nothing
    eager = _outputs(torch, nv, shape[1], m // shape[3], m)
    plan.search(series.data_ptr(), nsamp, ntrials, nsamp, *[o.data_ptr() for o in eager], stream=built.torch_stream_handle())
    torch.cuda.synchronize()
    assert not _equal_outputs(torch, eager, before)
    for _ in range(2):
        for o, b in zip(outs, before):
            o.copy_(b)
        g.replay()
        torch.cuda.synchronize()
        assert _equal_outputs(torch, eager, outs)
    # the eager run is the composition: the resampled series on the device, then the long-frame plan over them
    resampled = _on_device(torch, np.full((nv, nsamp), np.nan, np.float32))
    plan.resample(series.data_ptr(), nsamp, ntrials, nsamp, 0, len(coefs), resampled.data_ptr(), nsamp, stream=built.torch_stream_handle())
    long_plan = built.PeriodLongPlan(eng, *shape, max_trials=nv)
    composed = _outputs(torch, nv, shape[1], m // shape[3], m)
    long_plan.run(resampled.data_ptr(), nsamp, nv, nsamp, *[o.data_ptr() for o in composed], stream=built.torch_stream_handle())
    torch.cuda.synchronize()
    assert _equal_outputs(torch, eager, composed)
    _same_bits(resampled.cpu().numpy(), accel_ref.resample(host, coefs).reshape(nv, nsamp), "resampled")
    plan.close()
    long_plan.close()
    eng.close()


def test_two_plans_on_two_streams(built, engine):
    """two plans of two frame lengths, their runs interleaved on two streams, each plan's runs ordered on its own: every
    repetition has the bits of the plan's run alone"""
    import torch
    handle = built.torch_stream_handle
    shapes = ((16, 5, 64, 64, 8), (17, 3, 2048, 2048, 100))
    tables = ([TOP, 0], [-TOP, 3, _seeded(50, 1)[0]])
    ntrials = 2
    hosts = [_noise(ntrials, 1 << sh[0], seed=51 + j) for j, sh in enumerate(shapes)]
    series = [_on_device(torch, h) for h in hosts]
    plans = [built.AccelPlan(engine, *sh, tb, max_trials=3) for sh, tb in zip(shapes, tables)]
    sizes = [(ntrials * len(tb), sh[1], (1 << (sh[0] - 1)) // sh[3], 1 << (sh[0] - 1)) for sh, tb in zip(shapes, tables)]
    alone = []
    for j, sh in enumerate(shapes):
        outs = _outputs(torch, *sizes[j])
        plans[j].search(series[j].data_ptr(), 1 << sh[0], ntrials, 1 << sh[0], *[o.data_ptr() for o in outs], stream=handle())
        torch.cuda.synchronize()
        alone.append(outs)
        want = engine.accel_search(hosts[j], *sh, tables[j])
        _same_bits(outs[0].cpu().numpy()[:want[0].size], want[0].reshape(-1), (j, "best"))
        _same_bits(outs[2].cpu().numpy()[:want[2].size], want[2].reshape(-1), (j, "power"))
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    for s in streams:
        s.wait_stream(torch.cuda.current_stream())
    reps = 2
    outs = [[_outputs(torch, *sizes[j]) for _ in range(reps)] for j in range(2)]
    for rep in range(reps):
        for j, sh in enumerate(shapes):
            plans[j].search(series[j].data_ptr(), 1 << sh[0], ntrials, 1 << sh[0], *[o.data_ptr() for o in outs[j][rep]], stream=handle(streams[j]))
    torch.cuda.synchronize()
    for j in range(2):
        for rep in range(reps):
            assert _equal_outputs(torch, outs[j][rep], alone[j]), (j, rep)
    for plan in plans:
        plan.close()


# ---- the scene and the chain on the device ----------------------------------------------------------------------

SCENE_LOG2N, SCENE_NSAMP, SCENE_P0, SCENE_MATCH, SCENE_NACCEL = 16, 60000, 137.3, 6, 8
SCENE_PLAN = (5, 64, 256, 8)                                 # levels, norm, seg, klo
SCENE_NCHAN = 4
SCENE_DELAYS = np.array([[0, 3, 7, 12]], np.int32)


def scene_coefs(coef_from_shift):
    step = coef_from_shift(10.0, SCENE_NSAMP)
    return [(a - 2) * step for a in range(SCENE_NACCEL)], 6 * step


def scene_rows(coefs):
    """rows float32 [nsamp + 12, 4]: in every channel noise of mean 1 and deviation 1 / 2 -- a sum of mean 4 and deviation
    1 -- and a quarter of a train of Gaussian pulses (deviation 1.2 samples, amplitude 1 in the sum) at m_k = k P + c' k P
    (L - k P), P = 137.3, c' the matched coefficient's; channel i lags by its delay, which the one DM trial removes"""
    last = SCENE_NSAMP - 1
    cp = coefs[SCENE_MATCH] / 2.0 ** 64
    nrows = SCENE_NSAMP + int(SCENE_DELAYS.max())
    rng = np.random.default_rng(7)
    rows = 1.0 + 0.5 * rng.standard_normal((nrows, SCENE_NCHAN))
    k = np.arange(int(last / SCENE_P0) + 1) * SCENE_P0
    centres = k + cp * k * (last - k)
    r = np.arange(nrows, dtype=np.float64)
    for i in range(SCENE_NCHAN):
        for lo in range(0, centres.size, 64):
            d = (r - SCENE_DELAYS[0, i])[:, None] - centres[None, lo:lo + 64]
            rows[:, i] += 0.25 * np.exp(-0.5 * (d / 1.2) ** 2).sum(axis=1)
    return rows.astype(np.float32)


def scene_lnq(best, at, lnq):
    """lnq [naccel, levels, nseg] of the peaks (0 where nothing was taken)"""
    out = np.zeros(best.shape)
    for idx in np.ndindex(*best.shape):
        if at[idx] >= 0:
            out[idx] = lnq(float(best[idx]), 1 << idx[1])
    return out


def scene_conditions(lnq, at, samples):
    """the smallest lnq lies at the matched acceleration on a bin whose period is within one fundamental bin (P0^2 / N
    samples) of P0, and every acceleration two or more steps away lies at least 5 above it (the margin of DESIGN.md 4.22)
    -> (the period, the smallest lnq of every acceleration)"""
    idx = np.unravel_index(np.argmin(lnq), lnq.shape)
    period = samples(SCENE_LOG2N, idx[1], int(at[idx]))
    per_accel = lnq.reshape(lnq.shape[0], -1).min(axis=1)
    assert idx[0] == SCENE_MATCH, (idx, per_accel)
    assert abs(period - SCENE_P0) <= SCENE_P0 * SCENE_P0 / (1 << SCENE_LOG2N), period
    for a in range(lnq.shape[0]):
        if abs(a - SCENE_MATCH) >= 2:
            assert per_accel[a] >= per_accel[SCENE_MATCH] + 5.0, (a, per_accel)
    return period, per_accel


def test_the_scene(built, engine):
    """dedisp -> accel_search -> accel_resample of the winner -> fold on the device with no copy in between, over the
    scene of DESIGN.md 4.24: 60 000 samples at log2n 16, levels 5, norm 64, seg 256, klo 8, eight accelerations ten
    samples of mid-frame shift apart, the pulses along the map of a = 6.

    The conditions are fixed on the CPU beforehand with the restatements (dedisp_ref, accel_ref.search, fold_ref): the
    smallest lnq lies at a = 6 on a bin within one fundamental bin of 137.3 samples, every acceleration two or more
    steps away lies at least 5 above it, and folding the matched resampled series at that period into 16 bins gives a
    larger chi2 than folding the source.  Then the device: the same winner and period, and the CPU's profiles and hits to the bit
    (the dedispersed series, the map and the folding are bit-defined), hence its chi2."""
    log2n, nsamp, nbins = SCENE_LOG2N, SCENE_NSAMP, 16
    levels, norm, seg, klo = SCENE_PLAN
    m = 1 << (log2n - 1)
    nseg = m // seg
    coefs, ninth = scene_coefs(built.accel_coef_from_shift)
    assert coefs == scene_coefs(accel_ref.coef_from_shift)[0] and coefs[2] == 0
    # the ninth coefficient of the scene as first worded is beyond the limit: refused, and the scene does without it
    assert ninth > TOP >= max(coefs) and built.accel_supported(log2n, *SCENE_PLAN, coefs + [ninth]) == 0
    assert "every coefficient must be" in built.accel_last_error() and built.accel_supported(log2n, *SCENE_PLAN, coefs) == 1
    rows = scene_rows(coefs)
    # the restatements' chain meets the conditions by itself
    series = dedisp_ref.dedisp_ref(rows, SCENE_DELAYS, None, nsamp)
    assert abs(series.mean() - 4.0) < 0.05 and abs(series.std() - 1.0) < 0.05
    _, _, ref_best, ref_at = accel_ref.search(series, coefs, log2n, levels, norm, seg, klo)
    ref_period, ref_low = scene_conditions(scene_lnq(ref_best[0], ref_at[0], period_ref.lnq), ref_at[0], periodlong_ref.samples)
    matched = accel_ref.resample(series, coefs[SCENE_MATCH:SCENE_MATCH + 1])[:, 0]
    both = np.concatenate([matched, series])
    ref_prof, ref_hits = fold_ref.fold_ref(both, [fold_ref.step_of(ref_period)], [0], nbins, 65536, nsamp)
    x64 = both.astype(np.float64)
    ref_chi = [fold_ref.chi2(ref_prof[t, 0, 0], ref_hits[0, 0], x64[t].sum(), (x64[t] * x64[t]).sum(), nsamp) for t in range(2)]
    assert ref_chi[0] > ref_chi[1], ref_chi
    print("CPU: smallest lnq per acceleration %s; period %.3f; chi2 %.1f matched, %.1f source"
          % (" ".join("%.1f" % v for v in ref_low), ref_period, ref_chi[0], ref_chi[1]))

    stride = _ceil4(nsamp) + 4
    dd, acc = built.DedispPlan(engine, SCENE_DELAYS), built.AccelPlan(engine, log2n, levels, norm, seg, klo, coefs, max_trials=len(coefs))
    nv = len(coefs)
    bufs = [engine.upload(rows), engine.upload(np.full((2, stride), np.nan, np.float32)), engine.alloc(nv * levels * nseg * 4),
            engine.alloc(nv * levels * nseg * 4), engine.alloc(2 * nbins * 4), engine.alloc(nbins * 4)]
    ff = None
    try:
        # row 1 of the series' buffer is the source, row 0 takes the winner's resampled series
        d_source = bufs[1].ptr + stride * 4
        dd.run(bufs[0], nsamp, d_source, in_stride=SCENE_NCHAN, out_stride=stride)
        acc.search(d_source, stride, 1, nsamp, bufs[2], bufs[3])
        engine.sync()
        best = engine.download(bufs[2], np.float32, (nv, levels, nseg))
        at = engine.download(bufs[3], np.int32, (nv, levels, nseg))
        period, low = scene_conditions(scene_lnq(best, at, built.period_lnq), at, built.periodlong_samples)
        winner = int(np.argmin(low))
        acc.resample(d_source, stride, 1, nsamp, winner, 1, bufs[1], stride)
        step = built.fold_step(period)
        ff = built.FoldPlan(engine, [step], [0], nbins, 65536)
        ff.run(bufs[1], stride, 2, nsamp, bufs[4], bufs[5])
        engine.sync()
        dev_series = engine.download(bufs[1], np.float32, (2, stride))
        prof = engine.download(bufs[4], np.float32, (2, 1, 1, nbins))
        hits = engine.download(bufs[5], np.uint32, (1, 1, nbins))
    finally:
        for plan in (dd, acc, ff):
            if plan is not None:
                plan.close()
        for b in bufs:
            b.free()
    _same_bits(dev_series[:, :nsamp], both, "the source and the winner's series")
    assert np.isnan(dev_series[:, nsamp:]).all()
    assert winner == SCENE_MATCH and period == ref_period and step == fold_ref.step_of(period)
    _same_bits(prof, ref_prof, "prof")
    assert np.array_equal(hits, ref_hits)
    dev64 = dev_series[:, :nsamp].astype(np.float64)
    chi = [built.fold_chi2(prof[t, 0, 0], hits[0, 0], dev64[t].sum(), (dev64[t] * dev64[t]).sum(), nsamp) for t in range(2)]
    assert chi[0] > chi[1] and all(abs(c - r) <= 1e-12 * r for c, r in zip(chi, ref_chi)), (chi, ref_chi)
    print("device: smallest lnq per acceleration %s; period %.3f; chi2 %.1f matched, %.1f source"
          % (" ".join("%.1f" % v for v in low), period, chi[0], chi[1]))

"""GPU suite of include/rtlws_ffa.h (librtlws_ffa.so) against its numpy restatement (tests/ffa_ref.py): peaks and profiles
on uint32 views with NaN by place, places exactly; NaN in the stride's padding and behind samples_needed, a preset
pattern and a guard behind every output; signed data with exponents over 2^-6 .. 2^6.  Every stage at every lane border,
every pass count the plan makes, the width tables and planted peaks, the segments on both sides of the merge, the trial
counts past the pairs in flight, a NULL d_prof and a wider prof_stride, one plan many times and beside another, graph
capture, every refusal of a run, the chain dedispersion -> fast folding on the device, and a train found at its period."""
import numpy as np
import pytest

import dedisp_ref
import ffa_ref
import pulse_ref

pytestmark = pytest.mark.gpu

FILL = np.float32(-12345.678)
LANE_BORDERS = (16, 17, 63, 64, 65, 255, 256, 257, 1023, 1024)
LADDER16 = (1, 2, 3, 4, 6, 8, 12, 16, 24, 32, 48, 64, 96, 128, 255, 256)


@pytest.fixture(scope="module")
def ffa(built):
    import rtlws.ffa
    return rtlws.ffa


def _same_bits(got, want, what=None):
    """bit for bit on uint32 views, NaN by place (the default NaN of the host's additions and the device's may differ)"""
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape)
    nan = np.isnan(want) if got.dtype.kind == "f" else np.zeros(want.shape, bool)
    gnan = np.isnan(got) if got.dtype.kind == "f" else nan
    bad = (gnan != nan) | (~nan & (got.view(np.uint32) != want.view(np.uint32)))
    assert not bad.any(), (what, np.argwhere(bad)[:5], got[bad][:5], want[bad][:5])


_REFERENCES = {}


def _reference(key, x, p0, nper, L, widths, seg):
    """ffa_ref of a named input, computed once and shared"""
    if key is None:
        return ffa_ref.ffa_ref(x, p0, nper, L, widths, seg)
    full = (key, p0, nper, L, tuple(widths), seg)
    if full not in _REFERENCES:
        _REFERENCES[full] = ffa_ref.ffa_ref(x, p0, nper, L, widths, seg)
    return _REFERENCES[full]


def _padded(x, need):
    """x [ntrials, >= need] in rows of a stride four beyond the next multiple of 4, NaN in the padding and behind need"""
    stride = (need + 3) // 4 * 4 + 4
    padded = np.full((x.shape[0], stride), np.nan, np.float32)
    padded[:, :need] = x[:, :need]
    return padded, stride


def _check(got, want, p0, nper, L, widths, seg, ntrials, want_prof, name):
    """the three flat buffers of search(fill=FILL) against the restatement: the guards, the outputs, the profiles'
    columns of every base period, and FILL in the columns behind them (or everywhere without want_prof)"""
    peak, at, prof = got
    m, p_max, nseg, nw = 1 << L, p0 + nper - 1, (1 << L) // seg, len(widths)
    n1, n2 = ntrials * nper * nseg * nw, ntrials * nper * m * p_max
    assert peak.shape == at.shape == (n1 + 8,) and prof.shape == (n2 + 8,) and at.dtype == np.int32, name
    assert np.all(peak[n1:].view(np.uint32) == FILL.view(np.uint32)) and np.all(at[n1:] == FILL.view(np.int32)), name
    assert np.all(prof[n2:].view(np.uint32) == FILL.view(np.uint32)), name
    _same_bits(peak[:n1].reshape(want[0].shape), want[0], (name, "peak"))
    assert np.array_equal(at[:n1].reshape(want[1].shape), want[1]), (name, "at", np.argwhere(at[:n1].reshape(want[1].shape) != want[1])[:5])
    prof = prof[:n2].reshape(ntrials, nper, m, p_max)
    if not want_prof:
        assert np.all(prof.view(np.uint32) == FILL.view(np.uint32)), name
        return
    for i in range(nper):
        _same_bits(prof[:, i, :, :p0 + i], want[2][i], (name, "prof", i))
        assert np.all(prof[:, i, :, p0 + i:].view(np.uint32) == FILL.view(np.uint32)), (name, "behind p_i", i)


def _run(ffa, engine, x, p0, nper, L, widths, seg, want_prof=True, name=None, key=None):
    """x float32 [ntrials, >= samples_needed] through rtlws.ffa.search with NaN in the padding and behind samples_needed
    and preset guards behind the outputs, against the restatement -> (peak, at) of the device in their shapes"""
    need = ffa_ref.samples_needed(p0, nper, L)
    padded, stride = _padded(x, need)
    got = ffa.search(engine, padded, p0, nper, L, widths, seg, in_stride=stride, want_prof=want_prof, fill=FILL)
    want = _reference(key, x, p0, nper, L, widths, seg)
    _check(got, want, p0, nper, L, widths, seg, x.shape[0], want_prof, name)
    n1 = want[0].size
    return got[0][:n1].reshape(want[0].shape), got[1][:n1].reshape(want[1].shape)


# ---- every stage at every lane border ------------------------------------------------------------------------------

@pytest.mark.parametrize("p0", LANE_BORDERS)
def test_every_stage_at_every_lane_border(ffa, engine, p0):
    """L = 1 .. 5 at a column count on each side of every multiple of the 64 lanes that matters and at both limits: a row
    of one partial chunk, of whole chunks, of whole chunks and one column"""
    for L in range(1, 6):
        x = ffa_ref.signed_series(2, p0 << L, seed=100 * L + p0)
        widths = (1, 3, min(p0, 16))
        _run(ffa, engine, x, p0, 1, L, widths, 1 << (L // 2), name=(p0, L))


@pytest.mark.parametrize("p0", [63, 1022])
def test_three_base_periods_across_a_border(ffa, engine, p0):
    """nper = 3 across 63 .. 65 and 1022 .. 1024: the pitch of the tile is the last one's, the rows in memory each pair's own"""
    for L in (1, 3, 4):
        x = ffa_ref.signed_series(2, (p0 + 2) << L, seed=7 * L + p0)
        _run(ffa, engine, x, p0, 3, L, (1, 2, 5), 2, name=(p0, L))


# ---- every pass count ------------------------------------------------------------------------------------------------

def _pass_cases(ffa):
    """at p_max = 1024: the smallest L of two passes, the smallest of three, and one whose last pass has a single stage"""
    plans = {L: ffa.geometry(1024, 1, L, (1, 4), 1) for L in range(1, 10)}
    assert all(g[0] == 0 for g in plans.values())
    two = min(L for L, g in plans.items() if g[1] == 2)
    three = min(L for L, g in plans.items() if g[1] == 3)
    single = min(L for L, g in plans.items() if g[2][g[1] - 1] == 1)
    return plans, (single, two, three)


def test_the_cases_cover_every_pass_count(ffa):
    plans, cases = _pass_cases(ffa)
    assert {plans[L][1] for L in cases} == {1, 2, 3}
    assert all(sum(plans[L][2]) == L for L in cases) and all((1024 << L) <= 1 << 21 for L in cases)
    assert plans[cases[0]][2][plans[cases[0]][1] - 1] == 1
    assert all(max(g[5]) <= 160 * 1024 for g in plans.values())
    assert max(max(g[5]) for g in plans.values()) > 64 * 1024              # a tile above the LDS a kernel gets unasked


@pytest.mark.parametrize("which", [0, 1, 2])
def test_every_pass_count(ffa, engine, which):
    plans, cases = _pass_cases(ffa)
    L = cases[which]
    x = ffa_ref.signed_series(2, 1024 << L, seed=40 + L)
    for seg in (1, 1 << L):
        _run(ffa, engine, x, 1024, 1, L, (1, 4), seg, name=(L, seg), key=("passes", L))
    # the same stages at a pitch whose tile is larger split otherwise, and give the same kind of bits
    if which == 2:
        assert ffa.geometry(100, 1, L, (1, 4), 1)[1] == 2
        _run(ffa, engine, ffa_ref.signed_series(2, 100 << L, seed=41), 100, 1, L, (1, 4), 4, name=("pitch 100", L))


# ---- widths and peaks ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("widths", [(1,), "p0", (1, 2, 3, 5, 8, 13), LADDER16], ids=["one", "p0", "fibonacci", "ladder16"])
def test_width_tables(ffa, engine, widths):
    p0 = 300 if widths == LADDER16 else 70
    widths = (p0,) if widths == "p0" else widths
    x = ffa_ref.signed_series(2, (p0 + 1) << 4, seed=len(widths))
    _run(ffa, engine, x, p0, 2, 4, widths, 4, name=widths)


def test_a_pulse_across_the_last_column(ffa, engine):
    """a pulse of three columns planted at columns p - 1, 0, 1 of every row of a series of period p: width 3 finds it at
    column p - 1, where the sum wraps, in the row of shift 0"""
    p, L = 67, 4
    m = 1 << L
    x = (ffa_ref.signed_series(1, p * m, seed=77) * np.float32(2.0 ** -10)).reshape(m, p)
    for c in (p - 1, 0, 1):
        x[:, c] += 100.0
    peak, at = _run(ffa, engine, x.reshape(1, -1), p, 1, L, (1, 3), m, name="wrap")
    assert at[0, 0, 0, 1] == p - 1 and peak[0, 0, 0, 1] > 3 * 100.0 * m * 0.99
    want = ffa_ref.ffa_ref(x.reshape(1, -1), p, 1, L, (3,), 1)
    assert want[1][0, 0, 0, 0] == p - 1                          # row 0 is the plain fold: the planted columns line up


def test_constants_nan_zeros_subnormals_and_infinities(ffa, engine):
    p0, L, seg = 33, 4, 4
    need = ffa_ref.samples_needed(p0, 2, L)
    x = ffa_ref.signed_series(8, need, seed=90)
    x[0, :] = np.float32(1.5)                                   # every sum of a row is the same: the segment's first index wins
    x[1, :] = np.nan                                            # nothing above -Inf: (-Inf, -1)
    x[2, :] = -0.0
    x[3, 1::2] = 0.0
    x[3, 0::2] = -0.0
    x[4, :] = np.float32(2.0 ** -149) * (1 + np.arange(need) % 7).astype(np.float32)      # subnormals only: the sums stay exact
    x[5, :] = x[5] * np.float32(2.0 ** -130)                    # subnormals among small normals
    x[6, 100], x[6, 301], x[6, 500] = np.inf, -np.inf, np.nan
    x[7, :] = -np.inf
    peak, at = _run(ffa, engine, x, p0, 2, L, (1, 2, 7), seg, name="special values")
    for i, p in enumerate((p0, p0 + 1)):
        assert np.array_equal(at[0, i], np.repeat((np.arange(4) * seg * p)[:, None], 3, axis=1))
        assert np.array_equal(at[2, i], at[0, i]) and np.array_equal(at[3, i][:, 0], at[0, i][:, 0])
    assert np.all(peak[0, 0] == np.float32(1.5) * 16 * np.array([1, 2, 7], np.float32))
    assert np.all(at[1] == -1) and np.all(peak[1] == -np.inf) and np.all(at[7] == -1) and np.all(peak[7] == -np.inf)
    assert np.all(peak[4] > 0) and np.all(peak[4] < 2.0 ** -126)
    assert np.isinf(peak[6]).any() and not np.isnan(peak).any()


# ---- segments ----------------------------------------------------------------------------------------------------

def test_segments_on_both_sides_of_the_merge(ffa, engine):
    """seg = 1, seg = m, and every power of two between, at a plan of two passes, whose last workgroups hold 8 rows (a seg
    above them takes the merge launch), and at a plan of one pass, whose evaluating wavefronts hold several rows each"""
    for p0, L, two_passes in ((700, 6, True), (150, 6, False)):
        widths = (1, 2, 9)
        rc, passes, stages, _, _, _, merge, _, _ = ffa.geometry(p0, 1, L, widths, 1)
        last = stages[passes - 1]
        assert rc == 0 and merge == 0 and (passes == 2 and 1 < (1 << last) < (1 << L) if two_passes else passes == 1)
        x = ffa_ref.signed_series(2, p0 << L, seed=61)
        x[0, :] = np.float32(0.25)                              # ties everywhere: the least index of every segment
        merged = set()
        for seg_log2 in range(L + 1):
            merged.add(ffa.geometry(p0, 1, L, widths, 1 << seg_log2)[6])
            peak, at = _run(ffa, engine, x, p0, 1, L, widths, 1 << seg_log2, want_prof=False, name=(p0, "seg", 1 << seg_log2), key=("segments", p0))
            assert np.array_equal(at[0, 0, :, 0], np.arange((1 << L) >> seg_log2) * (p0 << seg_log2))
        assert merged == ({0, 1} if two_passes else {0})
        if two_passes:
            assert ffa.geometry(p0, 1, L, widths, 2 << last)[6] == 1 and ffa.geometry(p0, 1, L, widths, 1 << last)[6] == 0


# ---- the remaining run cases -------------------------------------------------------------------------------------------

def _on_device(torch, host):
    return torch.from_numpy(np.ascontiguousarray(host)).to(torch.device("cuda", 0))


def _outputs(torch, npeaks, nprof):
    return (_on_device(torch, np.full(npeaks + 8, FILL, np.float32)), _on_device(torch, np.full(npeaks + 8, 0x5EADBEEF, np.int32)),
            _on_device(torch, np.full(nprof + 8, FILL, np.float32)))


def _check_outputs(outs, want, nper, p0, prof_stride, what=None, with_prof=True):
    peak, at, prof = (o.cpu().numpy() for o in outs)
    n1 = want[0].size
    ntrials, m = want[2][0].shape[:2]
    n2 = ntrials * nper * m * prof_stride
    assert np.all(peak[n1:] == FILL) and np.all(at[n1:] == 0x5EADBEEF) and np.all(prof[n2:] == FILL), what
    _same_bits(peak[:n1].reshape(want[0].shape), want[0], (what, "peak"))
    assert np.array_equal(at[:n1].reshape(want[1].shape), want[1]), (what, "at")
    prof = prof[:n2].reshape(ntrials, nper, m, prof_stride)
    if not with_prof:
        assert np.all(prof == FILL), what
        return
    for i in range(nper):
        _same_bits(prof[:, i, :, :p0 + i], want[2][i], (what, "prof", i))
        assert np.all(prof[:, i, :, p0 + i:] == FILL), (what, "behind p_i", i)


@pytest.mark.parametrize("ntrials", [1, 3, "in flight + 1"])
def test_trial_counts(ffa, engine, ntrials):
    """one trial, three, and with a plan opened for two trials (six pairs in flight) a run of one trial more than the pairs
    in flight: four groups through the workspace and the merge, the last of them short"""
    import torch
    p0, nper, L, widths, seg = 40, 2, 5, (1, 6), 8
    rc, passes, _, _, _, _, merge, _, pairs = ffa.geometry(p0, nper, L, widths, seg, max_trials=1)
    assert rc == 0 and pairs == 2 and passes == 1
    if ntrials != "in flight + 1":
        _run(ffa, engine, ffa_ref.signed_series(ntrials, (p0 + 1) << L, seed=ntrials), p0, nper, L, widths, seg, name=ntrials)
        return
    # a plan of two passes and a merge, so that the groups go through the workspace; the last group is short
    p0, nper, L, seg = 700, 3, 6, 64
    rc, passes, stages, _, _, _, merge, ws, pairs = ffa.geometry(p0, nper, L, widths, seg, max_trials=2)
    assert rc == 0 and pairs == 6 and passes == 2 and merge == 1 and ws > 0
    ntrials = pairs + 1
    assert (ntrials * nper) % pairs and ntrials * nper > 3 * pairs
    need = ffa_ref.samples_needed(p0, nper, L)
    host, stride = _padded(ffa_ref.signed_series(ntrials, need, seed=5), need)
    want = ffa_ref.ffa_ref(host, p0, nper, L, widths, seg)
    plan = ffa.FfaPlan(engine, p0, nper, L, widths, seg, max_trials=2)
    assert plan.workspace_bytes() == ws and plan.samples_needed() == need
    p_max = p0 + nper - 1
    outs = _outputs(torch, want[0].size, ntrials * nper * (1 << L) * p_max)
    series = _on_device(torch, host)
    plan.run(series.data_ptr(), stride, ntrials, outs[0].data_ptr(), outs[1].data_ptr(), outs[2].data_ptr(), p_max, stream=ffa_stream(engine))
    torch.cuda.synchronize()
    _check_outputs(outs, want, nper, p0, p_max, "groups")
    plan.close()


def ffa_stream(engine):
    import rtlws
    return rtlws.torch_stream_handle()


def test_prof_options(ffa, engine):
    """d_prof NULL: the same peaks, nothing stored; prof_stride = p_max + 4: the columns behind every p_i untouched"""
    import torch
    p0, nper, L, widths, seg = 61, 3, 4, (1, 2, 4), 2
    need = ffa_ref.samples_needed(p0, nper, L)
    host, stride = _padded(ffa_ref.signed_series(2, need, seed=33), need)
    want = ffa_ref.ffa_ref(host, p0, nper, L, widths, seg)
    series = _on_device(torch, host)
    plan = ffa.FfaPlan(engine, p0, nper, L, widths, seg, max_trials=2)
    prof_stride = p0 + nper - 1 + 4
    for with_prof in (True, False):
        outs = _outputs(torch, want[0].size, 2 * nper * (1 << L) * prof_stride)
        plan.run(series.data_ptr(), stride, 2, outs[0].data_ptr(), outs[1].data_ptr(), outs[2].data_ptr() if with_prof else None,
                 prof_stride, stream=ffa_stream(engine))
        torch.cuda.synchronize()
        _check_outputs(outs, want, nper, p0, prof_stride, with_prof, with_prof)
    plan.close()


def test_one_plan_twice_and_two_plans(ffa, engine):
    """one plan run twice into preset buffers; then beside a second plan of other base periods, L, widths and seg, their
    runs in turn on one stream (a plan's runs share its workspace) and the two plans on two streams"""
    import torch
    import rtlws
    shapes = ((700, 2, 6, (1, 3), 64), (17, 1, 3, (2,), 1))
    hosts, wants, series, plans = [], [], [], []
    for j, (p0, nper, L, widths, seg) in enumerate(shapes):
        need = ffa_ref.samples_needed(p0, nper, L)
        host, stride = _padded(ffa_ref.signed_series(2, need, seed=80 + j), need)
        hosts.append((host, stride))
        wants.append(ffa_ref.ffa_ref(host, p0, nper, L, widths, seg))
        series.append(_on_device(torch, host))
        plans.append(ffa.FfaPlan(engine, p0, nper, L, widths, seg, max_trials=2))
    assert ffa.geometry(*shapes[0], max_trials=2)[1] == 2 and ffa.geometry(*shapes[0], max_trials=2)[6] == 1
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    for s in streams:
        s.wait_stream(torch.cuda.current_stream())
    reps = 2
    outs = [[_outputs(torch, wants[j][0].size, 2 * sh[1] * (1 << sh[2]) * (sh[0] + sh[1] - 1)) for _ in range(reps)] for j, sh in enumerate(shapes)]
    for rep in range(reps):
        for j, sh in enumerate(shapes):
            o = outs[j][rep]
            plans[j].run(series[j].data_ptr(), hosts[j][1], 2, o[0].data_ptr(), o[1].data_ptr(), o[2].data_ptr(), sh[0] + sh[1] - 1,
                         stream=rtlws.torch_stream_handle(streams[j]))
    torch.cuda.synchronize()
    for j, sh in enumerate(shapes):
        for rep in range(reps):
            _check_outputs(outs[j][rep], wants[j], sh[1], sh[0], sh[0] + sh[1] - 1, (j, rep))
    for plan in plans:
        plan.close()


def test_capture_and_replay(built, ffa):
    """tests/test_graph_gpu.py's pattern for this plan: rtlws_ffa_run of two passes and a merge captured on a side stream
    enqueues nothing, replays give the eager launches' bits and the restatement's, twice"""
    import torch
    eng = built.Engine(0)
    p0, nper, L, widths, seg = 650, 2, 5, (1, 5), 32
    g0 = ffa.geometry(p0, nper, L, widths, seg, max_trials=1)
    assert g0[1] == 2 and g0[6] == 1 and g0[8] == 2             # two passes, a merge, and two groups for two trials
    need = ffa_ref.samples_needed(p0, nper, L)
    host, stride = _padded(ffa_ref.signed_series(2, need, seed=72), need)
    want = ffa_ref.ffa_ref(host, p0, nper, L, widths, seg)
    series = _on_device(torch, host)
    plan = ffa.FfaPlan(eng, p0, nper, L, widths, seg, max_trials=1)
    nprof = 2 * nper * (1 << L) * (p0 + 1)
    outs = _outputs(torch, want[0].size, nprof)
    before = [o.clone() for o in outs]
    g = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        with torch.cuda.graph(g, stream=side):
            plan.run(series.data_ptr(), stride, 2, outs[0].data_ptr(), outs[1].data_ptr(), outs[2].data_ptr(), p0 + 1, stream=built.torch_stream_handle())
    torch.cuda.current_stream().wait_stream(side)
    assert all(torch.equal(o, b) for o, b in zip(outs, before))              # capture enqueued nothing
    for _ in range(2):
        for o, b in zip(outs, before):
            o.copy_(b)
        g.replay()
        torch.cuda.synchronize()
        _check_outputs(outs, want, nper, p0, p0 + 1, "replay")
    eager = _outputs(torch, want[0].size, nprof)
    plan.run(series.data_ptr(), stride, 2, eager[0].data_ptr(), eager[1].data_ptr(), eager[2].data_ptr(), p0 + 1, stream=built.torch_stream_handle())
    torch.cuda.synchronize()
    assert all(torch.equal(e.view(torch.int32), o.view(torch.int32)) for e, o in zip(eager, outs))
    plan.close()
    eng.close()


def test_every_refusal_of_a_run(ffa, engine):
    """in the header's order, each with the one before it mended; nothing is launched: the outputs keep their preset"""
    import torch
    p0, nper, L, widths, seg = 20, 2, 3, (1, 2), 2
    need = ffa_ref.samples_needed(p0, nper, L)
    series = _on_device(torch, np.zeros((2, need + 8), np.float32))
    outs = _outputs(torch, 2 * nper * 4 * 2, 2 * nper * 8 * (p0 + 1))
    plan = ffa.FfaPlan(engine, p0, nper, L, widths, seg, max_trials=2)
    d_in, d_peak, d_at, d_prof = series.data_ptr(), outs[0].data_ptr(), outs[1].data_ptr(), outs[2].data_ptr()
    good = dict(d_in=d_in, in_stride=need + 8, ntrials=2, d_peak=d_peak, d_at=d_at, d_prof=d_prof, prof_stride=p0 + 1)
    refusals = [(dict(ntrials=0), "ntrials must be 1 .. 65536"), (dict(ntrials=65537), "ntrials must be 1 .. 65536"),
                (dict(in_stride=need + 6), "in_stride must be a multiple of 4"),
                (dict(d_in=None), "null pointer"), (dict(d_peak=None), "null pointer"), (dict(d_at=None), "null pointer"),
                (dict(d_in=d_in + 4), "d_in must be 16-byte aligned"), (dict(d_peak=d_peak + 2), "d_peak must be 4-byte aligned"),
                (dict(d_at=d_at + 1), "d_at must be 4-byte aligned"), (dict(d_prof=d_prof + 2), "d_prof must be 4-byte aligned"),
                (dict(in_stride=need - 4), "in_stride must be >= samples_needed"), (dict(prof_stride=p0), "prof_stride must be >= p0 + nper - 1")]
    for k, (change, text) in enumerate(refusals):
        args = dict(good)
        args.update(change)
        # everything later in the order is broken too: the earlier refusal is the one reported
        for later, _ in refusals[k + 1:]:
            if not set(later) & set(change) and list(later) != ["ntrials"]:
                args.update(later)
        rc = plan.run(**args, stream=ffa_stream(engine), check=False)
        assert rc == -1 and ffa.last_error() == "rtlws_ffa_run: " + text, (change, ffa.last_error())
    # a null plan comes behind the arguments that need none and before the plan's own rules
    L_ = ffa.lib()
    assert L_.rtlws_ffa_run(None, d_in, need - 4, 2, d_peak, d_at, d_prof, p0, None) == -1 and "null plan" in ffa.last_error()
    assert L_.rtlws_ffa_run(None, d_in + 4, need - 4, 2, d_peak, d_at, d_prof, p0, None) == -1 and "d_in must be" in ffa.last_error()
    # prof_stride is not looked at without a d_prof
    assert plan.run(d_in, need + 8, 2, d_peak, d_at, None, 0, stream=ffa_stream(engine)) == 0
    torch.cuda.synchronize()
    assert np.all(outs[2].cpu().numpy() == FILL) and not np.any(outs[0].cpu().numpy()[:32] == FILL)
    plan.close()


def test_dedispersion_into_the_search_on_the_device(built, ffa, engine):
    """rtlws_dedisp_run's series searched where they lie: rows -> dedisp -> ffa with no host copy in between; the peaks and
    profiles bit for bit the restatements' chain over the same rows"""
    p0, nper, L, widths, seg = 16, 3, 4, (1, 2, 4), 4
    nsamp = ffa_ref.samples_needed(p0, nper, L)
    delays = dedisp_ref.delays(*dedisp_ref.DELAY_SETS[1])
    ntrials, nchan = delays.shape
    nrows = dedisp_ref.rows_needed(delays, None, nsamp)
    rows = dedisp_ref.signed_rows(nrows, nchan, seed=17)
    stride = nsamp + 4
    m, p_max, nseg = 1 << L, p0 + nper - 1, (1 << L) // seg
    npeaks, nprof = ntrials * nper * nseg * len(widths), ntrials * nper * m * p_max
    dd, ff = built.DedispPlan(engine, delays), ffa.FfaPlan(engine, p0, nper, L, widths, seg, max_trials=ntrials)
    bufs = [engine.upload(rows), engine.upload(np.full((ntrials, stride), np.nan, np.float32)), engine.alloc(npeaks * 4),
            engine.alloc(npeaks * 4), engine.upload(np.full(nprof, FILL, np.float32))]
    try:
        dd.run(bufs[0], nsamp, bufs[1], in_stride=nchan, out_stride=stride)
        ff.run(bufs[1], stride, ntrials, bufs[2], bufs[3], bufs[4], p_max)
        engine.sync()
        peak = engine.download(bufs[2], np.float32, (ntrials, nper, nseg, len(widths)))
        at = engine.download(bufs[3], np.int32, (ntrials, nper, nseg, len(widths)))
        prof = engine.download(bufs[4], np.float32, (ntrials, nper, m, p_max))
    finally:
        dd.close()
        ff.close()
        for b in bufs:
            b.free()
    series = dedisp_ref.dedisp_ref(rows, delays, None, nsamp)
    want = ffa_ref.ffa_ref(series, p0, nper, L, widths, seg)
    _same_bits(peak, want[0], "peak")
    assert np.array_equal(at, want[1])
    for i in range(nper):
        _same_bits(prof[:, i, :, :p0 + i], want[2][i], ("prof", i))


# ---- meaning -----------------------------------------------------------------------------------------------------

def test_a_train_is_found_at_its_period(built, ffa, engine):
    """Unit noise plus a train of period p + s0 / (m - 1) samples, p = 250, L = 7, s0 = 77, 4 sigma a pulse: first, on the
    restatement alone, the largest peak of width 1 lies within one row of s0; then the device's peaks are the
    restatement's, and rtlws_ffa_snr with the pulse search's moments of the series is finite and largest there"""
    p, L, s0, widths = 250, 7, 77, (1, 2, 4)
    m = 1 << L
    need = p << L
    x = ffa_ref.train(need, p + s0 / (m - 1), 4.0, seed=5)[None, :]
    want = ffa_ref.ffa_ref(x, p, 1, L, widths, 1)
    assert abs(int(np.argmax(want[0][0, 0, :, 0])) - s0) <= 1
    peak, at = _run(ffa, engine, x, p, 1, L, widths, 1, want_prof=False, name="train")
    _, _, mom = engine.pulse(x, (1,), 1024)
    assert np.array_equal(mom.view(np.uint64), pulse_ref.moments(x, 1024, need).view(np.uint64))
    sum1, sum2 = mom[0, :, 0].sum(), mom[0, :, 1].sum()
    snr = np.array([[ffa.snr(peak[0, 0, s, k], w, m, sum1, sum2, need) for k, w in enumerate(widths)] for s in range(m)])
    assert np.all(np.isfinite(snr))
    row, k = np.unravel_index(np.argmax(snr), snr.shape)
    assert abs(int(row) - s0) <= 1 and k == 0 and snr[row, k] > 8.0
    assert abs(ffa.period(p, int(row), L) - (p + s0 / (m - 1))) <= 1.0 / (m - 1)
    print("the train of period %.4f: snr %.1f at period %.4f (row %d, width 1); the largest elsewhere %.1f"
          % (p + s0 / (m - 1), snr[row, k], ffa.period(p, int(row), L), row, np.sort(snr[:, 0])[-2]))

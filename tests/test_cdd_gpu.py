"""GPU suite of include/rtlws_cdd.h (librtlws_cdd.so) against its restatement (tests/cdd_ref.py): the voltages of every
N held to both derived bounds with NaN in the input's padding and a preset pattern around every
output; single impulses, where the per-sample bound bites and a misplaced bin or a wrong digit of the inverse cannot
pass; the power rows in both layouts, bit for bit the f32 restatement over the same plan shape's voltages and within
the squared bound of the f64 reference, and through rtlws_dedisp_run; segments run alone against the whole run's bits;
graph capture; the refusals a plan decides.  Every test prints the worst share of each allowance it holds."""
import numpy as np
import pytest

import cdd_ref

pytestmark = pytest.mark.gpu

FILL = np.float32(-12345.678)


@pytest.fixture(scope="module")
def cdd(built):
    import rtlws.cdd
    return rtlws.cdd


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32)


def _tables(cdd, log2n, nchan, seed, chirp_at=None):
    """random unit phases per channel; channel chirp_at the chirp of a 1 MHz channel at 400 MHz whose overlap (4, 4) lies
    inside the suite's (lead, trail) = (5, 11)"""
    rng = np.random.default_rng(seed)
    t = np.exp(2j * np.pi * rng.random((nchan, 1 << log2n))).astype(np.complex64)
    if chirp_at is not None:
        assert max(cdd.overlap(400.0, 1.0, 0.05)) <= 5
        t[chirp_at] = cdd.chirp(log2n, 400.0, 1.0, 0.05)
    return t


def _gauss(nchan, n, seed):
    rng = np.random.default_rng(seed)
    return (rng.standard_normal((nchan, n)) + 1j * rng.standard_normal((nchan, n))).astype(np.complex64)


def _padded(x, need):
    """x [nchan, >= need] in rows of an odd stride three beyond need (channel 1 then starts 8-byte aligned and no more),
    NaN in the padding"""
    stride = need + 3 + (need % 2 == 1)
    assert stride % 2 == 1
    padded = np.full((x.shape[0], stride), np.nan + 1j * np.nan, np.complex64)
    padded[:, :need] = x[:, :need]
    return padded, stride


def _volts(cdd, engine, x, tables, lead, trail, nseg):
    """the voltages through dedisperse(fill=FILL) with NaN behind the samples a run reads and an odd out_stride three
    beyond the outputs: the preset around the outputs checked -> complex64 [nchan, nseg hop]"""
    nchan, n = tables.shape
    per = nseg * (n - lead - trail)
    padded, stride = _padded(x, cdd_ref.samples_needed(n, lead, trail, nseg))
    flat = cdd.dedisperse(engine, padded, tables, lead, trail, nseg=nseg, in_stride=stride, out_stride=per + 3, fill=FILL)
    assert flat.dtype == np.complex64 and flat.shape == (nchan * (per + 3) + cdd.GUARD,)
    body = flat[:nchan * (per + 3)].reshape(nchan, per + 3)
    assert np.all(_bits(body[:, per:]) == _bits(FILL)) and np.all(_bits(flat[nchan * (per + 3):]) == _bits(FILL)), "written outside the outputs"
    return np.ascontiguousarray(body[:, :per])


# ---- voltages at every N --------------------------------------------------------------------------------------------

@pytest.mark.parametrize("log2n", range(9, 15))
def test_voltages_within_both_bounds(cdd, engine, log2n):
    n, nchan, nseg, lead, trail = 1 << log2n, 3, 3, 5, 11
    tables = _tables(cdd, log2n, nchan, seed=log2n, chirp_at=1)
    x = _gauss(nchan, cdd_ref.samples_needed(n, lead, trail, nseg), seed=100 + log2n)
    got = _volts(cdd, engine, x, tables, lead, trail, nseg)
    per_sample, per_segment = cdd_ref.shares(got, x, tables, lead, trail, nseg)
    print("cdd voltages log2n %d: worst share of the per-sample allowance %.3g, of the per-segment allowance %.3g" % (log2n, per_sample, per_segment))
    assert per_sample <= 1.0 and per_segment <= 1.0


# ---- single impulses ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("log2n", [9, 12, 14])
def test_impulses_bite_the_per_sample_bound(cdd, engine, log2n):
    """one impulse a segment (||x_s||_1 = 1), segments that do not overlap so that it stays one, a random-phase table:
    every one of the N outputs of every segment within B1 mean|H| of the f64 value, some 1e-5 against outputs of
    magnitude N^-1/2"""
    n = 1 << log2n
    places = [m for m in (0, 1, 15, 16, 255, 256, 4095, n - 1) if m < n]
    places = sorted(set(places))
    nseg = len(places)
    tables = _tables(cdd, log2n, 2, seed=40 + log2n)
    x = np.zeros((2, nseg * n), np.complex64)
    for s, m in enumerate(places):
        x[0, s * n + m] = 1.0
        x[1, s * n + m] = np.complex64(0.6 - 0.8j)
    assert np.all(np.abs(np.abs(x.astype(np.complex128)).reshape(2, nseg, n).sum(axis=2) - 1.0) < 1e-7)
    got = _volts(cdd, engine, x, tables, 0, 0, nseg)
    per_sample, per_segment = cdd_ref.shares(got, x, tables, 0, 0, nseg)
    print("cdd impulses log2n %d: worst share of the per-sample allowance %.3g, of the per-segment allowance %.3g" % (log2n, per_sample, per_segment))
    assert per_sample <= 1.0 and per_segment <= 1.0
    # the same impulses inside overlapping segments: lead and trail cut the outputs where the header says
    lead, trail = 5, 11
    nseg2 = 2
    x2 = x[:, :cdd_ref.samples_needed(n, lead, trail, nseg2)]
    got2 = _volts(cdd, engine, x2, tables, lead, trail, nseg2)
    s1, s2 = cdd_ref.shares(got2, x2, tables, lead, trail, nseg2)
    print("cdd impulses log2n %d, lead 5, trail 11: %.3g, %.3g" % (log2n, s1, s2))
    assert s1 <= 1.0 and s2 <= 1.0


# ---- power rows ----------------------------------------------------------------------------------------------------

_POWER_INPUTS = {}


def _power_inputs(cdd, engine, log2n):
    """per N: (lead, trail) with hop divisible by 3, the tables, the input, and the run's own ksum == 0 voltages, once"""
    if log2n not in _POWER_INPUTS:
        n, nchan, nseg = 1 << log2n, 4, 2
        lead, trail = (5, 12) if log2n % 2 else (5, 11)        # 2^log2n is 2 (mod 3) at an odd log2n, 1 at an even one
        assert (n - lead - trail) % 3 == 0
        tables = _tables(cdd, log2n, nchan, seed=60 + log2n)
        x = _gauss(nchan, cdd_ref.samples_needed(n, lead, trail, nseg), seed=160 + log2n)
        volts = _volts(cdd, engine, x, tables, lead, trail, nseg)
        volts.setflags(write=False)
        _POWER_INPUTS[log2n] = (lead, trail, nseg, tables, x, volts)
    return _POWER_INPUTS[log2n]


def _power(cdd, engine, log2n, which, layout):
    """the power rows of _power_inputs' run at ksum `which` ("hop": one row a segment) in one layout, with NaN in the
    input's padding and a preset pattern around the rows: bit for bit the f32 restatement over the run's own voltages,
    and within the row allowance of the f64 reference"""
    lead, trail, nseg, tables, x, volts = _power_inputs(cdd, engine, log2n)
    nchan, n = tables.shape
    hop = n - lead - trail
    ksum = hop if which == "hop" else int(which)
    rows = nseg * hop // ksum
    padded, stride = _padded(x, cdd_ref.samples_needed(n, lead, trail, nseg))
    least, count = (nchan, rows) if layout == "time" else (rows, nchan)
    out_stride = least + 4
    flat = cdd.dedisperse(engine, padded, tables, lead, trail, ksum=ksum, layout=layout, nseg=nseg, in_stride=stride, out_stride=out_stride, fill=FILL)
    assert flat.dtype == np.float32 and flat.shape == (count * out_stride + cdd.GUARD,)
    body = flat[:count * out_stride].reshape(count, out_stride)
    assert np.all(_bits(body[:, least:]) == _bits(FILL)) and np.all(_bits(flat[count * out_stride:]) == _bits(FILL)), "written outside the rows"
    got = np.ascontiguousarray(body[:, :least].T if layout == "time" else body[:, :least])          # [nchan, rows]
    want = cdd_ref.power_rows(volts, ksum)
    assert np.array_equal(_bits(got), _bits(want)), np.argwhere(_bits(got) != _bits(want))[:5]
    ref, allowance = cdd_ref.power_allowance(x, tables, lead, trail, nseg, ksum)
    share = float((np.abs(got.astype(np.float64) - ref) / allowance).max())
    print("cdd power log2n %d ksum %d %s-major: worst share of the row allowance %.3g" % (log2n, ksum, layout, share))
    assert share <= 1.0


# every ksum at the two ends of N; between them, where the epilogue's `rows` loop and the tile's places take every other
# shape (one to eight rows a thread, the three- and the four-digit places), ksum 3 in both layouts
POWER_CASES = ([(log2n, which, layout) for layout in ("time", "channel") for which in ("1", "3", "hop") for log2n in (9, 14)]
               + [(log2n, "3", layout) for layout in ("time", "channel") for log2n in (10, 11, 12, 13)])


@pytest.mark.parametrize("log2n,which,layout", POWER_CASES)
def test_power_rows_are_the_voltages_bits(cdd, engine, log2n, which, layout):
    _power(cdd, engine, log2n, which, layout)


def test_the_waterfall_feeds_dedisp(cdd, engine):
    """time-major rows of four channels through rtlws_dedisp_run with a table of zeros: the channel sum in ascending
    channel, bit for bit"""
    lead, trail, nseg, tables, x, volts = _power_inputs(cdd, engine, 9)
    rows = cdd.dedisperse(engine, x, tables, lead, trail, ksum=3, layout="time", nseg=nseg)
    assert rows.shape == (nseg * (512 - lead - trail) // 3, 4)
    assert np.array_equal(_bits(rows.T), _bits(cdd_ref.power_rows(volts, 3)))
    summed = engine.dedisp(rows, np.zeros((1, 4), np.int32))
    want = ((rows[:, 0] + rows[:, 1]) + rows[:, 2]) + rows[:, 3]
    assert summed.shape == (1, rows.shape[0]) and np.array_equal(_bits(summed[0]), _bits(want))


# ---- chunking --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("ksum", [0, 16])
def test_segments_run_alone_give_the_whole_runs_bits(cdd, engine, ksum):
    log2n, nchan, nseg, lead, trail = 10, 2, 4, 5, 11
    n = 1 << log2n
    hop = n - lead - trail
    tables = _tables(cdd, log2n, nchan, seed=7, chirp_at=0)
    x = _gauss(nchan, cdd_ref.samples_needed(n, lead, trail, nseg), seed=8)
    whole = cdd.dedisperse(engine, x, tables, lead, trail, ksum=ksum, nseg=nseg)
    part = cdd.dedisperse(engine, np.ascontiguousarray(x[:, hop:]), tables, lead, trail, ksum=ksum, nseg=2)
    per = hop // ksum if ksum else hop
    assert whole.shape == (nchan, nseg * per) and part.shape == (nchan, 2 * per)
    view = np.uint32 if ksum else np.uint64
    assert np.array_equal(part.view(view), np.ascontiguousarray(whole[:, per:3 * per]).view(view))
    assert np.any(whole[:, per:3 * per] != 0)


# ---- graph capture -------------------------------------------------------------------------------------------------

def test_capture_and_replay(built, cdd):
    """tests/test_graph_gpu.py's pattern for this plan at the N whose LDS needs the opt-in: a run captured on a side stream
    enqueues nothing, replays give the eager launch's bits, twice"""
    import torch
    eng = built.Engine(0)
    dev = torch.device("cuda", 0)
    log2n, nchan, nseg, lead, trail = 14, 2, 2, 5, 11
    n = 1 << log2n
    hop = n - lead - trail
    tables = _tables(cdd, log2n, nchan, seed=21)
    need = cdd_ref.samples_needed(n, lead, trail, nseg)
    host = _gauss(nchan, need, seed=22)
    d_in = torch.from_numpy(host.view(np.float32)).to(dev)
    plan = cdd.CddPlan(eng, log2n, lead, trail, nchan, 0, tables)
    out = torch.full((nchan, nseg * hop, 2), float(FILL), dtype=torch.float32, device=dev)
    before = out.clone()
    g = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        with torch.cuda.graph(g, stream=side):
            plan.run(d_in.data_ptr(), need, nseg, out.data_ptr(), nseg * hop, stream=built.torch_stream_handle())
    torch.cuda.current_stream().wait_stream(side)
    assert torch.equal(out, before)                                          # capture enqueued nothing
    eager = torch.zeros_like(out)
    plan.run(d_in.data_ptr(), need, nseg, eager.data_ptr(), nseg * hop, stream=built.torch_stream_handle())
    torch.cuda.synchronize()
    for _ in range(2):
        out.copy_(before)
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(out.view(torch.int32), eager.view(torch.int32))
    got = eager.cpu().numpy().view(np.complex64).reshape(nchan, nseg * hop)
    s1, s2 = cdd_ref.shares(got, host, tables, lead, trail, nseg)
    assert s1 <= 1.0 and s2 <= 1.0
    plan.close()
    eng.close()


# ---- what a plan refuses ---------------------------------------------------------------------------------------------

def test_every_refusal_of_a_run(built, cdd):
    """in the header's order behind the null plan, each with the one before it mended; nothing is launched: the output
    keeps its preset"""
    import torch
    eng = built.Engine(0)
    dev = torch.device("cuda", 0)
    log2n, nchan, lead, trail = 9, 2, 5, 11
    hop = 512 - lead - trail
    tables = _tables(cdd, log2n, nchan, seed=31)
    d_in = torch.zeros((nchan, 2 * hop + 512 + 2, 2), dtype=torch.float32, device=dev)
    out = torch.full((4 * nchan * hop + 8,), float(FILL), dtype=torch.float32, device=dev)
    volts, power = cdd.CddPlan(eng, log2n, lead, trail, nchan, 0, tables), cdd.CddPlan(eng, log2n, lead, trail, nchan, 16, tables)
    i, o, need2 = d_in.data_ptr(), out.data_ptr(), hop + 512
    cases = [
        (volts, (i, need2, 2, o, 2 * hop, "time"), "voltages are channel-major"),
        (volts, (i, need2, 2, o + 4, 2 * hop, "channel"), "d_out must be 8-byte aligned for voltages"),
        (volts, (i, need2 - 1, 2, o, 2 * hop, "channel"), "in_stride must be >= samples_needed"),
        (volts, (i, need2, 2, o, 2 * hop - 1, "channel"), "out_stride must be >= the outputs of a channel"),
        (power, (i, need2, 2, o + 4, 2 * hop // 16 - 1, "channel"), "out_stride must be >= the outputs of a channel"),
        (power, (i, need2, 2, o + 4, nchan - 1, "time"), "out_stride must be >= nchan"),
        (power, (i + 4, need2, 2, o, nchan, "time"), "d_in must be 8-byte aligned"),
        (power, (i, need2, 2, o + 2, nchan, "time"), "d_out must be 4-byte aligned"),
        (power, (i, need2, 2, o, nchan, 2), "unknown layout"),
        (power, (i, need2, -1, o, nchan, "time"), "nseg must be 0 .. 1048576"),
    ]
    for plan, args, text in cases:
        assert plan.run(*args, check=False) == -1 and cdd.last_error() == "rtlws_cdd_run: " + text, (args, cdd.last_error())
    assert volts.samples_needed(0) == 0 and volts.samples_needed(2) == need2 and volts.samples_needed(-1) == -1
    assert power.run(i, 0, 0, o, nchan, "time") == 0 and volts.run(i, 0, 0, o, 0) == 0          # nseg == 0 does nothing
    assert power.run(i, need2, 2, o + 4, nchan, "time") == 0                                      # 4-byte aligned rows are served
    eng.sync()
    got = out.cpu().numpy()
    assert np.all(_bits(got[:1]) == _bits(FILL)) and np.all(_bits(got[1 + 2 * (hop // 16) * nchan:]) == _bits(FILL)) and np.all(got[1:1 + 2 * (hop // 16) * nchan] >= 0)
    volts.close(), power.close()
    eng.close()

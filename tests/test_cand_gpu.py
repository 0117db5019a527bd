"""GPU suite of include/rtlws_cand.h (librtlws_cand.so) against its numpy restatement (tests/cand_ref.py), bits throughout:
f32 on uint32 views with NaN by place, f64 on uint64 views, hits exactly; NaN in the stride's padding and behind
rows_needed, a preset pattern behind every output.  The cube at every block shape and lane-group count, a ragged last
sub-integration and nsamp below sub, the delays' extremes, special steps, both sides of the register-forwarding branch,
masks, special values, hits on and off, a run from a later sub-integration; the refinement at every count of bins per
lane, across the chunk of 32 rows and the 8 trials of a workgroup, with P and T on and off; and the two chained on the
device on a planted pulsar, one plan many times and beside another, both runs in one captured graph, every refusal of
a run."""

import numpy as np
import pytest

import cand_ref
import dedisp_ref
import fold_ref

pytestmark = pytest.mark.gpu

FILL = np.float32(-12345.678)
M64 = 1 << 64
SUB, NSAMP = 100, 1030                           # eleven sub-integrations, the last of 30 samples
SWEEP = (64, 1, 151e6, 2.4e6, 512 / 2.4e6)       # dedisp_ref.DELAY_SETS[2]'s band: up to 854 rows at trial 32


@pytest.fixture(scope="module")
def cand(built):
    import rtlws.cand
    return rtlws.cand


def _same_bits(got, want, what=None):
    """bit for bit, NaN by place (the default NaN of the host's additions and the device's may differ)"""
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    word = np.uint64 if got.dtype == np.float64 else np.uint32
    nan = np.isnan(want) if got.dtype.kind == "f" else np.zeros(want.shape, bool)
    gnan = np.isnan(got) if got.dtype.kind == "f" else nan
    bad = (gnan != nan) | (~nan & (np.ascontiguousarray(got).view(word) != np.ascontiguousarray(want).view(word)))
    assert not bad.any(), (what, np.argwhere(bad)[:5], got[bad][:5], want[bad][:5])


def _sweep(nchan, ncand, top=32):
    """int32 [ncand, nchan]: dispersion sweeps of rtlws_dedisp_delays' own table, the last candidate the steepest"""
    band = (nchan,) + SWEEP[1:]
    trials = dedisp_ref.delays(*band, top + 1, 0.0, 1.0)
    return np.ascontiguousarray(trials[np.linspace(top // 3, top, ncand).astype(int)])


def _fold(cand, engine, x, steps, phases, nbins, sub, nsamp, delays=None, mask=None, want_hits=True, name=None):
    """x float32 [>= rows_needed, nchan] through rtlws.cand.fold with NaN in the stride's padding and in four rows behind
    rows_needed and preset guards behind the outputs, against the restatement; -> (cube, hits) of the device"""
    nchan, ncand = x.shape[1], len(steps)
    need = cand_ref.rows_needed(ncand, nchan, delays, mask, nsamp)
    nsub = cand_ref.subints(nsamp, sub)
    stride = nchan + 4
    padded = np.full((need + 4, stride), np.nan, np.float32)
    padded[:need, :nchan] = x[:need]
    cube, hits = cand.fold(engine, padded, steps, phases, nbins, sub, delays, mask, nsamp=nsamp, in_stride=stride, nchan=nchan,
                           want_hits=want_hits, fill=FILL)
    n1, n2 = ncand * nsub * nchan * nbins, ncand * nsub * nbins
    assert cube.shape == (n1 + cand.GUARD,) and hits.shape == (n2 + cand.GUARD,) and hits.dtype == np.uint32
    assert np.all(cube[n1:].view(np.uint32) == FILL.view(np.uint32)) and np.all(hits[n2:] == FILL.view(np.uint32)), name
    cube, hits = cube[:n1].reshape(ncand, nsub, nchan, nbins), hits[:n2].reshape(ncand, nsub, nbins)
    want_cube, want = cand_ref.cube_ref(x, steps, phases, nchan, nbins, sub, nsamp, delays, mask)
    _same_bits(cube, want_cube, (name, "cube"))
    if want_hits:
        assert np.array_equal(hits, want), (name, np.argwhere(hits != want)[:5])
        assert np.all(hits.sum(axis=2) == np.minimum(sub, nsamp - sub * np.arange(nsub))[None, :]), name
    else:
        assert np.all(hits == FILL.view(np.uint32)), name
    return cube, hits


# ---- the cube -----------------------------------------------------------------------------------------------------

NCHANS, NBINS = (4, 64, 68, 132), (2, 50, 64, 65, 128, 129, 256)


def test_the_cases_cover_the_borders(cand):
    """all three waves_per_block; one lane group, a full wavefront, a ragged one and more than two; a workgroup with a
    whole wavefront behind the row; a ragged last sub-integration"""
    assert {cand.fold_geometry(1, 4, nbins, SUB)[4] for nbins in NBINS} == {4, 2, 1}
    assert [-(-n // 64) for n in NCHANS] == [1, 1, 2, 3] and [n % 64 for n in NCHANS] == [4, 0, 4, 4]
    assert cand.fold_geometry(1, 68, 64, SUB, NSAMP)[1] == 11 and cand.fold_geometry(1, 132, 129, SUB, NSAMP)[1] == 33
    assert NSAMP % SUB == 30 and cand_ref.subints(NSAMP, SUB) == 11


@pytest.mark.parametrize("nbins", NBINS)
@pytest.mark.parametrize("nchan", NCHANS)
def test_every_block_shape_and_lane_group_count(cand, engine, nchan, nbins):
    """three candidates behind a dispersion sweep's delays (one where the row holds too few channels for a sweep: random to
    40), non-dyadic periods, seeded phases"""
    ncand = 3
    steps, phases = fold_ref.table(ncand, seed=nchan + nbins, first=2.7 + nbins / 3.0, spread=11.3)
    delays = _sweep(nchan, ncand) if nchan >= 64 else dedisp_ref.random_table(ncand, nchan, 40, seed=nbins)
    x = dedisp_ref.signed_rows(NSAMP + int(delays.max()), nchan, seed=nchan * 1000 + nbins)
    _fold(cand, engine, x, steps, phases, nbins, SUB, NSAMP, delays, name=(nchan, nbins))


@pytest.mark.parametrize("nchan,nbins,nsamp,sub", [(4, 2, 37, SUB), (68, 65, 37, SUB), (132, 256, 99, SUB), (64, 50, 1, 16), (68, 129, 16, 16),
                                                     (68, 64, 17, 16), (132, 50, 5 * 16 + 15, 16)])
def test_one_candidate_zero_delays_and_short_runs(cand, engine, nchan, nbins, nsamp, sub):
    """ncand 1 with a NULL delay table; nsamp below sub, one sample, sub at its least, the unrolled loop's ends (15, 16 and
    17 samples)"""
    steps, phases = fold_ref.table(1, seed=nsamp, first=3.1)
    x = dedisp_ref.signed_rows(nsamp, nchan, seed=nsamp + nchan)
    _fold(cand, engine, x, steps, phases, nbins, sub, nsamp, name=(nchan, nbins, nsamp))


def test_the_delays_extremes(cand, engine):
    """nchan 4 with the entries (0, 65535, 1, 65534), and the same with 65535 masked: rows_needed falls to nsamp + 65534"""
    delays = np.array([[0, 65535, 1, 65534]], np.int32)
    nsamp = 130
    steps, phases = fold_ref.table(1, seed=9, first=7.3)
    x = dedisp_ref.pooled_rows(nsamp + 65535, 4, seed=9)
    cube, _ = _fold(cand, engine, x, steps, phases, 50, SUB, nsamp, delays, name="extremes")
    assert cube.any(axis=(0, 1, 3)).all()
    _fold(cand, engine, x, steps, phases, 50, SUB, nsamp, delays, mask=np.array([1, 0, 1, 1], np.uint8), name="extremes, one masked")


@pytest.mark.parametrize("nbins", [2, 50, 256])
def test_special_steps_and_both_sides_of_the_forwarding_branch(cand, engine, nbins):
    """steps 0 (the bin never changes), 1 (nor here), 2^63, 2^64 - 1 (backwards), the least step that changes the bin at
    every sample, and an ordinary one; phases at the wrap"""
    every = (-(-(1 << 32) // nbins) + 1) << 32                                  # the bin looks at the phase's high word: a bin and a little a sample
    steps = np.array([0, 1, 1 << 63, M64 - 1, every, fold_ref.step_of(33.3)], np.uint64)
    phases = np.array([M64 - 1, 0, 12345, 5, 7, 1 << 63], np.uint64)
    nsamp = 2 * SUB + 7
    b = fold_ref.bins_of(steps[4], phases[4], nbins, 0, nsamp)
    assert np.all(np.diff(b) != 0) and np.all(np.diff(fold_ref.bins_of(steps[1], phases[1], nbins, 0, nsamp)) == 0)
    x = dedisp_ref.signed_rows(nsamp + 40, 68, seed=nbins)
    delays = dedisp_ref.random_table(6, 68, 40, seed=3)
    cube, hits = _fold(cand, engine, x, steps, phases, nbins, SUB, nsamp, delays, name=("steps", nbins))
    assert hits[0, 0, nbins - 1] == SUB and hits[1, 0, 0] == SUB


def test_masks(cand, engine):
    """a mask that drops a whole lane group (the second wavefront of a workgroup reads nothing), a scattered one, and one
    that drops every channel: +0.0 throughout and no row read at all (the rows are all NaN)"""
    nchan, nbins, ncand = 132, 64, 2
    steps, phases = fold_ref.table(ncand, seed=5, first=4.4)
    delays = _sweep(nchan, ncand)
    x = dedisp_ref.signed_rows(NSAMP + int(delays.max()), nchan, seed=55)
    group = np.ones(nchan, np.uint8)
    group[64:128] = 0
    cube, _ = _fold(cand, engine, x, steps, phases, nbins, SUB, NSAMP, delays, group, name="a lane group masked")
    assert not cube[:, :, 64:128].any() and not np.signbit(cube[:, :, 64:128]).any() and cube[:, :, 128:].any()
    _fold(cand, engine, x, steps, phases, nbins, SUB, NSAMP, delays, dedisp_ref.random_mask(nchan, 8), name="a scattered mask")
    none = np.zeros(nchan, np.uint8)
    assert cand_ref.rows_needed(ncand, nchan, delays, none, NSAMP) == NSAMP
    cube, hits = _fold(cand, engine, np.full((NSAMP, nchan), np.nan, np.float32), steps, phases, nbins, SUB, NSAMP, delays, none, name="all masked")
    assert not cube.view(np.uint32).any() and hits.sum() == ncand * NSAMP


@pytest.mark.parametrize("nbins", [2, 65])
def test_special_values(cand, engine, nbins):
    """NaN, both infinities, -0.0 and subnormals among ordinary floats (dedisp_ref.special_rows), and rows of subnormals
    alone, whose sums stay subnormal"""
    nchan, nsamp = 68, 3 * SUB + 1
    steps, phases = fold_ref.table(2, seed=nbins, first=5.9)
    delays = dedisp_ref.random_table(2, nchan, 25, seed=nbins)
    x = dedisp_ref.special_rows(nsamp + 25, nchan, seed=nbins)
    assert np.isnan(x).any() and np.isposinf(x).any() and np.isneginf(x).any() and (x.view(np.uint32) == 0x80000000).any()
    cube, _ = _fold(cand, engine, x, steps, phases, nbins, SUB, nsamp, delays, name=("special", nbins))
    assert np.isnan(cube).any() and not np.isnan(cube).all()                    # a NaN reaches its bin and no other
    tiny = (dedisp_ref.hashed_ints((nsamp + 25) * nchan, 300, seed=1).astype(np.uint32) + np.uint32(1)).view(np.float32).reshape(-1, nchan)
    cube, _ = _fold(cand, engine, tiny, steps, phases, nbins, SUB, nsamp, delays, name=("subnormal", nbins))
    assert cube.any() and np.all(np.abs(cube) < np.finfo(np.float32).tiny)
    zeros = np.full((nsamp + 25, nchan), -0.0, np.float32)
    cube, _ = _fold(cand, engine, zeros, steps, phases, nbins, SUB, nsamp, delays, name=("-0.0", nbins))
    assert not cube.view(np.uint32).any()                                       # +0.0 + -0.0 = +0.0


def test_hits_off(cand, engine):
    steps, phases = fold_ref.table(3, seed=12, first=3.7)
    x = dedisp_ref.signed_rows(NSAMP, 68, seed=12)
    _fold(cand, engine, x, steps, phases, 129, SUB, NSAMP, want_hits=False, name="no hits")


def _on_device(torch, host):
    return torch.from_numpy(np.ascontiguousarray(host)).to(torch.device("cuda", 0))


def _preset(torch, count, dtype=np.float32):
    return _on_device(torch, np.full(count + 8, FILL, dtype))


def _guarded(tensor, count, what=None):
    got = tensor.cpu().numpy()
    assert got.size == count + 8 and np.all(got[count:] == got.dtype.type(FILL)), what
    return got[:count]


def test_a_run_from_a_later_subintegration(built, cand, engine):
    """the run over the rows from 3 sub on with every phi0 replaced by rtlws_fold_phase_at: the whole run's sub-integrations
    from 3 on, bit for bit; the rows stay where they are, the pointer moves"""
    import torch
    nchan, nbins, ncand, s0 = 68, 50, 2, 3
    steps, phases = fold_ref.table(ncand, seed=21, first=6.1)
    delays = _sweep(nchan, ncand)
    host = dedisp_ref.signed_rows(NSAMP + int(delays.max()), nchan, seed=21)
    rows = _on_device(torch, host)
    whole = cand.CandFoldPlan(engine, steps, phases, nchan, nbins, SUB, delays)
    later = cand.CandFoldPlan(engine, steps, [built.fold_phase_at(st, ph, s0 * SUB) for st, ph in zip(steps, phases)], nchan, nbins, SUB, delays)
    nsub = whole.subints(NSAMP)
    n1, n2 = ncand * nsub * nchan * nbins, ncand * (nsub - s0) * nchan * nbins
    a, b = _preset(torch, n1), _preset(torch, n2)
    ha, hb = _preset(torch, ncand * nsub * nbins, np.int32), _preset(torch, ncand * (nsub - s0) * nbins, np.int32)
    whole.run(rows.data_ptr(), nchan, NSAMP, a.data_ptr(), ha.data_ptr(), stream=built.torch_stream_handle())
    later.run(rows.data_ptr() + 4 * s0 * SUB * nchan, nchan, NSAMP - s0 * SUB, b.data_ptr(), hb.data_ptr(), stream=built.torch_stream_handle())
    torch.cuda.synchronize()
    want, want_hits = cand_ref.cube_ref(host, steps, phases, nchan, nbins, SUB, NSAMP, delays)
    got = _guarded(a, n1).reshape(want.shape)
    _same_bits(got, want, "whole")
    _same_bits(_guarded(b, n2).reshape(ncand, nsub - s0, nchan, nbins), got[:, s0:], "later")
    assert np.array_equal(_guarded(hb, ncand * (nsub - s0) * nbins).reshape(ncand, nsub - s0, nbins), want_hits[:, s0:].view(np.int32))
    assert whole.rows_needed(NSAMP) == NSAMP + int(delays.max()) and whole.rows_needed(0) == 0
    whole.close()
    later.close()


# ---- the refinement -----------------------------------------------------------------------------------------------

def _search(cand, engine, cube, a, g, want_prof=True, want_tphase=True, name=None):
    ncand, nsub, nchan, nbins = cube.shape
    ndm, ntr = a.shape[1], g.shape[1]
    stat, total, prof, tphase = cand.search(engine, cube, a, g, want_prof=want_prof, want_tphase=want_tphase, fill=FILL)
    n0, n1, n2 = ncand * ndm * ntr, ncand * ndm * ntr * nbins, ncand * ndm * nsub * nbins
    for got, n in ((stat, n0), (total, n0), (prof, n1), (tphase, n2)):
        assert got.shape == (n + cand.GUARD,) and np.all(got[n:] == got.dtype.type(FILL)), name
    want = cand_ref.search_ref(cube, a, g)
    _same_bits(stat[:n0].reshape(ncand, ndm, ntr), want[0], (name, "stat"))
    _same_bits(total[:n0].reshape(ncand, ndm, ntr), want[1], (name, "total"))
    if want_prof:
        _same_bits(prof[:n1].reshape(ncand, ndm, ntr, nbins), want[2], (name, "P"))
    else:
        assert np.all(prof == FILL), name
    if want_tphase:
        _same_bits(tphase[:n2].reshape(ncand, ndm, nsub, nbins), want[3], (name, "T"))
    else:
        assert np.all(tphase == FILL), name


# (nsub, ndm, ntr): each count of the issue's lists, and the borders of the stages' own tiles: 8 trials a workgroup
# (ndm 5, 8, 33; ntr 7, 16, 65) and 32 rows a chunk (nchan 68; nsub 33 and 64)
SEARCH_SHAPES = ((1, 1, 1), (3, 5, 7), (17, 33, 65), (17, 1, 65), (1, 33, 7), (33, 8, 16), (64, 5, 1))


# the counts of bins a lane holds, ceil(nbins / 64) = 1 .. 4: both sides of every border (64 | 65, 128 | 129, 192 | 193), the
# three upper ones at the channel count whose stage 1 crosses the chunk
FIRST_SEARCH_BINS = (2, 50, 64, 65, 256)
SEARCH_BINS = [(nbins, nchan) for nchan in (4, 68) for nbins in FIRST_SEARCH_BINS] + [(nbins, 68) for nbins in (128, 129, 192, 193)]


@pytest.mark.parametrize("nbins,nchan", SEARCH_BINS)
def test_every_count_of_bins_per_lane_and_every_tile_border(cand, engine, nbins, nchan):
    """Gaussian f32 with exponents over 2^-6 .. 2^6, where the order of the additions shows; shifts that include 0 and
    nbins - 1; two candidates"""
    for nsub, ndm, ntr in SEARCH_SHAPES:
        seed = nbins * 100 + nchan + nsub
        cube = cand_ref.gaussian_cube(2, nsub, nchan, nbins, seed)
        a, g = cand_ref.shift_table((2, ndm, nchan), nbins, seed + 1), cand_ref.shift_table((2, ntr, nsub), nbins, seed + 2)
        assert a.min() == g.min() == 0 and a.max() == g.max() == nbins - 1
        _search(cand, engine, cube, a, g, name=(nbins, nchan, nsub, ndm, ntr))


@pytest.mark.parametrize("want_prof,want_tphase", [(False, False), (True, False), (False, True)])
def test_profiles_and_time_phase_rows_on_and_off(cand, engine, want_prof, want_tphase):
    cube = cand_ref.gaussian_cube(1, 17, 68, 129, seed=77)
    a, g = cand_ref.shift_table((1, 5, 68), 129, 78), cand_ref.shift_table((1, 7, 17), 129, 79)
    _search(cand, engine, cube, a, g, want_prof, want_tphase, name=(want_prof, want_tphase))


def test_special_values_in_the_cube(cand, engine):
    """NaN and infinities reach the bins their shifts send them to; -0.0 throughout sums to +0.0"""
    cube = cand_ref.gaussian_cube(1, 3, 8, 50, seed=80)
    cube[0, 1, 3, 7], cube[0, 2, 5, 49], cube[0, 0, 0, 0] = np.nan, np.inf, -np.inf
    a, g = cand_ref.shift_table((1, 5, 8), 50, 81), cand_ref.shift_table((1, 7, 3), 50, 82)
    _search(cand, engine, cube, a, g, name="special")
    _search(cand, engine, np.full((1, 3, 8, 50), -0.0, np.float32), a, g, name="-0.0")


# ---- both ---------------------------------------------------------------------------------------------------------

def test_the_chain_on_the_device_finds_the_planted_offsets(built, cand, engine):
    """the synthetic dispersed pulsar of tests/test_cand_cpu.py, 64 channels x 4096 rows: the cube goes from rtlws_cand_fold_run
    to rtlws_cand_search_run where it lies; every output is the restatement's bits and the planted offsets are the strict
    maximum of stat"""
    import torch
    import test_cand_cpu
    p = cand_ref.PULSAR
    box = {}

    def fold(rows, steps, phases, nchan, nbins, sub, nsamp, delays):
        box.update(rows=rows, steps=steps, phases=phases, delays=delays)
        return np.zeros((1, cand_ref.subints(nsamp, sub), nchan, nbins), np.float32)                   # the shape is all planted_search asks

    shape, a, g = test_cand_cpu.planted_search(cand, fold)
    ncand, nsub, nchan, nbins = shape.shape
    ndm, ntr = a.shape[1], g.shape[1]
    rows = _on_device(torch, box["rows"])
    fplan = cand.CandFoldPlan(engine, box["steps"], box["phases"], nchan, nbins, p["sub"], box["delays"])
    splan = cand.CandSearchPlan(engine, ncand, nsub, nchan, nbins, a, g)
    assert fplan.rows_needed(p["nsamp"]) == box["rows"].shape[0]
    n_cube, n_hits, n_sum, n_prof, n_t = shape.size, nsub * nbins, ndm * ntr, ndm * ntr * nbins, ndm * nsub * nbins
    cube, hits = _preset(torch, n_cube), _preset(torch, n_hits, np.int32)
    stat, total, prof, tphase = _preset(torch, n_sum, np.float64), _preset(torch, n_sum, np.float64), _preset(torch, n_prof), _preset(torch, n_t)
    st = built.torch_stream_handle()
    fplan.run(rows.data_ptr(), nchan, p["nsamp"], cube.data_ptr(), hits.data_ptr(), stream=st)
    splan.run(cube.data_ptr(), stat.data_ptr(), total.data_ptr(), prof.data_ptr(), tphase.data_ptr(), stream=st)
    torch.cuda.synchronize()
    want_cube, want_hits = cand_ref.cube_ref(box["rows"], box["steps"], box["phases"], nchan, nbins, p["sub"], p["nsamp"], box["delays"])
    want = cand_ref.search_ref(want_cube, a, g)
    _same_bits(_guarded(cube, n_cube).reshape(shape.shape), want_cube, "cube")
    assert np.array_equal(_guarded(hits, n_hits).reshape(1, nsub, nbins), want_hits.view(np.int32))
    got_stat = _guarded(stat, n_sum).reshape(1, ndm, ntr)
    _same_bits(got_stat, want[0], "stat")
    _same_bits(_guarded(total, n_sum).reshape(1, ndm, ntr), want[1], "total")
    _same_bits(_guarded(prof, n_prof).reshape(1, ndm, ntr, nbins), want[2], "P")
    _same_bits(_guarded(tphase, n_t).reshape(1, ndm, nsub, nbins), want[3], "T")
    best = np.unravel_index(np.argmax(got_stat[0]), got_stat[0].shape)
    assert best == (p["q_true"], p["r_true"]) and (got_stat[0] == got_stat[0].max()).sum() == 1
    fplan.close()
    splan.close()


def test_one_plan_many_runs_and_two_plans_side_by_side(built, cand, engine):
    """two fold plans and two search plans of different shapes, run in turn twice over fresh buffers: every run the
    restatement's bits"""
    import torch
    st = built.torch_stream_handle()
    cases = []
    for nchan, nbins, nsamp, seed in ((68, 50, 330, 1), (64, 129, 250, 2)):
        steps, phases = fold_ref.table(2, seed=seed, first=4.9)
        delays = _sweep(nchan, 2)
        host = dedisp_ref.signed_rows(nsamp + int(delays.max()), nchan, seed=seed)
        nsub = cand_ref.subints(nsamp, SUB)
        a, g = cand_ref.shift_table((2, 5, nchan), nbins, seed + 10), cand_ref.shift_table((2, 7, nsub), nbins, seed + 20)
        want_cube, want_hits = cand_ref.cube_ref(host, steps, phases, nchan, nbins, SUB, nsamp, delays)
        cases.append(dict(nchan=nchan, nbins=nbins, nsamp=nsamp, nsub=nsub, rows=_on_device(torch, host), want_cube=want_cube, want_hits=want_hits,
                          want=cand_ref.search_ref(want_cube, a, g), fplan=cand.CandFoldPlan(engine, steps, phases, nchan, nbins, SUB, delays),
                          splan=cand.CandSearchPlan(engine, 2, nsub, nchan, nbins, a, g)))
    for _ in range(2):
        outs = []
        for k in cases:
            n_cube, n_sum = k["want_cube"].size, k["want"][0].size
            cube, hits = _preset(torch, n_cube), _preset(torch, k["want_hits"].size, np.int32)
            stat, total = _preset(torch, n_sum, np.float64), _preset(torch, n_sum, np.float64)
            k["fplan"].run(k["rows"].data_ptr(), k["nchan"], k["nsamp"], cube.data_ptr(), hits.data_ptr(), stream=st)
            k["splan"].run(cube.data_ptr(), stat.data_ptr(), total.data_ptr(), stream=st)
            outs.append((cube, hits, stat, total))
        torch.cuda.synchronize()
        for k, (cube, hits, stat, total) in zip(cases, outs):
            _same_bits(_guarded(cube, k["want_cube"].size).reshape(k["want_cube"].shape), k["want_cube"], "cube")
            assert np.array_equal(_guarded(hits, k["want_hits"].size).reshape(k["want_hits"].shape), k["want_hits"].view(np.int32))
            _same_bits(_guarded(stat, k["want"][0].size).reshape(k["want"][0].shape), k["want"][0], "stat")
            _same_bits(_guarded(total, k["want"][1].size).reshape(k["want"][1].shape), k["want"][1], "total")
    for k in cases:
        k["fplan"].close()
        k["splan"].close()


def test_capture_and_replay(built, cand):
    """tests/test_fold_gpu.py::test_capture_and_replay's pattern for both plans in one graph on one stream: the capture
    enqueues nothing, and a replay over new rows gives the restatement's bits for them"""
    import torch
    eng = built.Engine(0)
    nchan, nbins, ncand, nsamp = 68, 65, 2, 330
    steps, phases = fold_ref.table(ncand, seed=31, first=5.3)
    delays = _sweep(nchan, ncand)
    hosts = [dedisp_ref.signed_rows(nsamp + int(delays.max()), nchan, seed=s) for s in (31, 32)]
    nsub = cand_ref.subints(nsamp, SUB)
    a, g = cand_ref.shift_table((ncand, 5, nchan), nbins, 33), cand_ref.shift_table((ncand, 7, nsub), nbins, 34)
    rows = _on_device(torch, hosts[0])
    fplan = cand.CandFoldPlan(eng, steps, phases, nchan, nbins, SUB, delays)
    splan = cand.CandSearchPlan(eng, ncand, nsub, nchan, nbins, a, g)
    n_cube, n_sum = ncand * nsub * nchan * nbins, ncand * 5 * 7
    outs = [_preset(torch, n_cube), _preset(torch, ncand * nsub * nbins, np.int32), _preset(torch, n_sum, np.float64), _preset(torch, n_sum, np.float64),
            _preset(torch, n_sum * nbins), _preset(torch, ncand * 5 * nsub * nbins)]
    before = [o.clone() for o in outs]
    graph = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            fplan.run(rows.data_ptr(), nchan, nsamp, outs[0].data_ptr(), outs[1].data_ptr(), stream=built.torch_stream_handle())
            splan.run(outs[0].data_ptr(), outs[2].data_ptr(), outs[3].data_ptr(), outs[4].data_ptr(), outs[5].data_ptr(), stream=built.torch_stream_handle())
    torch.cuda.current_stream().wait_stream(side)
    assert all(torch.equal(o, b) for o, b in zip(outs, before))                  # capture enqueued nothing
    for host in hosts:
        rows.copy_(torch.from_numpy(host))
        for o, b in zip(outs, before):
            o.copy_(b)
        graph.replay()
        torch.cuda.synchronize()
        want_cube, want_hits = cand_ref.cube_ref(host, steps, phases, nchan, nbins, SUB, nsamp, delays)
        want = cand_ref.search_ref(want_cube, a, g)
        _same_bits(_guarded(outs[0], n_cube).reshape(want_cube.shape), want_cube, "replayed cube")
        assert np.array_equal(_guarded(outs[1], want_hits.size).reshape(want_hits.shape), want_hits.view(np.int32))
        for o, w, what in zip(outs[2:], want, ("stat", "total", "P", "T")):
            _same_bits(_guarded(o, w.size).reshape(w.shape), w, "replayed " + what)
    fplan.close()
    splan.close()
    eng.close()


def test_every_refusal_of_a_run(cand, engine):
    """with live plans: each refusal of the header's list in its order, -1 and the text, and nothing written"""
    nchan, nbins = 8, 4
    steps, phases = fold_ref.table(64, seed=41)
    fplan = cand.CandFoldPlan(engine, steps, phases, nchan, nbins, 16)
    rows = engine.upload(np.zeros((64, nchan), np.float32))
    cube = engine.upload(np.full(64 * 4 * nchan * nbins + 8, FILL, np.float32))
    hits = engine.upload(np.full(64 * 4 * nbins + 8, FILL, np.float32))
    L = cand.lib()
    run = lambda d_rows, in_stride, nsamp, d_cube, d_hits: L.rtlws_cand_fold_run(fplan.h, d_rows, in_stride, nsamp, d_cube, d_hits, None)
    for args, text in (((rows.ptr, nchan, -1, cube.ptr, hits.ptr), "nsamp must be 0 .. 2^30"),
                       ((rows.ptr, nchan, (1 << 30) + 1, cube.ptr, hits.ptr), "nsamp must be 0 .. 2^30"),
                       ((rows.ptr, 0, 64, cube.ptr, hits.ptr), "in_stride must be >= 4 and a multiple of 4"),
                       ((rows.ptr, nchan + 2, 64, cube.ptr, hits.ptr), "in_stride must be >= 4 and a multiple of 4"),
                       ((None, nchan, 64, cube.ptr, hits.ptr), "null pointer"), ((rows.ptr, nchan, 64, None, hits.ptr), "null pointer"),
                       ((rows.ptr + 8, nchan, 64, cube.ptr, hits.ptr), "d_rows must be 16-byte aligned"),
                       ((rows.ptr, nchan, 64, cube.ptr + 2, hits.ptr), "d_cube must be 4-byte aligned"),
                       ((rows.ptr, nchan, 64, cube.ptr, hits.ptr + 1), "d_hits must be 4-byte aligned"),
                       ((rows.ptr, 4, 64, cube.ptr, hits.ptr), "in_stride must be >= nchan"),
                       ((rows.ptr, nchan, 1 << 30, cube.ptr, hits.ptr), "more workgroups than one grid holds")):
        assert run(*args) == -1 and cand.last_error() == "rtlws_cand_fold_run: " + text, (args, cand.last_error())
    assert run(rows.ptr, nchan, 0, cube.ptr, hits.ptr) == 0 and cand.last_error() == ""              # nsamp 0 does nothing
    a, g = np.zeros((1, 1, nchan), np.int32), np.zeros((1, 1, 4), np.int32)
    splan = cand.CandSearchPlan(engine, 1, 4, nchan, nbins, a, g)
    sums = engine.upload(np.full(16, FILL, np.float64))
    run = lambda d_cube, d_stat, d_total, d_prof, d_t: L.rtlws_cand_search_run(splan.h, d_cube, d_stat, d_total, d_prof, d_t, None)
    for args, text in (((None, sums.ptr, sums.ptr + 8, None, None), "null pointer"), ((cube.ptr, None, sums.ptr, None, None), "null pointer"),
                       ((cube.ptr, sums.ptr, None, None, None), "null pointer"), ((cube.ptr + 1, sums.ptr, sums.ptr + 8, None, None), "d_cube must be 4-byte aligned"),
                       ((cube.ptr, sums.ptr + 4, sums.ptr + 8, None, None), "d_stat must be 8-byte aligned"),
                       ((cube.ptr, sums.ptr, sums.ptr + 4, None, None), "d_total must be 8-byte aligned"),
                       ((cube.ptr, sums.ptr, sums.ptr + 8, cube.ptr + 2, None), "d_prof must be 4-byte aligned"),
                       ((cube.ptr, sums.ptr, sums.ptr + 8, None, cube.ptr + 3), "d_tphase must be 4-byte aligned")):
        assert run(*args) == -1 and cand.last_error() == "rtlws_cand_search_run: " + text, (args, cand.last_error())
    engine.sync()
    assert np.all(engine.download(cube, np.float32, (64 * 4 * nchan * nbins + 8,)) == FILL)
    assert np.all(engine.download(hits, np.float32, (64 * 4 * nbins + 8,)) == FILL) and np.all(engine.download(sums, np.float64, (16,)) == np.float64(FILL))
    for plan in (fplan, splan):
        plan.close()
    for buf in (rows, cube, hits, sums):
        buf.free()

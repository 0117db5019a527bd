"""GPU suite of include/rtlws_dedisp.h (librtlws_dedisp.so) against its numpy restatement (tests/dedisp_ref.py): every
comparison with it bit for bit on uint32 views, the f64 bound on every case, padding columns, rows behind rows_needed
and the output's padding untouched, runs from a later row, the spectrometer's rows end to end, and graph capture; then
the plan on both sides of every border of its forms (tests/dedisp_form_cases.py), signed rows, rows that hold -0.0,
subnormals, infinities and NaN, NaN and -Inf under the mask, the limits of the table, and one plan run many times, over
a sub-band of a wider waterfall and beside another plan on another stream."""
import numpy as np
import pytest

import dedisp_form_cases as forms
import dedisp_ref
from dedisp_ref import DELAY_SETS

pytestmark = pytest.mark.gpu

TILE = 256                                       # tile_out; every case asserts that rtlws_dedisp_geometry says so
FILL = np.float32(-12345.678)                    # the sums are of non-negative floats: no output is this
NCHANS = (4, 16, 20, 64, 1024, 4096)
NTRIALS = (33, 9, 8, 7, 2, 1)                    # paired with NCHANS: the widest rows with the fewest trials
NOUTS = (1, TILE - 1, TILE, TILE + 1, 2 * TILE + 3)
MASKS = ("none", "random", "zero", "first", "last", "middle")
KINDS = ("zero", "rand1", "rand5", "rand300", "rand5000", "mixed")


def _mask(code, nchan, seed):
    if code == "none":
        return None
    if code == "random":
        return dedisp_ref.random_mask(nchan, seed)
    if code == "zero":
        return np.zeros(nchan, np.uint8)
    return dedisp_ref.one_kept(nchan, {"first": 0, "last": nchan - 1, "middle": (nchan // 2 + 1) % nchan}[code])


def _table(kind, ntrials, nchan, seed):
    if kind == "zero":
        return np.zeros((ntrials, nchan), np.int32)
    if kind == "mixed":
        return dedisp_ref.mixed_table(ntrials, nchan, seed)
    if kind.startswith("rand"):
        return dedisp_ref.random_table(ntrials, nchan, int(kind[4:]), seed)
    return dedisp_ref.delays(*DELAY_SETS[int(kind[3:])])


def _cases():
    """Every value of NCHANS, NTRIALS, NOUTS and MASKS with every kind of table; the mixed table needs more than eight
    trials, so its rows are paired with 33 and 9 trials only.  The tables of rtlws_dedisp_delays have their own shapes:
    every NOUTS and MASKS value with that kind, the two large ones with the masks that keep one position."""
    out = []
    for kk, kind in enumerate(KINDS):
        for j in range(6):
            ntrials = (33, 9)[j % 2] if kind == "mixed" else NTRIALS[j]
            out.append((kind, NCHANS[j], ntrials, NOUTS[(j + kk) % 5], MASKS[(j + 2 * kk) % 6]))
    for kind, nout, mask in (("set0", 1, "first"), ("set0", TILE + 1, "random"), ("set1", TILE - 1, "none"), ("set1", 2 * TILE + 3, "zero"),
                             ("set2", TILE, "none"), ("set2", 2 * TILE + 3, "random"), ("set2", TILE + 1, "last"), ("set3", 1, "none"),
                             ("set3", TILE + 1, "middle"), ("set3", TILE - 1, "zero")):
        args = DELAY_SETS[int(kind[3:])]
        out.append((kind, args[0], args[5], nout, mask))
    return out


CASES = _cases()
WORST = {}


def test_the_cases_cover_the_lists():
    for kind in KINDS:
        mine = [c for c in CASES if c[0] == kind]
        assert {c[1] for c in mine} == set(NCHANS) and {c[3] for c in mine} == set(NOUTS) and {c[4] for c in mine} == set(MASKS)
        assert {c[2] for c in mine} == (set(NTRIALS) if kind != "mixed" else {33, 9})
    sets = [c for c in CASES if c[0].startswith("set")]
    assert {c[0] for c in sets} == {"set0", "set1", "set2", "set3"} and {c[3] for c in sets} == set(NOUTS) and {c[4] for c in sets} == set(MASKS)


@pytest.mark.parametrize("case", CASES, ids=["-".join(str(x) for x in c) for c in CASES])
def test_against_the_restatement(built, engine, case):
    kind, nchan, ntrials, nout, mask_code = case
    seed = CASES.index(case) + 1
    delays, mask = _table(kind, ntrials, nchan, seed), _mask(mask_code, nchan, seed)
    rc, blocks, threads, lds, tile, per, most = built.dedisp_geometry(delays, mask, nout)
    cap = 8 if ntrials >= 5 else 4 if ntrials >= 3 else ntrials
    assert rc == 0 and tile == TILE and threads == 256 and blocks == -(-nout // tile) * -(-ntrials // per) and per <= cap
    if kind in ("rand300", "rand5000", "mixed"):
        # positions 0 and 1 of one trial lie that far apart (the mixed table: of its random trials): the narrower plans
        wide = built.dedisp_geometry(delays, None, nout)[5]
        assert wide == 1 and (wide < cap or ntrials == 1), (wide, cap)
        if mask is None:
            assert per == 1
    elif mask_code in ("none", "zero") or kind in ("zero", "rand1", "rand5"):
        assert per == cap
    need = dedisp_ref.rows_needed(delays, mask, nout)
    assert need == nout + most
    # NaN in the padding columns and in every row from rows_needed on; the output's padding preset
    rows = np.full((need + 3, nchan + 4), np.nan, np.float32)
    rows[:need, :nchan] = dedisp_ref.pooled_rows(need, nchan, seed)
    whole = engine.dedisp(rows, delays, mask, nout=nout, in_stride=nchan + 4, out_stride=nout + 3, fill=FILL)
    assert whole.shape == (ntrials, nout + 3) and whole.dtype == np.float32
    assert np.all(whole[:, nout:].view(np.uint32) == FILL.view(np.uint32))
    got = np.ascontiguousarray(whole[:, :nout])
    assert not np.isnan(got).any()
    want, want64 = dedisp_ref.dedisp_both(rows, delays, mask, nout)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), np.argwhere(got.view(np.uint32) != want.view(np.uint32))[:5]
    kept = [i for i in range(nchan) if mask is None or mask[i]]
    if len(kept) == 1:                           # that column, delayed: the indexing without any summation
        for t in range(ntrials):
            d = delays[t, kept[0]]
            assert np.array_equal(got[t].view(np.uint32), rows[d:d + nout, kept[0]].view(np.uint32))
    if not kept:
        assert not got.view(np.uint32).any()     # +0.0, no sign bit
    bound = nchan * 2.0 ** -24 * want64            # the terms are non-negative: their magnitudes sum to the f64 sum
    err = np.abs(got.astype(np.float64) - want64)
    assert np.all(err <= bound)
    ratio = float((err[bound > 0] / bound[bound > 0]).max()) if (bound > 0).any() else 0.0
    WORST[case] = ratio
    print("%s: %d trials a workgroup, %d B of LDS, |D - D64| at most %.4f of M 2^-24 sum|terms|; the worst of the %d cases so far %.4f"
          % ("-".join(str(x) for x in case), per, lds, ratio, len(WORST), max(WORST.values())))


def _stepped(ntrials, nchan, step):
    """trial t delays every position by t * step rows, and the odd positions by one more"""
    return (np.arange(ntrials)[:, None] * step + np.arange(nchan)[None, :] % 2).astype(np.int32)


# (table, trials a workgroup, LDS) for every form a plan takes: groups of 8, 4 and 2 in either LDS, one trial with 128-,
# 64-, 32- and 16-byte pieces of a row, one trial with every position by itself
FORMS = ((lambda: np.zeros((3, 20), np.int32), 4, 36 * 1024), (lambda: _stepped(9, 20, 40), 4, 64 * 1024),
         (lambda: _stepped(9, 20, 3), 8, 36 * 1024), (lambda: _stepped(9, 20, 30), 8, 64 * 1024),
         (lambda: _stepped(9, 20, 100), 2, 64 * 1024), (lambda: _stepped(2, 20, 10), 2, 36 * 1024),
         (lambda: _stepped(9, 20, 300), 1, 36 * 1024), (lambda: dedisp_ref.random_table(9, 20, 200, 1) + _stepped(9, 20, 300), 1, 64 * 1024),
         (lambda: dedisp_ref.random_table(9, 20, 300, 1), 1, 36 * 1024), (lambda: dedisp_ref.random_table(9, 20, 1000, 1), 1, 64 * 1024),
         (lambda: dedisp_ref.random_table(9, 20, 1900, 1), 1, 36 * 1024), (lambda: dedisp_ref.random_table(9, 20, 3500, 1), 1, 64 * 1024),
         (lambda: dedisp_ref.random_table(9, 20, 4000, 1), 1, 36 * 1024))


@pytest.mark.parametrize("which", range(len(FORMS)))
def test_every_form_of_the_plan(built, engine, which):
    """20 positions (a last chunk of one quad behind whatever the plan's chunk is) at tile_out + 1 outputs, bit for bit"""
    make, per, lds = FORMS[which]
    delays = make()
    nout = TILE + 1
    geo = built.dedisp_geometry(delays, None, nout)
    assert (geo[0], geo[3], geo[5]) == (0, lds, per), geo
    rows = dedisp_ref.pooled_rows(dedisp_ref.rows_needed(delays, None, nout), 20, seed=which)
    for mask in (None, dedisp_ref.random_mask(20, which)):
        got = engine.dedisp(rows, delays, mask, nout=nout)
        assert np.array_equal(got.view(np.uint32), dedisp_ref.dedisp_ref(rows, delays, mask, nout).view(np.uint32)), mask


@pytest.mark.parametrize("kind,ntrials,nchan", [("set2", 33, 64), ("rand300", 9, 20), ("rand5000", 2, 16)])
def test_a_run_from_a_later_row(built, engine, kind, ntrials, nchan):
    """Outputs of a run over rows[j0:] equal outputs j0 .. of the whole run, and both the restatement"""
    delays = _table(kind, ntrials, nchan, seed=5)
    nout = 2 * TILE + 3
    need = dedisp_ref.rows_needed(delays, None, nout)
    rows = dedisp_ref.pooled_rows(need, nchan, seed=9)
    whole = engine.dedisp(rows, delays, nout=nout)
    assert np.array_equal(whole.view(np.uint32), dedisp_ref.dedisp_ref(rows, delays, None, nout).view(np.uint32))
    for j0 in (1, TILE, TILE + 1):
        part = engine.dedisp(rows[j0:], delays)
        assert part.shape == (ntrials, nout - j0) and np.array_equal(part.view(np.uint32), whole[:, j0:].view(np.uint32)), j0
    again = engine.dedisp(rows, delays, nout=nout)
    assert np.array_equal(again.view(np.uint32), whole.view(np.uint32))


def _dispersed_capture(built, t0, n0, nout):
    """A capture of noise with one burst per channel, channel i's where row n0 + d[t0][i] of
    engine.pfbspec(iq, 6, taps, 4, hop=32, shifted=True) is formed, d the third table of DELAY_SETS"""
    k, T, K, hop = 6, 4, 4, 32
    M = 1 << k
    delays = dedisp_ref.delays(*DELAY_SETS[2])
    nrows = dedisp_ref.rows_needed(delays, None, nout)
    nsamples = (nrows * K - 1) * hop + T * M
    b = dedisp_ref.hashed_ints(2 * nsamples, 255, seed=41).reshape(nsamples, 2).astype(np.float64)
    x = (b[:, 0] - 127.5) / 16.0 + 1j * (b[:, 1] - 127.5) / 16.0                   # noise of about +-8
    s = np.arange(K * hop)
    for i in range(M):
        c = (i + M // 2) % M                                                        # shifted rows: position i is channel c
        at = (n0 + int(delays[t0, i])) * K * hop + T * M // 2
        x[at:at + K * hop] += 6.0 * np.exp(2j * np.pi * c * (at + s) / M)
    iq = np.clip(np.rint(np.stack([x.real, x.imag], axis=1) + 128.0), 0, 255).astype(np.uint8)
    return iq, built.pfb_design(k, T), delays, nrows


def test_end_to_end_behind_the_spectrometer(built, engine):
    t0, n0, nout = 20, 100, 300
    iq, taps, delays, nrows = _dispersed_capture(built, t0, n0, nout)
    rows = engine.pfbspec(iq, 6, taps, 4, hop=32, shifted=True)
    assert rows.shape == (nrows, 64) and rows.dtype == np.float32
    want = dedisp_ref.dedisp_ref(rows, delays, None, nout)
    assert np.unravel_index(np.argmax(want), want.shape) == (t0, n0)              # the restatement alone puts it there
    got = engine.dedisp(rows, delays, nout=nout)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    assert np.unravel_index(np.argmax(got), got.shape) == (t0, n0)
    floor = np.median(got)
    print("dedispersed peak %.3g at (t, n) = (%d, %d), %.1f times the median; trial 0 at that n: %.1f times"
          % (got[t0, n0], t0, n0, got[t0, n0] / floor, got[0, n0] / floor))
    assert got[t0, n0] > 1.5 * np.delete(got, t0, axis=0).max()                   # no other trial comes near


def test_capture_and_replay(built):
    """tests/test_graph_gpu.py's pattern for this plan: rtlws_dedisp_run captured on a side stream enqueues nothing,
    replays give the eager launch's bits and the restatement's, twice"""
    import torch
    dev = torch.device("cuda", 0)
    eng = built.Engine(0)
    delays = dedisp_ref.delays(*DELAY_SETS[2])
    ntrials, nchan = delays.shape
    nout = 2 * TILE + 3
    rows_host = dedisp_ref.pooled_rows(dedisp_ref.rows_needed(delays, None, nout), nchan, seed=3)
    rows = torch.from_numpy(rows_host).to(dev)
    out = torch.zeros((ntrials, nout), dtype=torch.float32, device=dev)
    plan = built.DedispPlan(eng, delays)
    assert plan.rows_needed(nout) == rows_host.shape[0]
    g = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        with torch.cuda.graph(g, stream=side):
            plan.run(rows.data_ptr(), nout, out.data_ptr(), stream=built.torch_stream_handle())
    torch.cuda.current_stream().wait_stream(side)
    assert float(out.abs().sum()) == 0.0            # capture enqueued nothing
    g.replay()
    torch.cuda.synchronize()
    first = out.clone()
    out.zero_()
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, first)                  # replays are bit-identical
    want = dedisp_ref.dedisp_ref(rows_host, delays, None, nout)
    assert np.array_equal(first.cpu().numpy().view(np.uint32), want.view(np.uint32))
    eager = torch.zeros_like(out)
    plan.run(rows.data_ptr(), nout, eager.data_ptr(), stream=built.torch_stream_handle())
    torch.cuda.synchronize()
    assert torch.equal(eager, first)
    plan.close()
    eng.close()


# ---- the borders of the plan, signed and special values, the limits, one plan many times ------------------------------

def _bits_differ(got, want):
    """where two float32 arrays differ: bit for bit, but NaN by place and not by payload (the default NaN of the host's
    additions and of the device's differ in the sign bit)"""
    nan = np.isnan(want)
    return np.argwhere((np.isnan(got) != nan) | (~nan & (got.view(np.uint32) != want.view(np.uint32))))


def _assert_bits(got, want, what=None):
    assert got.shape == want.shape and got.dtype == want.dtype == np.float32
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (what, np.argwhere(got.view(np.uint32) != want.view(np.uint32))[:5])


def _plan_of(built, case, delays, mask=None):
    """The geometry of a table of tests/dedisp_form_cases.py is the form its case names (tests/test_dedisp_forms_cpu.py
    says the same without a GPU); -> rows needed"""
    rc, blocks, threads, lds, tile, per, most = built.dedisp_geometry(delays, mask, forms.NOUT)
    want = forms.form(case.plan_spread, case.plan_per)
    assert (rc, threads, tile, per, lds, most) == (0, 256, TILE, case.plan_per, want[1], int(delays.max())), (per, lds, most)
    assert blocks == -(-forms.NOUT // TILE) * -(-case.ntrials // per)
    return forms.NOUT + most


def _border_case(built, engine, case):
    """A table whose plan stands on one side of a border of its forms, 36 positions (a last chunk of one quad behind
    every chunk width), tile_out + 1 outputs: with no mask and with one that keeps the delayed position, bit for bit;
    NaN in the padding columns and behind rows_needed"""
    delays = forms.table(case)
    need = _plan_of(built, case, delays)
    seed = forms.CASES.index(case) + 1
    rows = np.full((need + 3, forms.NCHAN + 4), np.nan, np.float32)
    rows[:need, :forms.NCHAN] = dedisp_ref.pooled_rows(need, forms.NCHAN, seed)
    mask = forms.masks(case)[0][1]
    assert _plan_of(built, case, delays, mask) == need
    for m in (None, mask):
        got = engine.dedisp(rows, delays, m, nout=forms.NOUT, in_stride=forms.NCHAN + 4)
        _assert_bits(got, dedisp_ref.dedisp_ref(rows, delays, m, forms.NOUT), "no mask" if m is None else "masked")


@pytest.mark.parametrize("case", forms.CASES, ids=[forms.case_id(c) for c in forms.CASES])
def test_every_border_of_the_plan(built, engine, case):
    _border_case(built, engine, case)


SIX = pytest.mark.parametrize("case", forms.SIX_FORMS, ids=[forms.case_id(c) for c in forms.SIX_FORMS])


@SIX
def test_signed_and_special_rows(built, engine, case):
    """Terms of both signs: bit for bit, and within the bound on the magnitudes of the f64 sum.  Rows that hold -0.0,
    subnormals, +Inf, -Inf and a quiet NaN (tests/test_dedisp_cpu.py::test_reference_on_signed_and_special_rows says what
    the sums then hold): NaN exactly where the restatement has NaN, every other output bit for bit, so a planted value
    reaches the (t, n) that read it and no other"""
    which = forms.SIX_FORMS.index(case)
    delays = forms.table(case)
    need = _plan_of(built, case, delays)
    rows = dedisp_ref.signed_rows(need, forms.NCHAN, seed=which + 1)
    got = engine.dedisp(rows, delays, nout=forms.NOUT)
    want, want64 = dedisp_ref.dedisp_both(rows, delays, None, forms.NOUT)
    _assert_bits(got, want)
    assert np.all(np.abs(got.astype(np.float64) - want64) <= dedisp_ref.bound(np.abs(rows), delays, None, forms.NOUT))

    rows = dedisp_ref.special_rows(need, forms.NCHAN, seed=which + 1)
    got = engine.dedisp(rows, delays, nout=forms.NOUT)
    with np.errstate(invalid="ignore"):
        want = dedisp_ref.dedisp_ref(rows, delays, None, forms.NOUT)
    differ = _bits_differ(got, want)
    assert not len(differ), (differ[:5], got[tuple(differ[0])], want[tuple(differ[0])])
    assert np.array_equal(np.isfinite(got), np.isfinite(want)) and np.array_equal(np.isnan(got), np.isnan(want))
    assert not (got.view(np.uint32) == 0x80000000).any()


@SIX
def test_masked_positions_are_never_added(built, engine, case):
    """What the mask leaves out may hold anything: with NaN and with -Inf in those columns the outputs are finite and
    bit for bit the restatement of the rows without them, under a random mask, one that leaves out a position of every
    quad and one that leaves out whole quads"""
    which = forms.SIX_FORMS.index(case)
    delays = forms.table(case)
    need = _plan_of(built, case, delays)
    clean = dedisp_ref.signed_rows(need, forms.NCHAN, seed=which + 11)
    for name, mask in forms.masks(case):
        assert _plan_of(built, case, delays, mask) == need
        want = dedisp_ref.dedisp_ref(clean, delays, mask, forms.NOUT)
        assert np.isfinite(want).all()
        for fill in (np.nan, -np.inf):
            rows = clean.copy()
            rows[:, mask == 0] = fill
            got = engine.dedisp(rows, delays, mask, nout=forms.NOUT)
            assert np.isfinite(got).all(), (name, fill)
            _assert_bits(got, want, (name, fill))


def _limit(name):
    """(table, trials a workgroup, LDS bytes, nout) at a limit of the header"""
    t, i = np.arange(4096)[:, None], np.arange(4096)[None, :]
    if name == "every-delay-65535":              # groups of 8 with a base of 65535
        return np.full((9, 8), 65535, np.int32), 8, forms.SMALL_LDS, forms.NOUT
    if name == "0-and-65535-in-one-quad":        # every position by itself
        return np.array([[0, 65535, 0, 65535], [65535, 0, 65535, 65535]], np.int32), 1, forms.SMALL_LDS, forms.NOUT
    if name in ("4096-trials", "4093-trials"):   # 512 groups of 8 that spread 23, the last one of five trials
        return ((t[:int(name[:4])] + i[:, :4]) % 24).astype(np.int32), 8, forms.SMALL_LDS, forms.NOUT
    assert name == "4096-trials-of-4096"
    return ((t + i) % 7).astype(np.int32), 8, forms.SMALL_LDS, 1


@pytest.mark.parametrize("name", ["every-delay-65535", "0-and-65535-in-one-quad", "4096-trials", "4093-trials", "4096-trials-of-4096"])
def test_the_limits(built, engine, name):
    """The largest delay, the most trials and the largest table of the header, launched: bit for bit"""
    delays, per, lds, nout = _limit(name)
    ntrials, nchan = delays.shape
    geo = built.dedisp_geometry(delays, None, nout)
    assert geo == (0, -(-nout // TILE) * -(-ntrials // per), 256, lds, TILE, per, int(delays.max())), geo
    need = dedisp_ref.rows_needed(delays, None, nout)
    assert need * nchan * 4 <= (9 << 18) and (nchan < 4096 or need <= 8)          # about 2 MB of rows at the most
    rows = dedisp_ref.pooled_rows(need, nchan, seed=len(name))
    got = engine.dedisp(rows, delays, nout=nout)
    want = dedisp_ref.dedisp_ref(rows, delays, None, nout)
    assert got.shape == (ntrials, nout)
    _assert_bits(got[-1:], want[-1:], "the last trial")
    _assert_bits(got[8 * ((ntrials - 1) // 8):], want[8 * ((ntrials - 1) // 8):], "the last group")
    _assert_bits(got, want)


def _on_device(torch, host):
    return torch.from_numpy(np.ascontiguousarray(host)).to(torch.device("cuda", 0))


@pytest.mark.parametrize("what", ["every-nout", "a-sub-band", "two-plans-two-streams"])
def test_one_plan_many_runs(built, engine, what):
    """rtlws_dedisp_plan directly, on torch buffers.  One plan at nout 1, tile_out and 2 tile_out + 3 in turn into one
    preset buffer of a wider out_stride: each run is the restatement and leaves the padding as it was.  A plan of 16
    positions over columns 16 .. 31 and 48 .. 63 of a waterfall 64 wide whose other columns hold NaN: the restatement of
    the slice.  Two plans of different tables, shapes and masks alive at once, their runs interleaved on two streams."""
    import torch
    handle = built.torch_stream_handle
    if what == "every-nout":
        case = forms.SIX_FORMS[2]
        delays, mask = forms.table(case), forms.masks(case)[1][1]
        nouts, width = (1, TILE, 2 * TILE + 3), 2 * TILE + 8
        rows_host = dedisp_ref.pooled_rows(dedisp_ref.rows_needed(delays, mask, nouts[-1]), forms.NCHAN, seed=21)
        rows, out = _on_device(torch, rows_host), _on_device(torch, np.full((case.ntrials, width), FILL, np.float32))
        plan = built.DedispPlan(engine, delays, mask)
        for nout in nouts:
            assert plan.rows_needed(nout) == dedisp_ref.rows_needed(delays, mask, nout) <= rows_host.shape[0]
            plan.run(rows.data_ptr(), nout, out.data_ptr(), out_stride=width, stream=handle())
            torch.cuda.synchronize()
            got = out.cpu().numpy()
            _assert_bits(np.ascontiguousarray(got[:, :nout]), dedisp_ref.dedisp_ref(rows_host, delays, mask, nout), nout)
            assert np.all(got[:, nout:].view(np.uint32) == FILL.view(np.uint32)), nout
        plan.close()
    elif what == "a-sub-band":
        delays, mask, nout = dedisp_ref.random_table(9, 16, 30, seed=6), dedisp_ref.random_mask(16, 6), TILE + 1
        assert built.dedisp_geometry(delays, mask, nout)[5] == 8
        need = dedisp_ref.rows_needed(delays, mask, nout)
        wide = np.full((need, 64), np.nan, np.float32)
        for k in (1, 3):
            wide[:, 16 * k:16 * k + 16] = dedisp_ref.pooled_rows(need, 16, seed=30 + k)
        rows, out = _on_device(torch, wide), _on_device(torch, np.zeros((9, nout), np.float32))
        plan = built.DedispPlan(engine, delays, mask)
        for k in (1, 3):
            out.fill_(float(FILL))
            plan.run(rows.data_ptr() + 4 * 16 * k, nout, out.data_ptr(), in_stride=64, stream=handle())
            torch.cuda.synchronize()
            _assert_bits(out.cpu().numpy(), dedisp_ref.dedisp_ref(wide[:, 16 * k:16 * k + 16], delays, mask, nout), k)
        plan.close()
    else:
        nout, reps = TILE + 1, 3
        case = forms.SIX_FORMS[0]
        tables = ((forms.table(case), forms.masks(case)[0][1]), (dedisp_ref.random_table(5, 20, 300, seed=8), None))
        assert [built.dedisp_geometry(d, m, nout)[5] for d, m in tables] == [8, 1]
        hosts = [dedisp_ref.pooled_rows(dedisp_ref.rows_needed(d, m, nout), d.shape[1], seed=40 + j) for j, (d, m) in enumerate(tables)]
        rows = [_on_device(torch, h) for h in hosts]
        outs = [[_on_device(torch, np.full((d.shape[0], nout), FILL, np.float32)) for _ in range(reps)] for d, _ in tables]
        plans = [built.DedispPlan(engine, d, m) for d, m in tables]
        streams = [torch.cuda.Stream(), torch.cuda.Stream()]
        for s in streams:
            s.wait_stream(torch.cuda.current_stream())
        for rep in range(reps):
            for j in (0, 1):
                plans[j].run(rows[j].data_ptr(), nout, outs[j][rep].data_ptr(), stream=handle(streams[j]))
        torch.cuda.synchronize()
        for j, (d, m) in enumerate(tables):
            want = dedisp_ref.dedisp_ref(hosts[j], d, m, nout)
            for rep in range(reps):
                _assert_bits(outs[j][rep].cpu().numpy(), want, (j, rep))
        for plan in plans:
            plan.close()

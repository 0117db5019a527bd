"""GPU suite of include/rtlws_subdedisp.h (librtlws_subdedisp.so) against its numpy restatement (tests/subdedisp_ref.py):
every output and every subband series bit for bit on uint32 views, NaN compared by place.  Every case runs with NaN in the
input stride's padding and in the rows behind rows_needed, the workspace and the outputs preset to a NaN pattern before
the run -- the workspace's pad words, the words behind nout of every trial, behind d_out and behind work_floats still hold
it afterwards -- and every finite case is held to the f64 sums of the same terms within the bound of two chained sums.
The shapes, nout, the nominals, the tables, every form of either stage on both sides of its borders
(tests/subdedisp_form_cases.py), masks, signed and special rows, the identities with rtlws_dedisp_run, the plan's uses
(the subband series, a later row, one plan at three nout, two plans on two streams, a captured graph), the limits, a
run's refusals in the header's order, and a dispersed pulse through the helper's tables."""
import ctypes as C

import numpy as np
import pytest

import dedisp_form_cases as forms1
import dedisp_ref
import subdedisp_form_cases as forms
import subdedisp_ref as ref

pytestmark = pytest.mark.gpu

TILE = 256
FILL = np.array([0x7FC5A5A5], np.uint32).view(np.float32)[0]          # a quiet NaN with a payload: the preset pattern
FILL_BITS = np.uint32(0x7FC5A5A5)


@pytest.fixture(scope="module")
def sd(built):
    import rtlws.subdedisp
    return rtlws.subdedisp


def _bits_differ(got, want):
    """where two float32 arrays differ: bit for bit, but NaN by place and not by payload (the default NaN of the host's
    additions and of the device's differ in the sign bit)"""
    nan = np.isnan(want)
    return np.argwhere((np.isnan(got) != nan) | (~nan & (got.view(np.uint32) != want.view(np.uint32))))


def _assert_bits(got, want, name):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype == np.float32, (name, got.shape, want.shape)
    bad = _bits_differ(got, want)
    assert bad.size == 0, (name, len(bad), bad[:4].tolist(), [(got[tuple(b)], want[tuple(b)]) for b in bad[:4]])


def _check(sd, engine, rows, first, d1, d2, mask=None, nout=None, name=None, finite=True, under=None):
    """rows float32 [>= rows_needed, M] through rtlws.subdedisp.dedisperse the hard way (see the module's text); `under`:
    what lies under the masked positions.  Returns (D, P) of the restatement."""
    first, d1, d2 = np.asarray(first, np.int32), np.asarray(d1, np.int32), np.asarray(d2, np.int32)
    (A, M), (T, B) = d1.shape, d2.shape
    m1, m2 = ref.maxima(d1, d2, mask)
    if nout is None:
        nout = rows.shape[0] - m1 - m2
    need, mid = ref.rows_needed(d1, d2, mask, nout), ref.mid_stride(d1, d2, mask, nout)
    nmid = nout + m2
    assert rows.shape[0] >= need and rows.shape[1] == M
    if nout == 0:                                                 # nothing is read and nothing is written
        out, work = sd.dedisperse(engine, np.full((2, M + 4), np.nan, np.float32), first, d1, d2, mask, nout=0, in_stride=M + 4, out_stride=3, fill=FILL)
        assert out.shape == (3 * T + sd.GUARD,) and work.shape == (sd.GUARD,) and need == mid == 0
        assert np.all(out.view(np.uint32) == FILL_BITS) and np.all(work.view(np.uint32) == FILL_BITS), name
        return None, None
    clean = np.array(rows[:max(need, 1)], np.float32)
    dirty = clean.copy()
    if mask is not None and under is not None:
        dirty[:, np.asarray(mask) == 0] = under
    stride, ostride = M + 4, nout + 3
    padded = np.full((need + 2, stride), np.nan, np.float32)
    padded[:need, :M] = dirty[:need]
    out, work = sd.dedisperse(engine, padded, first, d1, d2, mask, nout=nout, in_stride=stride, out_stride=ostride, fill=FILL)
    D, P, D64 = ref.subdedisp_both(clean, first, d1, d2, mask, nout)
    assert out.shape == (T * ostride + sd.GUARD,) and work.shape == (A * B * mid + sd.GUARD,), (name, out.shape, work.shape)
    got = out[:T * ostride].reshape(T, ostride)
    _assert_bits(got[:, :nout], D, name)
    assert np.all(got[:, nout:].view(np.uint32) == FILL_BITS) and np.all(out[T * ostride:].view(np.uint32) == FILL_BITS), name
    gotp = work[:A * B * mid].reshape(A, B, mid)
    _assert_bits(gotp[:, :, :nmid], P, (name, "P"))
    assert np.all(gotp[:, :, nmid:].view(np.uint32) == FILL_BITS) and np.all(work[A * B * mid:].view(np.uint32) == FILL_BITS), name
    if finite and nout:
        bound = ref.bound(clean, first, d1, d2, mask, nout)
        err = np.abs(D.astype(np.float64) - D64)
        assert np.all(err <= bound), (name, float((err / np.maximum(bound, 1e-300)).max()))
        gerr = np.abs(got[:, :nout].astype(np.float64) - D64)
        assert np.all(gerr <= bound), name
        print("%s: largest share of the f64 bound %.3f" % (name, float((gerr[bound > 0] / bound[bound > 0]).max()) if (bound > 0).any() else 0.0))
    return D, P


def _rows(need, M, seed, signed=False):
    if need * M > 1 << 16:
        return dedisp_ref.pooled_rows(need, M, seed)
    return (dedisp_ref.signed_rows if signed else dedisp_ref.hashed_rows)(need, M, seed)


# ---- shapes, nout, nominals, tables -------------------------------------------------------------------------------

SHAPES = [(4, 1), (8, 2), (16, 1), (16, 4), (48, 4), (64, 2), (72, 2), (96, 2), (256, 64), (1024, 16), (4096, 64), (4096, 1024)]


@pytest.mark.parametrize("M,B", SHAPES, ids=["%dx%d" % s for s in SHAPES])
def test_every_shape(sd, engine, M, B):
    """C = 4 (a border behind every quad), 12 (borders inside a chunk), 32 (on the chunk), 36 (across chunks, a partial last
    chunk), and more subbands than stage 2 stages at once (64, 1024); three nominals of 2, 3 and 1 trials"""
    first = np.array([0, 2, 5, 6], np.int32)
    d1, d2 = ref.random_tables(first, M, B, 20, 10, seed=M + B)
    nout = 257 if M < 4096 else 130
    rows = _rows(ref.rows_needed(d1, d2, None, nout), M, seed=M + B)
    _check(sd, engine, rows, first, d1, d2, None, nout, name=(M, B))


NOUTS = [(1, 10), (255, 10), (256, 10), (257, 10), (513, 10), (250, 10), (257, 3), (0, 10)]


@pytest.mark.parametrize("nout,max_d2", NOUTS, ids=["nout%d-d2max%d" % s for s in NOUTS])
def test_every_nout(sd, engine, nout, max_d2):
    """nout 1, 255, 256, 257 and 513; nmid = 260 across a tile's border while nout = 250 is not, and a multiple of 4 (no
    pad words); nmid = 267 and 260 = 257 + 3 (one pad word and none); nout = 0 does nothing"""
    M, B = 48, 4
    first = np.array([0, 3, 4, 9], np.int32)
    d1, d2 = ref.random_tables(first, M, B, 7, max_d2, seed=nout)
    assert ref.maxima(d1, d2)[1] == max_d2
    rows = _rows(max(ref.rows_needed(d1, d2, None, nout), 1), M, seed=nout + 1)
    _check(sd, engine, rows, first, d1, d2, None, nout, name=(nout, max_d2))


SIZES = (1, 2, 7, 8, 9, 17, 3)


@pytest.mark.parametrize("A", [1, 2, 7, 8, 9, 33])
def test_every_count_of_nominals(sd, engine, A):
    """A nominals of 1, 2, 7, 8, 9, 17 and 3 trials in turn, beginning with another size for every A: a ragged first whose
    stage-2 groups are partial at the end of most nominals, and stage-1 groups partial at the end of the table"""
    sizes = [SIZES[(A + k) % len(SIZES)] for k in range(A)]
    first = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
    M, B = 16, 4
    d1, d2 = ref.random_tables(first, M, B, 6, 9, seed=A)
    got = sd.geometry(first, d1, d2, None, 100)
    assert got == (0,) + forms.geometry(first, d1, d2, None, 100)
    assert got[6] == (8 if max(sizes) >= 5 else 4 if max(sizes) >= 3 else max(sizes)) and got[5] == forms1.cap(A)
    rows = _rows(ref.rows_needed(d1, d2, None, 100), M, seed=A + 50)
    _check(sd, engine, rows, first, d1, d2, None, 100, name=("nominals", A))


TABLES = [(0, 0), (1, 1), (1, 5000), (5, 300), (300, 5), (5000, 1), (300, 300), (5000, 5000)]


@pytest.mark.parametrize("max1,max2", TABLES, ids=["d1to%d-d2to%d" % t for t in TABLES])
def test_random_tables(sd, engine, max1, max2):
    M, B = 48, 4
    first = ref.even_first(11, 4)
    d1, d2 = ref.random_tables(first, M, B, max1, max2, seed=max1 + 3 * max2)
    rows = _rows(ref.rows_needed(d1, d2, None, 300), M, seed=max1 + max2 + 7)
    _check(sd, engine, rows, first, d1, d2, None, 300, name=("random", max1, max2))


@pytest.mark.parametrize("which", range(len(ref.DELAY_SETS)))
def test_the_helper_s_sweeps(sd, engine, which):
    args = ref.DELAY_SETS[which]
    first, d1, d2, smear = sd.delays(*args)
    want = ref.tables(*args)
    assert np.array_equal(first, want[0]) and np.array_equal(d1, want[1]) and np.array_equal(d2, want[2])
    nout = 300
    rows = _rows(ref.rows_needed(d1, d2, None, nout), args[0], seed=which + 60)
    _check(sd, engine, rows, first, d1, d2, None, nout, name=("sweep", which))


# ---- every form of either stage, both sides of every border ---------------------------------------------------------

def _stage1_case(sd, engine, case):
    first, d1, d2 = forms.stage1_case_tables(case)
    got = sd.geometry(first, d1, d2, None, forms.NOUT)
    assert (got[0], got[5], got[3][0]) == (0, case.plan_per, forms1.form(case.plan_spread, case.plan_per)[1])
    rows = _rows(ref.rows_needed(d1, d2, None, forms.NOUT), forms.NCHAN1, seed=case.spread + case.per)
    _check(sd, engine, rows, first, d1, d2, None, forms.NOUT, name=forms1.case_id(case))


def _stage2_case(sd, engine, case):
    first, d1, d2 = forms.stage2_case_tables(case)
    got = sd.geometry(first, d1, d2, None, forms.NOUT)
    assert (got[0], got[6], got[3][1]) == (0, case.plan_per, forms.form2(case.plan_spread, case.plan_per)[0])
    rows = _rows(ref.rows_needed(d1, d2, None, forms.NOUT), forms.NCHAN2, seed=case.spread + case.per)
    _check(sd, engine, rows, first, d1, d2, None, forms.NOUT, name=forms.case2_id(case))


@pytest.mark.parametrize("case", forms.STAGE1_CASES, ids=forms1.case_id)
def test_every_border_of_stage_1(sd, engine, case):
    _stage1_case(sd, engine, case)


@pytest.mark.parametrize("case", forms.STAGE2_CASES, ids=forms.case2_id)
def test_every_border_of_stage_2(sd, engine, case):
    _stage2_case(sd, engine, case)


def _form_tables(stage, k):
    if stage == 1:
        case = forms.STAGE1_FORMS[k]
        return forms.stage1_case_tables(case), forms.NCHAN1, forms1.case_id(case)
    case = forms.STAGE2_FORMS[k]
    return forms.stage2_case_tables(case), forms.NCHAN2, forms.case2_id(case)


FORMS = [(1, k) for k in range(len(forms.STAGE1_FORMS))] + [(2, k) for k in range(len(forms.STAGE2_FORMS))]


@pytest.mark.parametrize("stage,k", FORMS, ids=["stage%d-form%d" % f for f in FORMS])
def test_signed_and_special_rows(sd, engine, stage, k):
    """one table per form of each stage: rows of both signs (held to the f64 bound on the magnitudes), and rows holding -0.0,
    subnormals, +-Inf and NaN (bit for bit, NaN by place)"""
    (first, d1, d2), M, name = _form_tables(stage, k)
    need = ref.rows_needed(d1, d2, None, forms.NOUT)
    _check(sd, engine, dedisp_ref.signed_rows(need, M, seed=k + 11), first, d1, d2, None, forms.NOUT, name=(name, "signed"))
    special = dedisp_ref.special_rows(need, M, seed=k + 23)
    D, P = _check(sd, engine, special, first, d1, d2, None, forms.NOUT, name=(name, "special"), finite=False)
    assert np.isnan(D).any(), name


# ---- masks ------------------------------------------------------------------------------------------------------------

def _masks(M, B):
    C_ = M // B
    one, sub, but_one, zeros, all_but_a_channel = (np.ones(M, np.uint8) for _ in range(5))
    one[C_ + 1] = 0
    sub[C_:2 * C_] = 0
    but_one[:] = 0
    but_one[2 * C_:3 * C_] = 1
    zeros[:] = 0
    all_but_a_channel[C_:2 * C_] = 0
    all_but_a_channel[2 * C_ - 1] = 1
    return (("none", None), ("one channel", one), ("a whole subband", sub), ("every subband but one", but_one), ("all zeros", zeros),
            ("all of a subband but one channel", all_but_a_channel))


@pytest.mark.parametrize("which", range(6), ids=[m[0].replace(" ", "-") for m in _masks(48, 4)])
@pytest.mark.parametrize("under", [np.nan, -np.inf], ids=["nan-under", "neginf-under"])
def test_masked_positions_are_never_added(sd, engine, which, under):
    """NaN or -Inf under every masked position; a masked subband's d2 is 60000, which counts neither in max_d2 nor in what is
    read; its series is +0.0 and is written"""
    M, B = 48, 4
    name, mask = _masks(M, B)[which]
    first = np.array([0, 1, 9, 12], np.int32)
    d1, d2 = ref.random_tables(first, M, B, 12, 30, seed=which + 5)
    if mask is not None:
        gone = ~ref.kept_subbands(M, B, mask)
        d2[:, gone] = 60000
        d1[:, np.asarray(mask) == 0] = 40000
    nout = 270
    rows = _rows(nout + 12 + 30, M, seed=which + 70, signed=True)
    D, P = _check(sd, engine, rows, first, d1, d2, mask, nout, name=("mask", name), under=under)
    if mask is not None:
        gone = ~ref.kept_subbands(M, B, mask)
        assert not P[:, gone].any() and not np.signbit(P[:, gone]).any()
        if not mask.any():
            assert not D.any() and not np.signbit(D).any() and P.shape[2] == nout


# ---- the identities with rtlws_dedisp_run on the device -------------------------------------------------------------

def test_one_subband_is_the_dedispersion_on_the_device(sd, engine):
    """B = 1, d2 = 0, A = T: rtlws_dedisp_run of d1, bit for bit"""
    for M, T, maxd in ((16, 5, 7), (36, 9, 300), (72, 3, 20)):
        d1 = dedisp_ref.random_table(T, M, maxd, seed=M)
        rows = dedisp_ref.signed_rows(300 + maxd, M, seed=M + 1)
        got = sd.dedisperse(engine, rows, np.arange(T + 1), d1, np.zeros((T, 1), np.int32))
        _assert_bits(got, engine.dedisp(rows, d1), (M, T))


def test_exact_sums_do_not_see_the_subbands_on_the_device(sd, engine):
    """A = T, d2 = 0, integer-valued rows whose sums stay below 2^24: rtlws_dedisp_run of d1, bit for bit, for B > 1"""
    for M, B, T in ((16, 4, 3), (48, 4, 5), (72, 2, 4), (72, 18, 9), (256, 64, 2)):
        d1 = dedisp_ref.random_table(T, M, 40, seed=B)
        rows = dedisp_ref.hashed_ints(340 * M, 255, seed=M).astype(np.float32).reshape(340, M)
        got = sd.dedisperse(engine, rows, np.arange(T + 1), d1, np.zeros((T, B), np.int32))
        want = engine.dedisp(rows, d1)
        assert got.shape == want.shape == (T, 300)
        _assert_bits(got, want, (M, B))


# ---- the plan's uses ---------------------------------------------------------------------------------------------------

def _on_device(torch, host):
    return torch.from_numpy(np.ascontiguousarray(host)).to(torch.device("cuda", 0))


def _case():
    M, B = 48, 4
    first = np.array([0, 3, 4, 13], np.int32)
    d1, d2 = ref.random_tables(first, M, B, 25, 40, seed=17)
    return M, B, first, d1, d2


def test_want_subbands_returns_the_series(sd, engine):
    M, B, first, d1, d2 = _case()
    rows = dedisp_ref.signed_rows(400, M, seed=2)
    D, P = sd.dedisperse(engine, rows, first, d1, d2, want_subbands=True)
    wantD, wantP = ref.subdedisp_ref(rows, first, d1, d2, want_subbands=True)
    assert D.shape == (13, 400 - 65) and P.shape == (3, B, ref.mid_stride(d1, d2, None, 335))
    _assert_bits(D, wantD, "D")
    _assert_bits(P[:, :, :wantP.shape[2]], wantP, "P")
    _assert_bits(sd.dedisperse(engine, rows, first, d1, d2), wantD, "D alone")


def test_a_run_from_a_later_row(sd, engine):
    M, B, first, d1, d2 = _case()
    rows = dedisp_ref.signed_rows(700, M, seed=3)
    whole = sd.dedisperse(engine, rows, first, d1, d2)
    _assert_bits(whole, ref.subdedisp_ref(rows, first, d1, d2), "whole")
    for j0 in (1, 255, 300):
        _assert_bits(sd.dedisperse(engine, rows[j0:], first, d1, d2), whole[:, j0:], j0)


def test_one_plan_at_three_nout_into_one_buffer(sd, built, engine):
    import torch
    M, B, first, d1, d2 = _case()
    mask = dedisp_ref.random_mask(M, 3)
    nouts, width = (1, TILE, 2 * TILE + 3), 2 * TILE + 8
    rows_host = dedisp_ref.signed_rows(ref.rows_needed(d1, d2, mask, nouts[-1]), M, seed=21)
    plan = sd.SubdedispPlan(engine, first, d1, d2, mask)
    rows, out = _on_device(torch, rows_host), _on_device(torch, np.full((13, width), FILL, np.float32))
    work = _on_device(torch, np.full(plan.work_floats(nouts[-1]) + 8, FILL, np.float32))
    for nout in nouts:
        assert plan.rows_needed(nout) == ref.rows_needed(d1, d2, mask, nout) and plan.mid_stride(nout) == ref.mid_stride(d1, d2, mask, nout)
        assert plan.work_floats(nout) == 3 * B * plan.mid_stride(nout)
        plan.run(rows.data_ptr(), nout, work.data_ptr(), out.data_ptr(), out_stride=width, stream=built.torch_stream_handle())
        torch.cuda.synchronize()
        got = out.cpu().numpy()
        _assert_bits(got[:, :nout], ref.subdedisp_ref(rows_host, first, d1, d2, mask, nout), nout)
        assert np.all(got[:, nout:].view(np.uint32) == FILL_BITS), nout
    assert np.all(work.cpu().numpy()[plan.work_floats(nouts[-1]):].view(np.uint32) == FILL_BITS)
    plan.close()


def test_two_plans_on_two_streams(sd, built, engine):
    import torch
    nout, reps = TILE + 1, 3
    t1, t2 = forms.stage2_case_tables(forms.STAGE2_FORMS[1]), forms.stage1_case_tables(forms.STAGE1_FORMS[4])
    tables = (t1, t2)
    assert [sd.geometry(*t, None, nout)[5:7] for t in tables] == [(forms1.cap(1), 8), (1, 2)]
    hosts = [dedisp_ref.pooled_rows(ref.rows_needed(t[1], t[2], None, nout), t[1].shape[1], seed=40 + j) for j, t in enumerate(tables)]
    plans = [sd.SubdedispPlan(engine, *t) for t in tables]
    rows = [_on_device(torch, h) for h in hosts]
    outs = [[_on_device(torch, np.full((t[2].shape[0], nout), FILL, np.float32)) for _ in range(reps)] for t in tables]
    works = [[_on_device(torch, np.full(p.work_floats(nout), FILL, np.float32)) for _ in range(reps)] for p in plans]
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    for s in streams:
        s.wait_stream(torch.cuda.current_stream())
    for rep in range(reps):
        for j in (0, 1):
            plans[j].run(rows[j].data_ptr(), nout, works[j][rep].data_ptr(), outs[j][rep].data_ptr(), stream=built.torch_stream_handle(streams[j]))
    torch.cuda.synchronize()
    for j, t in enumerate(tables):
        want = ref.subdedisp_ref(hosts[j], *t, None, nout)
        for rep in range(reps):
            _assert_bits(outs[j][rep].cpu().numpy(), want, (j, rep))
    for plan in plans:
        plan.close()


def test_capture_and_replay(sd, built):
    """tests/test_graph_gpu.py's pattern for this plan: the two launches of rtlws_subdedisp_run captured on a side stream
    enqueue nothing; replays give the eager run's bits and the restatement's, twice.  The process's queue settings are as
    they were: nothing here touches them"""
    import torch
    eng = built.Engine(0)
    args = ref.DELAY_SETS[2]
    first, d1, d2, _ = sd.delays(*args)
    nout = 2 * TILE + 3
    rows_host = dedisp_ref.pooled_rows(ref.rows_needed(d1, d2, None, nout), args[0], seed=3)
    plan = sd.SubdedispPlan(eng, first, d1, d2)
    assert plan.rows_needed(nout) == rows_host.shape[0]
    rows = _on_device(torch, rows_host)
    out = torch.zeros((args[6], nout), dtype=torch.float32, device=rows.device)
    work = torch.zeros(plan.work_floats(nout), dtype=torch.float32, device=rows.device)
    g = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        with torch.cuda.graph(g, stream=side):
            plan.run(rows.data_ptr(), nout, work.data_ptr(), out.data_ptr(), stream=built.torch_stream_handle())
    torch.cuda.current_stream().wait_stream(side)
    assert float(out.abs().sum()) == 0.0 and float(work.abs().sum()) == 0.0            # capture enqueued nothing
    g.replay()
    torch.cuda.synchronize()
    once, once_work = out.clone(), work.clone()
    out.zero_()
    work.zero_()
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, once) and torch.equal(work, once_work)                     # replays are bit-identical
    wantD, wantP = ref.subdedisp_ref(rows_host, first, d1, d2, None, nout, want_subbands=True)
    _assert_bits(once.cpu().numpy(), wantD, "replay")
    mid = plan.mid_stride(nout)
    _assert_bits(once_work.cpu().numpy().reshape(-1, args[1], mid)[:, :, :wantP.shape[2]], wantP, "replay, P")
    eager, eager_work = torch.zeros_like(out), torch.zeros_like(work)
    plan.run(rows.data_ptr(), nout, eager_work.data_ptr(), eager.data_ptr(), stream=built.torch_stream_handle())
    torch.cuda.synchronize()
    assert torch.equal(eager, once)
    plan.close()
    eng.close()


# ---- the limits ----------------------------------------------------------------------------------------------------------

LIMITS = ["4096-nominals-of-one-trial", "4096-trials-of-one-nominal", "every-d1-65535", "every-d2-65535", "0-and-65535-in-one-quad", "4096x1024-nine-trials"]


@pytest.mark.parametrize("name", LIMITS)
def test_the_limits(sd, engine, name):
    if name == "4096-nominals-of-one-trial":
        M, B, nout = 64, 4, 10
        first = np.arange(4097, dtype=np.int32)
        d1, d2 = ref.random_tables(first, M, B, 5, 6, seed=1)
    elif name == "4096-trials-of-one-nominal":
        M, B, nout = 64, 4, 10
        first = np.array([0, 4096], np.int32)
        d1, d2 = ref.random_tables(first, M, B, 5, 6, seed=2)
    elif name == "every-d1-65535":
        M, B, nout = 8, 2, 1
        first = np.array([0, 1, 3], np.int32)
        d1, d2 = np.full((2, M), 65535, np.int32), np.zeros((3, B), np.int32)
    elif name == "every-d2-65535":
        M, B, nout = 8, 2, 1
        first = np.array([0, 1, 3], np.int32)
        d1, d2 = np.zeros((2, M), np.int32), np.full((3, B), 65535, np.int32)
    elif name == "0-and-65535-in-one-quad":
        M, B, nout = 8, 2, 3
        first = np.array([0, 2, 3], np.int32)
        d1, d2 = np.zeros((2, M), np.int32), np.zeros((3, B), np.int32)
        d1[0, 1], d1[1, 6], d2[0, 1], d2[1, 0] = 65535, 65535, 65535, 65535
        assert sd.geometry(first, d1, d2, None, nout)[5:7] == (1, 1) and forms.plan(first, d1, d2)[0] == (1, forms.SMALL_LDS)
    else:
        M, B, nout = 4096, 1024, 40
        first = np.array([0, 9], np.int32)
        d1, d2 = ref.random_tables(first, M, B, 3, 9, seed=4)
    assert sd.supported(M, B, len(first) - 1, int(first[-1])) == 1
    rows = dedisp_ref.pooled_rows(ref.rows_needed(d1, d2, None, nout), M, seed=len(name))
    _check(sd, engine, rows, first, d1, d2, None, nout, name=name)


# ---- a run's refusals ------------------------------------------------------------------------------------------------------

def test_every_refusal_of_a_run_in_the_header_s_order(sd, engine):
    M, B, first, d1, d2 = _case()
    plan = sd.SubdedispPlan(engine, first, d1, d2)
    nout = 16
    rows, work, out = engine.alloc(4 * M * plan.rows_needed(nout)), engine.alloc(4 * plan.work_floats(nout)), engine.alloc(4 * 13 * nout)
    L = sd.lib()
    run = lambda d_rows, in_stride, n, d_work, d_out, out_stride, p=plan.h: L.rtlws_subdedisp_run(p, d_rows, in_stride, n, d_work, d_out, out_stride, None)
    r, w, o = rows.ptr, work.ptr, out.ptr
    # each line breaks the rules behind it as well
    for args, text in (((r + 4, 2, -1, w + 2, o + 2, -2), "nout must be >= 0"), ((r + 4, 2, nout, w + 2, o + 2, 1), "in_stride must be >= nchan"),
                       ((r + 4, 6, nout, w + 2, o + 2, 1), "in_stride must be a multiple of 4"), ((r + 4, 8, nout, w + 2, o + 2, nout - 1), "out_stride must be >= nout"),
                       ((None, 8, nout, w + 2, o + 2, nout), "null pointer"), ((r + 4, 8, nout, None, o + 2, nout), "null pointer"),
                       ((r + 4, 8, nout, w + 2, None, nout), "null pointer"), ((r + 4, 8, nout, w + 2, o + 2, nout), "d_rows must be 16-byte aligned"),
                       ((r, 8, nout, w + 2, o + 2, nout), "d_work must be 4-byte aligned"), ((r, 8, nout, w, o + 2, nout), "d_out must be 4-byte aligned")):
        assert run(*args) == -1 and sd.last_error() == "rtlws_subdedisp_run: " + text, (args, sd.last_error())
        assert run(*args, p=None) == -1 and sd.last_error() == "rtlws_subdedisp_run: " + text, (args, sd.last_error())
    assert run(r, 8, nout, w, o, nout, p=None) == -1 and sd.last_error().startswith("rtlws_subdedisp_run: null plan")
    assert run(r, 8, nout, w, o, nout) == -1 and sd.last_error() == "rtlws_subdedisp_run: in_stride must be >= nchan"        # the plan's 48
    assert run(r, M - 4, (1 << 40), w, o, 1 << 40) == -1 and sd.last_error() == "rtlws_subdedisp_run: in_stride must be >= nchan"
    assert run(r, M, (1 << 40), w, o, 1 << 40) == -1 and sd.last_error() == "rtlws_subdedisp_run: more workgroups than one grid holds"
    assert run(None, M, 0, None, None, 0) == 0 and sd.last_error() == ""                                                  # nout 0 does nothing
    assert run(r, M, nout, w, o, nout) == 0 and sd.last_error() == ""
    engine.sync()
    plan.close()
    for b in (rows, work, out):
        b.free()


# ---- end to end ------------------------------------------------------------------------------------------------------------

def test_a_dispersed_pulse_through_the_helper_s_tables(sd, built, engine):
    """(256, 16): the maximum of D lies at the trial the pulse was swept at and within 1 row of the injection; the
    restatement alone says the same, and neighbouring trials' tables differ"""
    k = ref.PULSE
    rows, t0, row0 = ref.pulse_waterfall()
    first, d1, d2, smear = sd.delays(*ref.pulse_sweep())
    full = built.dedisp_delays(*ref.pulse_sweep()[:1], *ref.pulse_sweep()[2:9])
    assert np.array_equal(full, dedisp_ref.delays(*ref.pulse_sweep()[:1], *ref.pulse_sweep()[2:9]))      # what swept the pulse
    assert all(not np.array_equal(d2[t], d2[t + 1]) for t in range(k["ntrials"] - 1)) and all(not np.array_equal(d1[a], d1[a + 1]) for a in range(len(first) - 2))
    assert first[2] <= t0 < first[3] and t0 - first[2] == k["per_nominal"] // 2
    want = ref.subdedisp_ref(rows, first, d1, d2)
    for what, D in (("restatement", want), ("device", sd.dedisperse(engine, rows, first, d1, d2))):
        t, n = np.unravel_index(int(np.argmax(D)), D.shape)
        print("%s: smear_rows %.2f, maximum %.0f of %d at trial %d (swept at %d), row %d (injected at %d .. %d); the next best trial %.0f"
              % (what, smear, D[t, n], k["nchan"], t, t0, n, row0, row0 + 2, np.delete(D, t, axis=0).max()))
        assert t == t0 and abs(int(n) - (row0 + 1)) <= 1, (what, t, n)
    _assert_bits(sd.dedisperse(engine, rows, first, d1, d2), want, "end to end")

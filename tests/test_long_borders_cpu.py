"""tests/long_border_cases.py held to its conditions: the tables reach every pass length, kind and group border they
claim (and fail without any one entry), the group plan restates rtlws_long_open, the accuracy metric separates a sound
f64 transform from one with a 1e-13 twiddle defect, and the numpy restatement has the exact relations the GPU suite
asks of the kernels.  No GPU."""
import copy

import numpy as np
import pytest

import long_border_cases as bc
import long_kernels as lk
from test_long_cpu import four_step

LENGTHS = {128, 256, 512, 1024}


def conditions(t):
    """Every condition on the tables; raises AssertionError at the first that does not hold."""
    # a: every (N1, N2) pair
    assert {(bc.n1(m), bc.n2(m)) for m in t["accuracy"]} == {(bc.n1(m), bc.n2(m)) for m in lk.SIZES}
    assert len({(bc.n1(m), bc.n2(m)) for m in lk.SIZES}) == 7
    # b, c: pass B's stores and sums at every N2
    assert {bc.n2(m) for m in t["stores"]} == LENGTHS and {bc.n2(m) for m in t["k_sums"]} == LENGTHS
    # d: both passes at every length
    assert {bc.n1(m) for m in t["scaling"]} == LENGTHS and {bc.n2(m) for m in t["scaling"]} == LENGTHS
    # e: the conversion in pass A at the widest and the narrowest tile
    assert {bc.pass_a_columns(m) for m in t["extremes"]} == {64, 8}
    # b - e together reach every N1 as well
    assert {bc.n1(m) for k in ("stores", "k_sums", "scaling", "extremes") for m in t[k]} == LENGTHS
    # f: three frames through an identity and a permuted pass A grid
    assert {bc.grid_is_permuted(m, 3) for m in t["own_row"]} == {False, True}
    # g: identity grids of both residues, permuted grids at two sizes, the largest among them
    grids = [bc.pass_a_grid(m, F) for m, F in t["place"]]
    assert {g % 8 for g in grids if g % 8} == {6, 2}
    assert len({m for m, F in t["place"] if bc.grid_is_permuted(m, F)}) >= 2
    assert max(m for m, F in t["place"]) == 20 and all(1 <= F <= 5 for m, F in t["place"])
    # h: every sample size crosses a group border under two row sizes, and every row size under two sample sizes
    for kind in bc.INPUTS:
        assert len({r for i, r in t["group_kinds"] if i == kind}) == 2, kind
    for kind in bc.ROWS:
        assert len({i for i, r in t["group_kinds"] if r == kind}) == 2, kind
    plans = {mf: bc.group_plan(bc.GROUP_FRAMES, 1 << bc.GROUP_M, bc.GROUP_K, mf) for mf in t["group_max_frames"]}
    assert [bc.GROUP_FRAMES] in plans.values()                                          # the one-group run
    assert any(len(p) > 1 and p[-1] < p[0] for mf, p in plans.items() if mf % bc.GROUP_K == 0)   # a ragged last group
    assert any(mf % bc.GROUP_K and p[0] > mf > bc.GROUP_K for mf, p in plans.items())   # max_frames above a row, no multiple of K
    assert [bc.GROUP_K] * (bc.GROUP_FRAMES // bc.GROUP_K) in plans.values()             # one row per group
    # i: every kind; pass A at T = 64 and T = 8; pass B at T = 8 under both row kinds whose runs of T items are
    # shorter than a 128-byte line there (8 and 32 bytes)
    assert {i for m, i, r in t["outside"]} == set(bc.INPUTS) and {r for m, i, r in t["outside"]} == set(bc.ROWS)
    assert {bc.pass_a_columns(m) for m, i, r in t["outside"]} >= {64, 8}
    assert {r for m, i, r in t["outside"] if bc.pass_b_columns(m) == 8} == {"u8", "f32"}
    assert len({m for m, i, r in t["outside"]}) >= 4


def test_the_tables_hold_what_the_suite_asks_for():
    conditions(bc.tables())
    assert bc.PASS_A_FIRST_M == tuple(min(m for m in lk.SIZES if bc.n1(m) == L) for L in sorted(LENGTHS))
    assert bc.PASS_B_FIRST_M == tuple(min(m for m in lk.SIZES if bc.n2(m) == L) for L in sorted(LENGTHS))
    assert set(bc.PASS_A_FIRST_M) <= set(bc.SCALING_M)
    assert [bc.pass_a_grid(m, F) for m, F in bc.PLACE_CASES] == [6, 10, 16, 256]
    assert [bc.pass_a_grid(m, 3) for m in bc.OWN_ROW_M] == [6, 24]
    assert (bc.pass_a_columns(14), bc.pass_a_columns(19)) == (64, 8)
    assert sorted(bc.STORES_GAIN) == list(bc.STORES_M) and sorted(bc.STORES_GAIN.values()) == [-25, 0, 9, 100]
    assert all(lk.log2_n1(m) + lk.log2_n2(m) == m for m in lk.SIZES)
    assert (bc.OUTSIDE_GUARD + bc.OUTSIDE_SKEW) % 16 == 8               # rtlws_long_run's minimum alignment of d_in, no more


def test_deleting_any_entry_breaks_a_condition():
    whole = bc.tables()
    n = 0
    for name, table in whole.items():
        for i in range(len(table)):
            t = copy.deepcopy(whole)
            del t[name][i]
            try:
                conditions(t)
            except AssertionError:
                pass
            else:
                pytest.fail("the conditions hold without %s[%d] = %r" % (name, i, table[i]))
            n += 1
    assert n == sum(len(v) for v in whole.values()) == 7 + 4 + 4 + 5 + 2 + 2 + 4 + 6 + 4 + 5


def test_group_plan_restates_rtlws_long_open():
    N, K, F = 1 << bc.GROUP_M, bc.GROUP_K, bc.GROUP_FRAMES
    assert bc.group_plan(F, N, K, 10) == [10]
    assert bc.group_plan(F, N, K, 4) == [4, 4, 2]
    assert bc.group_plan(F, N, K, 3) == [4, 4, 2] and bc.frames_in_flight(N, K, 3) == 4        # rounded up to whole rows
    assert bc.group_plan(F, N, K, 1) == [2] * 5
    assert bc.frames_in_flight(N, K, 0) == K and bc.frames_in_flight(N, K, -5) == K           # < 1 means one row
    # the figures tests/test_long_gpu.py::test_grouping_and_arguments reads from the library
    assert 16 * N * bc.frames_in_flight(N, 2, 4) == 4 * 16 * N
    assert 16 * (1 << 20) * bc.frames_in_flight(1 << 20, 3, 1000) == 63 * (16 << 20)
    assert bc.frames_in_flight(1 << 20, 100, 1) == 100                                       # one row's frames above the cap
    assert bc.group_plan(12, N, 2, 4) == [4, 4, 4]


def test_long_double_is_wider_than_double():
    """What the truth of the accuracy tests rests on; the GPU test asserts it too and fails, not skips, without it."""
    assert np.finfo(np.longdouble).eps <= 2.0 ** -63
    x = np.random.default_rng(1).standard_normal(4096).astype(np.clongdouble)
    X = np.fft.fft(x)
    assert X.dtype == np.clongdouble
    assert np.abs(X - np.fft.fft(x.astype(np.complex128))).max() > 0    # not the f64 transform widened


def test_rows_from_powers_is_the_reference_row(oracle):
    from rtlws import synth
    N, K = 1 << 14, 3
    iq = synth.tone_noise_iq(2 * K, N, seed=8)
    ref = oracle.batch_spectra_u8(iq, N, K=K, nthreads=8)
    t = bc.truth_rows(iq, "cu8", K)
    assert t.dtype == np.longdouble and t.shape == ref.shape
    assert np.abs(t.astype(np.float64) - ref).max() <= 1e-12 * ref.max()
    for slot in (N // 2, N // 2 - 1):
        assert (np.abs(t[:, slot].astype(np.float64) - ref[:, slot]) <= 1e-13 * ref[:, slot]).all()
    assert np.abs(bc.four_step_rows(iq, "cu8", K) - ref).max() <= 1e-12 * ref.max()
    assert bc.e_metric(ref, ref) == 0.0 and abs(bc.e_metric(ref * (1 + 1e-6), ref) / (1e-6 * np.sqrt(np.mean(ref ** 2)) / ref.mean()) - 1) < 1e-6


def _oracle_row(oracle, frames, input, N):
    add = {"cu8": oracle.spectrum_add_cmplx_u8, "cs32": oracle.spectrum_add_cmplx_s32, "rf32": oracle.spectrum_add_real_f32}[input]
    row = np.zeros(N)
    assert add(N, frames[0], row) == 0
    return row


def _four_step_with_twl_angles_times(x, scale):
    """test_long_cpu.four_step with every angle of the low twiddle table multiplied by `scale` before the rounding"""
    two_pi = np.longdouble("6.283185307179586476925286766559005768")
    a = -two_pi * np.arange(1024, dtype=np.longdouble) / np.longdouble(x.size) * np.longdouble(scale)
    return four_step(x, np.cos(a).astype(np.float64) + 1j * np.sin(a).astype(np.float64))


@pytest.mark.parametrize("m", bc.ACCURACY_M)
def test_the_two_cpu_transforms_bracket_the_bound(oracle, m):
    """On the frames of test_accuracy_against_long_double the oracle's e and the restatement's lie within 1.5x of each
    other for the three inputs: two independent f64 transforms agree on what an f64 transform's error is, so twice the
    larger of them is a bound that means something.  A twiddle table off by 1e-13 relative lies far outside it."""
    N = 1 << m
    frames = bc.accuracy_frames(m)
    es = {}
    for input in bc.INPUTS:
        truth = bc.truth_rows(frames[input], input)[0]
        eo =bc.e_metric(_oracle_row(oracle, frames[input], input, N), truth)
        ef = bc.e_metric(bc.four_step_rows(frames[input], input)[0], truth)
        print("m = %d %s: e(oracle) %.3g, e(four_step) %.3g, ratio %.3f" % (m, input, eo, ef, ef / eo))
        assert 0 < eo < 1e-15 and 0 < ef < 1e-15
        assert max(eo, ef) <= 1.5 * min(eo, ef), (m, input)
        es[input] = (eo, ef)
    # What the bound sees, in the restatement: twl built from angles times (1 + d).  The angles reach 2 pi 1023 / N,
    # so d = 1e-13 is a phase error of at most 3.9e-14 at m = 14 and 6.1e-16 at m = 20: there its rms, 3.5e-16, is below
    # the transform's own e of 5e-16, to which it adds in quadrature, and no f64 measurement can tell it from a sound
    # table; d = 1e-12 is seen at every m.
    bound = 2 * max(es["cu8"])
    truth = bc.truth_rows(frames["cu8"], "cu8")[0]
    x = bc.convert(frames["cu8"], "cu8")[0]
    for d, seen in ((1e-13, True if m <= 17 else False if m >= 19 else None), (1e-12, True)):   # m = 18: at the bound
        X = _four_step_with_twl_angles_times(x, 1 + d)
        e = bc.e_metric(bc.rows_from_powers((X.real ** 2 + X.imag ** 2)[None], 1)[0], truth)
        print("m = %d: twl angles times (1 + %g): e %.3g, %.2f of the bound" % (m, d, e, e / bound))
        assert seen is None or (e > bound) == seen, (m, d)
    assert _four_step_with_twl_angles_times(x, 1).tobytes() == four_step(x).tobytes()


def test_the_restatement_adds_k1_rows_in_order():
    """Relation c of the GPU suite, of rows_from_powers over four_step"""
    from rtlws import synth
    N = 1 << 14
    iq = synth.tone_noise_iq(3, N, seed=54)
    p = bc.four_step_rows(iq, "cu8", 1)
    s = bc.four_step_rows(iq, "cu8", 3)
    keep = np.arange(N) != N // 2
    assert np.array_equal(s[0][keep].view(np.uint64), ((p[0] + p[1]) + p[2])[keep].view(np.uint64))
    assert np.array_equal(p[:, N // 2].view(np.uint64), p[:, N // 2 - 1].view(np.uint64))
    assert len(set(p[:, N // 2].tolist())) == 3


@pytest.mark.parametrize("m", [14, 15])
def test_power_of_two_scaling_commutes_with_the_restatement(m):
    """Relation d: four_step of frames times 2^e is four_step times 2^e, bit for bit -- every operation is a
    multiplication by a table value, an addition or a square, and nothing overflows or goes subnormal."""
    N = 1 << m
    rng = np.random.default_rng(m + 1)
    f32 = rng.standard_normal(N).astype(np.float32)
    base = four_step(f32.astype(np.complex128))
    for e in (40, -40):
        scaled = f32 * np.float32(2.0 ** e)
        assert np.array_equal(scaled.astype(np.float64), f32.astype(np.float64) * 2.0 ** e)
        got = four_step(scaled.astype(np.complex128))
        assert np.array_equal(got.view(np.uint64), (base * 2.0 ** e).view(np.uint64)), e
    s32 = rng.integers(-(1 << 20), (1 << 20) + 1, size=(1, N, 2), dtype=np.int32)
    a = bc.four_step_rows(s32, "cs32")
    b = bc.four_step_rows(s32 << 8, "cs32")
    assert np.array_equal(b.view(np.uint64), (a * 2.0 ** 16).view(np.uint64))

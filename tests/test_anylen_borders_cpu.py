"""tests/anylen_border_cases.py held to its conditions: every listed length is where its reason says it is, the list
with the lengths run before reaches both sides of every border of pass 4's indexing, and the two numpy restatements
(and, at the small lengths, the oracle) agree at each of them, so the GPU suite's reference is good there.  No GPU."""
import numpy as np
import pytest

import anylen_border_cases as bc
import anylen_kernels as ak
import anylen_ref
import long_kernels as lk
from helpers import rel_err, EPS_STRICT, TOL_F64

TOL_REFERENCE = 1e-11          # what test_anylen_cpu.py gives the numpy reference: a tenth of TOL_F64


def test_the_list_holds_what_the_suite_asks_for():
    assert len(set(bc.LENGTHS)) == len(bc.LENGTHS) == 6 + 1 + 3 * len(bc.SIZES) and bc.SIZES == tuple(range(15, 21))
    assert all(reason for _, reason in bc.CASES)
    assert set(bc.LENGTHS) >= {63, 64, 65, 127, 128, 129, 8193}
    for m in bc.SIZES:
        assert {(1 << (m - 1)) - 1, 1 << (m - 1), bc.INNER_N[m]} <= set(bc.LENGTHS)
    assert bc.POW2 == tuple(1 << j for j in range(14, 20))
    before = set(ak.SMALL_N) | set(ak.PARITY_N.values())
    assert not before & set(bc.LENGTHS)                               # every one is new to the device
    assert [bc.frames_for(N) for N in (63, 65536, 65535, 91928, 1 << 19)] == [6, 6, 6, 3, 3]


def test_geometry_restates_the_split():
    for N in bc.LENGTHS:
        g = bc.geometry(N)
        assert g["m"] == anylen_ref.conv_log2(N) == ak.conv_log2(N)
        assert g["N1"] * g["N2"] == 1 << g["m"] and g["N1"] == 1 << lk.log2_n1(g["m"]) and g["N2"] == 1 << lk.log2_n2(g["m"])
        assert g["T"] * g["N2"] == 8192 and g["tiles"] * g["T"] == g["N1"]
        # the owner of bin N - 1 by enumeration of j = k1 + N1 k2
        k1 = (N - 1) % g["N1"]
        assert k1 + g["N1"] * ((N - 1) // g["N1"]) == N - 1
        assert (g["owner_tile"], g["owner_col"]) == divmod(k1, g["T"])
        # the run of T consecutive j that holds j = N/2 is cut unless N/2 is its first element
        assert g["wrap_cuts"] == ((N // 2) % g["T"] != 0) and g["wrap_in_run"] == (N // 2) % g["T"]
        assert g["last_run_kept"] == N - (N // g["T"]) * g["T"]
        assert g["tile_returns"] == any(k1_0 >= N for k1_0 in range(0, g["N1"], g["T"]))


def test_convolution_sizes_and_their_borders():
    for N in bc.LENGTHS:
        m = anylen_ref.conv_log2(N)
        assert (1 << m) >= 2 * N - 1 and (m == 14 or (1 << (m - 1)) < 2 * N - 1)
    assert [anylen_ref.conv_log2(N) for N in (63, 64, 65, 127, 128, 129)] == [14] * 6
    assert anylen_ref.conv_log2(8192) == 14 and anylen_ref.conv_log2(8193) == 15
    for m in bc.SIZES:
        assert anylen_ref.conv_log2((1 << (m - 1)) - 1) == m and anylen_ref.conv_log2(1 << (m - 1)) == m
        assert anylen_ref.conv_log2(bc.INNER_N[m]) == m
        assert anylen_ref.conv_log2((1 << (m - 1)) + 1) == m + 1
        N = 1 << (m - 1)                                               # the least slack: M = 2 N
        assert (1 << m) - N + 1 == (N - 1) + 2                         # b's wrapped half begins one element after a's last
    N = (1 << 19) - 1
    assert (N - 1) ** 2 > 1 << 37 and (N - 1) ** 2 < 1 << 38          # the chirp table's n^2, 64-bit on both sides


def test_inner_lengths_are_inner():
    for m, N in bc.INNER_N.items():
        g = bc.geometry(N)
        assert g["m"] == m
        assert g["owner_col"] not in (0, g["T"] - 1), N
        assert g["owner_tile"] not in (0, g["tiles"] - 1), N
        assert g["wrap_in_run"] not in (0, g["T"] - 1), N
        assert g["last_run_kept"] not in (0, 1), N
    assert sorted(m for m, N in bc.INNER_N.items() if N % 2) == [15, 17, 19]
    assert sorted(m for m, N in bc.INNER_N.items() if N % 2 == 0) == [16, 18, 20]


@pytest.mark.parametrize("m", bc.SIZES)
def test_every_border_of_a_convolution_size_is_reached(m):
    """The new lengths and the ones run before (anylen_kernels.PARITY_N), together, per M = 2^m above the smallest: the
    owner of bin N - 1 in column 0, in column T - 1 and in an inner column, and in a tile that is not the first; a
    wrap that cuts a run and one that does not; odd and even N.  (At M = 2^15 column 0 is 8193's.)"""
    ns = [N for N in bc.LENGTHS + tuple(ak.PARITY_N.values()) if anylen_ref.conv_log2(N) == m]
    gs = [bc.geometry(N) for N in ns]
    T = gs[0]["T"]
    cols = {g["owner_col"] for g in gs}
    assert 0 in cols and T - 1 in cols and any(0 < c < T - 1 for c in cols)
    assert any(g["owner_tile"] != 0 for g in gs) and any(0 < g["owner_tile"] < g["tiles"] - 1 for g in gs)
    assert {g["wrap_cuts"] for g in gs} == {False, True}
    assert {N % 2 for N in ns} == {0, 1}
    assert {g["last_run_kept"] for g in gs} >= {0, 1, T - 1}            # whole, one element kept, one lost


def test_the_smallest_convolution_size_around_its_borders():
    small = [N for N in bc.LENGTHS if anylen_ref.conv_log2(N) == 14]
    g = bc.geometry(small[0])
    assert (g["N1"], g["T"], g["tiles"]) == (128, 64, 2)
    edge = g["N1"] - g["T"]                                            # the last N whose second tile returns whole
    assert {edge - 1, edge, edge + 1} <= set(small)
    assert [bc.geometry(N)["tile_returns"] for N in (edge - 1, edge, edge + 1)] == [True, True, False]
    assert {g["N1"] - 1, g["N1"], g["N1"] + 1} <= set(small)
    # no length above N1 - T makes a tile return, at any size: the border is reachable at M = 2^14 only
    assert not any(bc.geometry(N)["tile_returns"] for N in bc.LENGTHS if N > edge)


@pytest.fixture(scope="module")
def frames():
    """N -> three random cu8 frames, made once"""
    made = {}

    def get(N):
        if N not in made:
            made[N] = np.random.default_rng(N).integers(0, 256, size=(3, N, 2), dtype=np.uint8)
            made[N].setflags(write=False)
        return made[N]
    return get


@pytest.mark.parametrize("N", bc.LENGTHS)
def test_the_two_restatements_agree_at_every_length(frames, N):
    """np.fft.fft with the row rules against Bluestein's algorithm as the kernels compute it, K = 3: the reference
    the GPU suite uses above 2048 points is good at every border (the least slack of the wrapped table b, the first
    and last length of a size, n^2 above 2^37)."""
    iq = frames(N)
    ref = anylen_ref.rows(iq, N, 3)
    e = rel_err(anylen_ref.bluestein_rows(iq, N, 3), ref, EPS_STRICT).max()
    print("N = %d: Bluestein restated against np.fft.fft, max strict rel err %.3g" % (N, e))
    assert e <= TOL_REFERENCE


@pytest.mark.parametrize("N", [N for N in bc.LENGTHS if N <= 129])
def test_the_oracle_agrees_at_the_small_lengths(frames, oracle, N):
    iq = frames(N)
    want = oracle.batch_spectra_u8(iq, N, K=3, nthreads=8)
    e = rel_err(anylen_ref.rows(iq, N, 3), want, EPS_STRICT).max()
    eb = rel_err(anylen_ref.bluestein_rows(iq, N, 3), want, EPS_STRICT).max()
    print("N = %d against the oracle: np.fft.fft %.3g, Bluestein restated %.3g" % (N, e, eb))
    assert e <= TOL_REFERENCE and eb <= TOL_F64
    i0 = N - N // 2
    for slot in (i0, i0 - 1):
        assert abs(anylen_ref.rows(iq, N, 3)[:, slot] - want[:, slot]).max() <= 1e-13 * want[:, slot].max()


def test_power_of_two_scaling_commutes_with_the_restatement():
    """What test_power_of_two_scaling_is_exact asks of the device holds of the algorithm in numpy: every operation is
    a multiplication by a table value, an addition or a square, and none overflows or goes subnormal."""
    for N in (bc.INNER_N[15], bc.INNER_N[16]):
        x = np.random.default_rng(N).standard_normal((2, N)).astype(np.float32)
        base = anylen_ref.bluestein_rows(x, N, 2, "rf32")
        for e in (40, -40):
            scaled = anylen_ref.bluestein_rows(x * np.float32(2.0 ** e), N, 2, "rf32")
            assert np.array_equal(scaled.view(np.uint64), (base * 2.0 ** (2 * e)).view(np.uint64)), (N, e)

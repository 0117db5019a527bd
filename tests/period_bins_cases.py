"""Inputs with a small ||y||_1 for the per-bin bound of the periodicity family's power spectra (period_ref.bound_bin,
periodlong_ref.bound_bin): a few impulses whose amplitudes are signed powers of two 2^-2 .. 2^2, so that one faulty path
of the transform -- one entry of a twiddle table, one swapped bin -- stands above the allowance b1 ||y||_1 instead of
drowning in a dense series.  tests/test_period_bins_gpu.py runs them on the device, tests/test_period_bins_cpu.py through
a numpy model of the kernels with mutated tables.  A plain module, like period_family.py beside it.

The places come from the index structure of the kernels.  The packed point is j = n >> 1 = j1 M2 + j2, re and im of it the
even and the odd n.  Long frames (periodlong.hip): M = M1 M2 of periodlong_ref.split, the columns transform over j1, the
twist is twist[k1][j2], the rows transform over j2.  Short frames (period.hip): the first radix-16 pass of row_fft.h takes
the points j2 + j1 M / 16, j1 < 16, so M1 = 16 and M2 = M / 16 there.

A case is (name, nsamp, n int64 [count], amplitudes float32 [count]); series() makes its float32 row of nsamp samples.
Every case's amplitudes sum to zero, so that the mean is zero and ||y||_1 is the sum of the amplitudes' sizes, except
the one pair named "unequal", which keeps the mean's term in play."""
import numpy as np

import periodlong_ref

SHORT_LOG2NS = tuple(range(10, 16))
LONG_LOG2NS = (16, 19, 20, 22)                   # both ends of M1 = 16, the first M1 = 256, the limit
SIZES = np.exp2(np.arange(-2, 3)).astype(np.float32)
EIGHT_TRIALS = 4


def split(log2n):
    """(log2 M1, log2 M2): periodlong_ref.split for the long frames, the first radix-16 pass for the short ones"""
    return periodlong_ref.split(log2n) if log2n >= periodlong_ref.MIN_LOG2N else (4, log2n - 5)


def sample(log2n, j1, j2, odd):
    """n of packed point (j1, j2), its re (odd 0) or im (odd 1)"""
    l1, l2 = split(log2n)
    assert 0 <= j1 < 1 << l1 and 0 <= j2 < 1 << l2 and odd in (0, 1)
    return 2 * ((j1 << l2) + j2) + odd


def place(log2n, n):
    """(j1, j2, odd) of sample n"""
    l1, l2 = split(log2n)
    j = n >> 1
    return j >> l2, j & ((1 << l2) - 1), n & 1


def balanced(rng, count, sizes):
    """count signed amplitudes whose sum is zero: count / 2 seeded sizes, each with both signs, in a seeded order"""
    half = rng.choice(sizes, count // 2).astype(np.float32)
    return rng.permutation(np.concatenate([half, -half])).astype(np.float32)


def pairs(log2n):
    """pairs of impulses a, -a: both parities of n; in one column j2 and in two; on each side of every border (j2 = 0 and
    M2 - 1, j1 = 0 and M1 - 1, n = 0 and N - 1) and at n = nsamp - 1 of an nsamp below N, even and odd.  No distance is
    N / 2 or N / 2 + 1 (the terms would be in phase or opposed in every bin, or hide the last bins)."""
    l1, l2 = split(log2n)
    n, m1, m2 = 1 << log2n, 1 << l1, 1 << l2
    at = lambda j1, j2, odd: sample(log2n, j1, j2, odd)
    c = m2 // 3 + 1
    out = [("one column", n, (at(0, c, 0), at(m1 // 4 + 1, c, 1)), 1.0),
           ("one column, odd first", n, (at(m1 - 1, m2 - 2, 1), at(m1 // 2 - 2, m2 - 2, 0)), 4.0),
           ("first and last column", n, (at(1, 0, 1), at(m1 - 1, m2 - 1, 0)), 0.25),
           ("n = 0", n, (at(0, 0, 0), at(m1 // 2 - 1, m2 - 1, 1)), 2.0),
           ("row 0's last, last row's first", n, (at(0, m2 - 1, 1), at(m1 - 1, 0, 0)), 0.5),
           ("n = N - 1", n, (at(m1 - 1, m2 - 1, 1), at(m1 // 2, 1, 0)), 1.0),
           ("nsamp - 1 even", n - 5, (n - 6, at(2, m2 // 2 + 1, 1)), 2.0),
           ("nsamp - 1 odd", n - 2, (n - 3, at(m1 // 2 + 1, m2 // 2 - 1, 0)), 0.5)]
    cases = [(name, nsamp, np.array(ns, np.int64), np.array([a, -a], np.float32)) for name, nsamp, ns, a in out]
    cases.append(("unequal", n, np.array([at(3, 5, 1), at(m1 - 2, m2 - 7, 0)], np.int64), np.array([2.0, -0.5], np.float32)))
    for name, nsamp, ns, _ in cases:
        assert ns.max() < nsamp and abs(int(ns[0]) - int(ns[1])) % (n // 2) > 1, name
    return cases


def combs(log2n):
    """every j2 of one row j1 (every column of the twist, every point of a row transform: ||y||_1 = M2) and every j1 of one
    column j2 (every row of the twist, every point of a column transform), signed so that no bin is a geometric sum; the
    parities alternate along the comb"""
    l1, l2 = split(log2n)
    n, m1, m2 = 1 << log2n, 1 << l1, 1 << l2
    rng = np.random.default_rng(1000 + log2n)
    j1, j2 = m1 // 3, m2 // 5 + 2
    row = np.array([sample(log2n, j1, c, c & 1) for c in range(m2)], np.int64)
    col = np.array([sample(log2n, r, j2, r & 1) for r in range(m1)], np.int64)
    return [("row %d" % j1, n, row, balanced(rng, m2, np.float32([1.0]))), ("column %d" % j2, n, col, balanced(rng, m1, SIZES))]


def eights(log2n, trials=EIGHT_TRIALS):
    """eight seeded signed impulses a trial"""
    n = 1 << log2n
    rng = np.random.default_rng(2000 + log2n)
    return [("eight %d" % t, n, np.sort(rng.choice(n, 8, replace=False)).astype(np.int64), balanced(rng, 8, SIZES)) for t in range(trials)]


def cases(log2n):
    return pairs(log2n) + combs(log2n) + eights(log2n)


def series(case):
    """float32 [nsamp] of a case"""
    _, nsamp, ns, amps = case
    x = np.zeros(nsamp, np.float32)
    x[ns] = amps
    return x


def stacked(some, width):
    """float32 [len(some), width] of cases, zeros behind each case's nsamp (the caller passes nsamp to the run itself)"""
    x = np.zeros((len(some), width), np.float32)
    for t, case in enumerate(some):
        x[t, :case[1]] = series(case)
    return x


ACCEL_LOG2N, ACCEL_COEFS = 16, (0, 1 << 40, -(1 << 40))


def accel_series():
    """the sparse series of the acceleration search's case: the first of eights(16)"""
    return series(eights(ACCEL_LOG2N)[0])

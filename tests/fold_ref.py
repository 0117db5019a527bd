"""include/rtlws_fold.h restated in numpy: the phases in uint64 with wrap-around, the bins in integers, the profiles added
with np.add.at, which adds unbuffered and in index order, so ascending n by construction -- the yardstick of
tests/test_fold_gpu.py, whose own properties tests/test_fold_cpu.py holds.

  phase_p(n) = (phi0_p + n step_p) mod 2^64;  bin_p(n) = (((phase_p(n) >> 32) nbins) >> 32)
  prof[t][p][s][b] = the f32 sum, ascending n, of the samples of sub-integration s that fall in bin b;  hits: their number
"""
from fractions import Fraction

import numpy as np

from pulse_ref import signed_series                      # float32 [ntrials, n]: both signs, exponents over 2^-6 .. 2^6

MAX_PERIODS, MIN_BINS, MAX_BINS, MIN_SUB, MAX_SUB, MAX_TRIALS, MAX_NSAMP = 4096, 2, 256, 64, 1 << 24, 65536, 1 << 30
TILE = 64                                                # samples a wavefront stages per step
TWO64 = 1 << 64


def step_of(period):
    """the integer nearest to 2^64 / P, halves up, from the double's exact value"""
    return int((Fraction(TWO64) / Fraction(float(period)) + Fraction(1, 2)).__floor__())


def phase_at(step, phi0, n0):
    return (int(phi0) + int(n0) * int(step)) % TWO64


def bins_of(step, phi0, nbins, n0, n1):
    """bin_p(n) for n = n0 .. n1 - 1, int64"""
    n = np.arange(n0, n1, dtype=np.uint64)
    phase = np.full(n.shape, int(phi0), np.uint64) + n * np.full(n.shape, int(step), np.uint64)          # arrays wrap mod 2^64
    return (((phase >> np.uint64(32)) * np.uint64(nbins)) >> np.uint64(32)).astype(np.int64)


def subints(nsamp, sub):
    return -(-nsamp // sub)


def waves_per_block(nbins):
    return 4 if nbins <= 64 else 2 if nbins <= 128 else 1


def plan(nperiods, nbins, sub, ntrials, nsamp):
    """(workgroups, threads, lds_bytes, tile, waves_per_block, nsub) as the header words it"""
    wpb = waves_per_block(nbins)
    groups = -(-nperiods // (64 * wpb))
    return ntrials * groups * subints(nsamp, sub), 64 * wpb, wpb * nbins * 256, TILE, wpb, subints(nsamp, sub)


def fold_ref(series, steps, phases, nbins, sub, nsamp):
    """(prof float32 [ntrials, nperiods, nsub, nbins], hits uint32 [nperiods, nsub, nbins]) of series float32
    [ntrials, >= nsamp]; nothing at or beyond nsamp is looked at.  One np.add.at per (period, sub-integration) over
    [trial, n] in C order: every (trial, bin) gets its samples in ascending n"""
    series = np.asarray(series, np.float32)
    assert series.ndim == 2 and series.shape[1] >= nsamp and len(steps) == len(phases)
    ntrials, nsub = series.shape[0], subints(nsamp, sub)
    prof = np.zeros((ntrials, len(steps), nsub, nbins), np.float32)
    hits = np.zeros((len(steps), nsub, nbins), np.uint32)
    rows = np.arange(ntrials)[:, None]
    with np.errstate(invalid="ignore", over="ignore"):
        for p, (step, phi0) in enumerate(zip(steps, phases)):
            for s in range(nsub):
                n0, n1 = s * sub, min((s + 1) * sub, nsamp)
                b = bins_of(step, phi0, nbins, n0, n1)
                acc = np.zeros((ntrials, nbins), np.float32)
                np.add.at(acc, (rows, b[None, :]), series[:, n0:n1])
                prof[:, p, s] = acc
                hits[p, s] = np.bincount(b, minlength=nbins)
    return prof, hits


def fold_by_the_letter(x, step, phi0, nbins, order=None):
    """one series, one period, one sub-integration in a plain Python loop of np.float32 additions; order: the n in the
    order they are added (None: ascending)"""
    acc = [np.float32(0.0)] * nbins
    count = [0] * nbins
    with np.errstate(invalid="ignore", over="ignore"):
        for n in (range(len(x)) if order is None else order):
            b = ((((int(phi0) + n * int(step)) % TWO64) >> 32) * nbins) >> 32
            acc[b] = np.float32(acc[b] + np.float32(x[n]))
            count[b] += 1
    return np.array(acc, np.float32), np.array(count, np.uint32)


def fold_partials(x, step, phi0, nbins, part):
    """partial profiles of `part` samples each, added in turn: what the contract is NOT"""
    total = np.zeros(nbins, np.float32)
    for n0 in range(0, len(x), part):
        acc, _ = fold_by_the_letter(x[n0:n0 + part], step, phase_at(step, phi0, n0), nbins)
        total = total + acc
    return total


def chi2(prof, hits, sum1, sum2, count):
    """rtlws_fold_chi2's expression in numpy f64, b ascending"""
    if count < 2 or len(prof) < 1:
        return np.nan
    mean = np.float64(sum1) / np.float64(count)
    var = np.float64(sum2) / np.float64(count) - mean * mean
    if not var > 0 or np.any(np.asarray(hits) == 0):
        return np.nan
    total = np.float64(0.0)
    for pb, hb in zip(np.asarray(prof, np.float64), np.asarray(hits, np.float64)):
        d = pb - hb * mean
        total = total + d * d / (hb * var)
    return total


def table(nperiods, seed, first=3.0, spread=0.37):
    """(steps, phases) uint64 [nperiods]: non-dyadic periods first + spread i samples, seeded phases"""
    rng = np.random.default_rng(seed)
    steps = np.array([step_of(first + spread * i) for i in range(nperiods)], np.uint64)
    return steps, rng.integers(0, TWO64, nperiods, dtype=np.uint64)

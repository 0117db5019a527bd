"""GPU suite of the periodicity family's power row, bin by bin: librtlws_period.so (log2n 10 .. 15), librtlws_periodlong.so
(16, 19, 20, 22) and librtlws_accel.so over the sparse inputs of tests/period_bins_cases.py -- pairs of impulses on each
side of every border of the index structure, combs along a row and a column of the twist, eight seeded impulses -- whose
||y||_1 is small enough for one faulty term of one bin to stand above period_ref.bound_bin / periodlong_ref.bound_bin.
Every bin of every trial is held to that allowance against the f64 spectrum; every case passes the aggregate bound and
the bit-for-bit checks of stages 2 - 4 behind it as well.  tests/test_period_bins_cpu.py shows on a numpy model of the
kernels which faults this check sees and the aggregate one does not.

Worst per-bin share of `bound_bin`, measured on one MI355X (printed by the tests, the largest of the three families):
0.0294, 0.0293, 0.0276, 0.0318, 0.0343, 0.0299 at log2n 10 .. 15; 0.0284, 0.0318, 0.0335, 0.0350 at log2n 16, 19, 20, 22;
0.0199 through rtlws_accel_search at log2n 16.  The aggregate bound's worst share on the same inputs: 0.0059 .. 0.0082."""
import numpy as np
import pytest

import accel_ref
import period_bins_cases as cases
import period_ref
import periodlong_ref
from period_family import FILL, check_behind, check_stage1, same_bits, unpack

pytestmark = pytest.mark.gpu

WORST, WORST_BIN = {}, {}
LOG2NS = cases.SHORT_LOG2NS + cases.LONG_LOG2NS


def _long(log2n):
    return log2n >= periodlong_ref.MIN_LOG2N


def _bounds(log2n):
    ref = periodlong_ref if _long(log2n) else period_ref
    return ref.bound(log2n), ref.bound_bin(log2n)


def _reference(log2n):
    """the f64 spectrum of a trial's samples; the premises of the aggregate bound hold for every case"""
    def reference(xs, name):
        ref, nyquist_small, mean_small = periodlong_ref.power_and_premises(xs, log2n)
        assert nyquist_small and mean_small, name
        return ref
    return reference


def _plan(log2n):
    """(levels, norm, seg, klo): few levels on the longest frames, whose restated harmonic sums are the host's long pole"""
    return (5, 64, 64, 1) if not _long(log2n) else (2, 1024, 1024, 8) if log2n < 20 else (1, 1024, 1024, 8)


def _run(built, engine, some, log2n, family):
    """cases of one nsamp in one launch: NaN behind nsamp, guards behind the outputs, both bounds of stage 1 and the checks
    behind it"""
    nsamp = some[0][1]
    assert all(c[1] == nsamp for c in some)
    levels, norm, seg, klo = _plan(log2n)
    m = 1 << (log2n - 1)
    stride = (nsamp + 3) // 4 * 4
    x = cases.stacked(some, stride)
    rows = x.copy()
    rows[:, nsamp:] = np.nan
    run = engine.periodlong if _long(log2n) else engine.period
    outs = run(rows, log2n, levels, norm, seg, klo, nsamp=nsamp, in_stride=stride, fill=FILL)
    name = (log2n, [c[0] for c in some])
    best, at, power, white = unpack(outs, len(some), levels, m // seg, m, built.PERIOD_GUARD, name)
    c, b1 = _bounds(log2n)
    check_stage1(power, x, nsamp, c, b1, _reference(log2n), WORST, WORST_BIN, (log2n, family), name)
    check_behind(power, white, best, at, levels, norm, seg, klo, name)


@pytest.mark.parametrize("family", ["pairs", "combs", "eights"])
@pytest.mark.parametrize("log2n", LOG2NS)
def test_sparse_inputs(built, engine, log2n, family):
    """every case of a family at a frame length; one launch per nsamp, two trials a launch from log2n 20 on"""
    some = getattr(cases, family)(log2n)
    per = len(some) if log2n < 20 else 2
    for nsamp in sorted({c[1] for c in some}):
        group = [c for c in some if c[1] == nsamp]
        for first in range(0, len(group), per):
            _run(built, engine, group[first:first + per], log2n, family)
    key = (log2n, family)
    print("log2n %d %s: worst bin %.3g of bound_bin %.3g, worst aggregate share %.3g" % (log2n, family, WORST_BIN[key], _bounds(log2n)[1], WORST[key]))


def test_through_the_acceleration_search(built, engine):
    """one sparse series at 2^16 under coefficients 0, +2^40, -2^40: every virtual trial's power row bin by bin against the
    f64 spectrum of accel_ref's resampled series, the checks behind it, and coefficient 0 bit for bit the plain search"""
    log2n, coefs, plan = cases.ACCEL_LOG2N, list(cases.ACCEL_COEFS), (2, 64, 256, 8)
    x = cases.accel_series()[None, :]
    best, at, power, white = engine.accel_search(x, log2n, *plan, coefs)
    resampled = accel_ref.resample(x, coefs)
    assert resampled.shape == (1, 3, 1 << log2n) and np.any(resampled[0, 1] != resampled[0, 0]) and np.any(resampled[0, 2] != resampled[0, 0])
    worst, worst_bin = {}, {}
    check_stage1(power[0], resampled[0], 1 << log2n, accel_ref.bound(log2n), accel_ref.bound_bin(log2n), _reference(log2n), worst, worst_bin,
                 log2n, "accel")
    check_behind(power[0], white[0], best[0], at[0], *plan, "accel")
    want = engine.periodlong(x, log2n, *plan)
    for g, w, what in zip((best, at, power, white), want, ("best", "at", "power", "white")):
        same_bits(g[:, 0], w, what, nan_by_place=False)
    print("accel log2n %d: worst bin %.3g of bound_bin %.3g" % (log2n, worst_bin[log2n], accel_ref.bound_bin(log2n)))

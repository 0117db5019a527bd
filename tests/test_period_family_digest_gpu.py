"""The periodicity-search family's outputs on fixed inputs, pinned to the bit (rtlws_period.h, rtlws_periodlong.h,
rtlws_accel.h), and every depth of the stages' trees against the restatement.

The libraries share the rule of the peaks and the untangling of a pair (csrc/period_stages.h) and one host header of
rules and plan (csrc/period_plan.h); the whitening and the harmonic walk with the peaks are written out twice, in
period.hip and over spans in periodlong.hip, and are promised to give the same bits.  The SHA-256 digests in
tests/golden/period_family_sha256.json were RECORDED ON AN MI355X FROM THE BUILD OF COMMIT 929f98b ("Acceleration
search: long frames read through index maps, no copy"), before any of the family's text was shared; whatever is moved
between the libraries' texts afterwards, or changed in one of the two restatements, has to give the same bytes.  A
digest that differs means an order, a rounding or a contraction changed -- find which, a tolerance is not the answer.

Inputs come from integer arithmetic alone (tests/helpers.py's counter hash): its bytes read as int8, converted exactly
to f32, plus a square wave of 0 / 24 every 19 samples, so that no libm is in the fixture.  Such a series has power in
every bin, and the test asserts that no whitened bin is NaN (an all-zero whitening block would give 0 / 0, whose bits
are not pinned).  The shapes are the smallest at which every branch of those stages is taken:
  period      log2n 10 (one wavefront, half its lanes idle in the whitening, M < 1024), 12 (two wavefronts), 15
              (sixteen); plans (levels, norm, seg, klo) (5, 16, 64, 1), (5, M, M, 1) and (1, min(1024, M), min(2048, M),
              seg - 1); nsamp N and N - 3 (a partial quad); two trials
  periodlong  log2n 16 (M1 = 16, two spans: a span's border inside the harmonic reads, a nonzero first segment) and 20
              (M1 = 256); plans (5, 16, 64, 1), (5, 16384, 16384, 1), (1, 1024, 2048, 2047); nsamp N and N - 3; one trial;
              and at log2n 16 two trials through a plan of max_trials = 1 (two groups)
  accel       log2n 16, one trial, coefficients [0, 2^40, -2^40, 12345], plan (5, 64, 256, 8): the search, and the
              resampling of the whole table

test_every_depth_of_the_trees runs every power-of-two norm 16 .. 16384 with every power-of-two seg 64 .. 16384 once
(norm i with seg i mod 9: eleven runs a library; period at log2n 15, periodlong at log2n 16), which the other suites'
plans (norm from 16, 1024, 2048, M, 16384) do not: every depth of the lanes' tree, the wavefronts' tree and the merge of
chunks, bit for bit against period_ref over the device's own power row."""
import hashlib
import json
import os

import numpy as np
import pytest

from helpers import hash_bytes
from period_family import check_behind, noise

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "period_family_sha256.json")
COEFS = [0, 1 << 40, -(1 << 40), 12345]
NAMES = ("best", "at", "power", "white")


def series_of(log2n, ntrials):
    """float32 [ntrials, N]: the hash's bytes as int8 plus 24 on every other stretch of 19 samples, all integers"""
    n = 1 << log2n
    x = hash_bytes(ntrials * n, seed=300 + log2n).view(np.int8).astype(np.float32).reshape(ntrials, n)
    return x + np.float32(24) * ((np.arange(n) // 19) % 2 == 0).astype(np.float32)


def short_plans(log2n):
    m = 1 << (log2n - 1)
    seg = min(2048, m)
    return ((5, 16, 64, 1), (5, m, m, 1), (1, min(1024, m), seg, seg - 1))


LONG_PLANS = ((5, 16, 64, 1), (5, 16384, 16384, 1), (1, 1024, 2048, 2047))


def cases():
    out = [("period", n, i, cut) for n in (10, 12, 15) for i in range(3) for cut in (0, 3)]
    out += [("periodlong", n, i, cut) for n in (16, 20) for i in range(3) for cut in (0, 3)]
    return out + [("periodlong", 16, "groups", 0), ("accel", 16, "search", 0), ("accel", 16, "resample", 0)]


def case_id(case):
    return "%s-%d-%s-cut%d" % case


def outputs(eng, case):
    """the named outputs of a case, each a contiguous array"""
    lib, log2n, which, cut = case
    nsamp = (1 << log2n) - cut
    if lib == "period":
        x = series_of(log2n, 2)[:, :nsamp]
        return dict(zip(NAMES, eng.period(x, log2n, *short_plans(log2n)[which])))
    if lib == "periodlong":
        if which == "groups":
            return dict(zip(NAMES, eng.periodlong(series_of(log2n, 2), log2n, *LONG_PLANS[0], max_trials=1)))
        x = series_of(log2n, 1)[:, :nsamp]
        return dict(zip(NAMES, eng.periodlong(x, log2n, *LONG_PLANS[which])))
    x = series_of(log2n, 1)
    if which == "search":
        return dict(zip(NAMES, eng.accel_search(x, log2n, 5, 64, 256, 8, COEFS)))
    return {"rows": eng.accel_resample(x, log2n, COEFS)}


def digests(eng, case):
    outs = outputs(eng, case)
    assert all(o.size > 0 for o in outs.values())
    if "white" in outs:
        assert not np.isnan(outs["white"]).any() and not np.isnan(outs["best"]).any(), "a NaN's bits are not pinned"
    return {name: hashlib.sha256(np.ascontiguousarray(o).tobytes()).hexdigest() for name, o in outs.items()}


def inputs_digest():
    h = hashlib.sha256()
    for log2n in (10, 12, 15, 16, 20):
        h.update(series_of(log2n, 2 if log2n <= 16 else 1).tobytes())
    return h.hexdigest()


def test_inputs_are_fixed():
    x = series_of(10, 2)
    assert x.dtype == np.float32 and x.shape == (2, 1024) and np.array_equal(x, np.rint(x)) and not np.array_equal(x[0], x[1])
    assert x.min() >= -128 and x.max() <= 127 + 24 and len(set(x[0].tolist())) > 200
    with open(GOLDEN) as fh:
        recorded = json.load(fh)
    assert sorted(recorded["sha256"]) == sorted(case_id(c) for c in cases()) and len(recorded["sha256"]) == 33
    assert all(sorted(d) == (["rows"] if "resample" in c else sorted(NAMES)) for c, d in recorded["sha256"].items())
    assert recorded["inputs_sha256"] == inputs_digest()


@pytest.mark.gpu
@pytest.mark.parametrize("case", cases(), ids=case_id)
def test_output_bit_identical_to_the_per_library_text(engine, case):
    with open(GOLDEN) as fh:
        recorded = json.load(fh)["sha256"]
    assert digests(engine, case) == recorded[case_id(case)]


TREE_NORMS = [16 << i for i in range(11)]                        # 16 .. 16384
TREE_SEGS = [64 << i for i in range(9)]                          # 64 .. 16384


def test_the_trees_cases_cover_every_depth(built):
    pairs = [(TREE_NORMS[i], TREE_SEGS[i % 9]) for i in range(11)]
    assert {p[0] for p in pairs} == set(TREE_NORMS) and {p[1] for p in pairs} == set(TREE_SEGS)
    assert TREE_NORMS[-1] == TREE_SEGS[-1] == 16384 == 1 << 14
    assert all(built.period_supported(15, 5, norm, seg, 1) == 1 and built.periodlong_supported(16, 5, norm, seg, 1) == 1 for norm, seg in pairs)


@pytest.mark.gpu
@pytest.mark.parametrize("lib,log2n", [("period", 15), ("periodlong", 16)])
def test_every_depth_of_the_trees(engine, lib, log2n):
    n = 1 << log2n
    x = noise(1, n, seed=700 + log2n)
    x[0] += (3.0 * np.cos(2.0 * np.pi * np.arange(n) / 37.5)).astype(np.float32)
    for i, norm in enumerate(TREE_NORMS):
        seg = TREE_SEGS[i % 9]
        best, at, power, white = getattr(engine, lib)(x, log2n, 5, norm, seg, 1)
        assert not np.isnan(white).any() and np.all(at >= 1)
        check_behind(power, white, best, at, 5, norm, seg, 1, (lib, norm, seg))

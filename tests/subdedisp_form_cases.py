"""The forms a subband dedispersion plan takes as data (include/rtlws_subdedisp.h, csrc/subdedisp.h,
csrc/subdedisp_shim.hip): the plan's rule for both stages restated over whole tables, tables whose plan is
a given form at a given spread for either stage, and the list of them that tests/test_subdedisp_gpu.py launches.
tests/test_subdedisp_cpu.py holds the list to its own conditions and rtlws_subdedisp_geometry to the rule.  Nothing here
touches the library.

Stage 1 is the dedispersion's tile over d1 as a table of A trials: its rule is tests/dedisp_form_cases.py's `form`, and its
tables here are that file's, read as d1.  Stage 2: a workgroup owns TILE outputs of `per` consecutive trials of one
nominal and stages 32 subbands at a time, columns of TILE + spread values, spread the widest difference of d2 inside a
subband that keeps a position and a group; 32 * (TILE + spread) + TILE words must fit 9216 (36 KiB) or 16384 (64 KiB).
Groups of 8, 4 and 2 trials are taken where they fit and the largest nominal fills more than half of one; one trial
spreads nothing."""
from collections import namedtuple

import numpy as np

import dedisp_form_cases as forms1
import dedisp_ref
import subdedisp_ref

TILE, CHUNK = forms1.TILE, 32
SMALL_WORDS, BIG_WORDS, SMALL_LDS, BIG_LDS = forms1.SMALL_WORDS, forms1.BIG_WORDS, forms1.SMALL_LDS, forms1.BIG_LDS
NOUT = TILE + 1
STEP = 500                 # between the d2 of neighbouring groups of a nominal: above 248, so no two groups share a workgroup
NCHAN1, NSUB1 = 36, 3      # stage 1's cases: subbands of 12 positions, their borders inside every chunk width but 4
NCHAN2, NSUB2 = 72, 18     # stage 2's cases: subbands of 4 positions, a partial chunk of 18 subbands


def form2(spread, per):
    """(LDS bytes, stride) of stage 2 with `per` trials a workgroup at a widest spread of `spread`; None: not served"""
    words = CHUNK * (TILE + spread) + TILE
    if per == 1:
        assert spread == 0
    return (BIG_LDS if words > SMALL_WORDS else SMALL_LDS, TILE + spread) if words <= BIG_WORDS else None


# the last spread either LDS size serves in stage 2 and the first it does not
BORDERS2 = ((SMALL_LDS, 24, 25), (BIG_LDS, 248, 249))


def groups2(first, per):
    """[(first trial, trials, nominal)] of stage 2: groups of `per` trials, none across a border of first"""
    return [(t0, min(per, int(first[a + 1]) - t0), a) for a in range(len(first) - 1) for t0 in range(int(first[a]), int(first[a + 1]), per)]


def spread1(d1, mask, per):
    """the widest spread of d1 inside four neighbouring positions and `per` aligned nominals, over the kept positions"""
    A, M = d1.shape
    keep = np.ones(M, bool) if mask is None else np.asarray(mask) != 0
    widest = 0
    for a0 in range(0, A, per):
        part = d1[a0:a0 + per].astype(np.int64)
        hi = np.where(keep[None, :], part, -1).max(axis=0).reshape(-1, 4).max(axis=1)
        lo = np.where(keep[None, :], part, 1 << 30).min(axis=0).reshape(-1, 4).min(axis=1)
        widest = max(widest, int(np.where(hi >= 0, hi - lo, 0).max()))
    return widest


def spread2(first, d2, keeps, per):
    widest = 0
    for t0, count, _ in groups2(first, per):
        part = d2[t0:t0 + count][:, keeps]
        if part.size:
            widest = max(widest, int((part.max(axis=0) - part.min(axis=0)).max()))
    return widest


def plan(first, d1, d2, mask=None):
    """(nominals a workgroup, LDS bytes) of stage 1 and (trials a workgroup, LDS bytes) of stage 2, by the rule"""
    first, d1, d2 = np.asarray(first), np.asarray(d1), np.asarray(d2)
    A, M = d1.shape
    for per in (8, 4, 2, 1):
        if per > 1 and per >= 2 * A:
            continue
        f = forms1.form(spread1(d1, mask, per), per)
        if f is not None:
            stage1 = (per, f[1])
            break
    most = int(np.diff(first).max())
    keeps = subdedisp_ref.kept_subbands(M, d2.shape[1], mask)
    stage2 = (1, SMALL_LDS)
    for per in (8, 4, 2):
        if per >= 2 * most:
            continue
        f = form2(spread2(first, d2, keeps, per), per)
        if f is not None:
            stage2 = (per, f[0])
            break
    return stage1, stage2


def geometry(first, d1, d2, mask, nout):
    """what rtlws_subdedisp_geometry reports behind its return code"""
    (per1, lds1), (per2, lds2) = plan(first, d1, d2, mask)
    m1, m2 = subdedisp_ref.maxima(d1, d2, mask)
    tiles = lambda n: -(-n // TILE)
    blocks = (tiles(nout + m2) * -(-d1.shape[0] // per1) if nout else 0, tiles(nout) * len(groups2(first, per2)))
    return blocks, (256, 256), (lds1, lds2), TILE, per1, per2, m1, m2


# ---- stage 1's cases: tests/dedisp_form_cases.py's tables as d1 ----
# every trial count 9 becomes nine nominals (a last group of one), every nominal two trials; d2 is random to 5

def stage1_case_tables(case):
    d1 = forms1.table(case, NCHAN1)
    first = subdedisp_ref.even_first(2 * d1.shape[0], 2)
    d2 = dedisp_ref.hashed_ints(2 * d1.shape[0] * NSUB1, 5, 31 + case.spread).reshape(-1, NSUB1)
    return first, d1, d2


STAGE1_CASES = forms1.CASES
STAGE1_FORMS = forms1.SIX_FORMS


# ---- stage 2's cases ----
# kind "border": trial j of a nominal delays every subband by 500 (j // per), and the trials with j % per == per - 1 the
# subband `place` by `spread` more: `per` trials spread `spread` in one subband, any 2 per of a nominal 500.  kind "drop":
# the later half of every group one value behind the earlier half in every subband, the delayed subband still `spread`
# behind the group's least: `per` trials spread `spread`, their later half spread - 1 and their earlier half nothing.
# Every nominal holds 2 per + 1 trials (its last group one trial), the last nominal per (one whole group and nothing else).
Case2 = namedtuple("Case2", "kind per spread place nominals plan_per plan_spread")
PLACES = ("first", "last")


def stage2_first(case):
    sizes = [2 * case.per + 1] * (case.nominals - 1) + [case.per]
    return np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)


def stage2_case_tables(case, nchan=NCHAN2, nsub=NSUB2):
    first = stage2_first(case)
    T = int(first[-1])
    j = np.arange(T) - first[subdedisp_ref.nominal_of(first)]
    d2 = np.repeat((STEP * (j // case.per))[:, None], nsub, axis=1).astype(np.int32)
    s = 0 if case.place == "first" else nsub - 1
    if case.kind == "border":
        d2[j % case.per == case.per - 1, s] += case.spread
    else:
        d2[j % case.per >= case.per // 2] += 1
        d2[j % case.per == case.per - 1, s] += case.spread - 1
    d1 = dedisp_ref.hashed_ints((len(first) - 1) * nchan, 5, 57 + case.spread).reshape(-1, nchan)
    return first, d1, d2


def delayed_subband(case, nsub=NSUB2):
    return 0 if case.place == "first" else nsub - 1


def case2_id(case):
    return "%s-per%d-spread%d-%s-%dnominals" % (case.kind, case.per, case.spread, case.place, case.nominals)


def _cases2():
    out = []
    for per in (8, 4, 2):
        for place in PLACES:
            nominals = 3 if place == "first" else 1
            for spread in (0, 1, 24, 25, 248):
                out.append(Case2("border", per, spread, place, nominals, per, spread))
            # past the border: the delayed trial alone is 249 behind its neighbours, and only one trial a workgroup serves it ...
            out.append(Case2("border", per, 249, place, nominals, 1, 0))
            # ... or only the whole group spreads it, and half the group is served at 248
            out.append(Case2("drop", per, 249, place, nominals, per // 2, 248 if per > 2 else 0))
    return out


STAGE2_CASES = _cases2()


def _the_case2(per, spread, place):
    return next(c for c in STAGE2_CASES if (c.kind, c.per, c.spread, c.place) == ("border", per, spread, place))


# one table per form of stage 2: 8 trials in either LDS, 4 and 2 trials, one trial
STAGE2_FORMS = (_the_case2(8, 24, "first"), _the_case2(8, 248, "last"), _the_case2(4, 25, "first"), _the_case2(2, 24, "last"),
                _the_case2(2, 249, "first"))

"""The forms a dedispersion plan takes as data (include/rtlws_dedisp.h, csrc/dedisp.h, csrc/dedisp_shim.hip, DESIGN.md
4.19): the rule that turns the widest spread of delays inside four neighbouring positions and a trial group into a
chunk width, an LDS size and a column stride, the last spread every form serves, tables whose plan is a given form at a
given spread, and the list of them that tests/test_dedisp_gpu.py launches.  tests/test_dedisp_forms_cpu.py holds the
list to its own conditions.  Nothing here touches the library.

A workgroup owns TILE outputs of `per` trials and stages chunk columns of TILE + spread rows, `stride` words apart, with
TILE zeros behind them; chunk * stride + TILE words must fit 9216 (36 KiB) or 16384 (64 KiB).  Groups of 8, 4 and 2
trials only take chunks of 32 positions; one trial narrows the chunk to 16, 8 and 4, and beyond that every position
gets a column of its own (`lone`), TILE rows whatever the spread."""
from collections import namedtuple

import numpy as np

import dedisp_ref

TILE = 256
SMALL_WORDS, BIG_WORDS = 9216, 16384
SMALL_LDS, BIG_LDS = 4 * SMALL_WORDS, 4 * BIG_WORDS
MAX_DELAY = 65535
NCHAN = 36                 # a partial last chunk behind every chunk width: 32 + 4, 16 + 16 + 4, 4 * 8 + 4, 9 * 4
NOUT = TILE + 1            # the first tile full: output 255 of the delayed trial reads the last word of the longest column
STEP = 500                 # between the delays of neighbouring trial groups: above 247, so no two groups share a workgroup


def fit_stride(height, quads):
    """csrc/dedisp.h fit_stride (tools/lds_sim.py dedisp_stride): the smallest stride >= height that is (8 / quads) times
    an odd number; any stride where a chunk is one quad"""
    unit = 8 // quads if quads > 1 else 1
    s = -(-height // unit)
    if quads > 1 and s % 2 == 0:
        s += 1
    return s * unit


def form(spread, per):
    """(chunk or "lone", LDS bytes, stride) of a plan of `per` trials a workgroup whose widest spread is `spread`; None
    where `per` trials are not served at that spread"""
    for chunk in ((32, 16, 8, 4) if per == 1 else (32,)):
        stride = fit_stride(TILE + spread, chunk // 4)
        words = chunk * stride + TILE
        if words <= BIG_WORDS:
            return chunk, BIG_LDS if words > SMALL_WORDS else SMALL_LDS, stride
    return ("lone", SMALL_LDS, fit_stride(TILE, 8)) if per == 1 else None


# ((chunk, LDS bytes), the last spread the form serves, the first one it does not): one trial a workgroup takes them in
# this order; groups of 8, 4 and 2 take the first two and nothing behind them
BORDERS = (((32, SMALL_LDS), 23, 24), ((32, BIG_LDS), 247, 248), ((16, SMALL_LDS), 302, 303), ((16, BIG_LDS), 750, 751),
           ((8, SMALL_LDS), 860, 861), ((8, BIG_LDS), 1756, 1757), ((4, SMALL_LDS), 1984, 1985), ((4, BIG_LDS), 3776, 3777),
           (("lone", SMALL_LDS), MAX_DELAY, None))

# spreads at which TILE + spread is 0 and 1 past a multiple of the rows one pass of the staging loop covers, 4 * 256 / quads
# (csrc/dedisp.hip: DEPTH rows of a thread, 256 / quads threads a quad): the loop's last pass begins at, and one before,
# the column's last row.  {quads: spreads}
STAGING = {8: (128, 129), 4: (256, 257), 2: (768, 769), 1: (1792, 1793, 2816, 2817)}

PLACES = ("first", "last")  # of the delayed position: position 3 of quad 0, position 0 of the row's last quad


def cap(ntrials):
    """the most trials a workgroup takes of a table of ntrials: 8 from five on, 4 for three and four"""
    return 8 if ntrials >= 5 else 4 if ntrials >= 3 else ntrials


def _bases(ntrials, nchan, per):
    t = np.arange(ntrials)
    return t, np.repeat((STEP * (t // per))[:, None], nchan, axis=1).astype(np.int32)


def border_table(ntrials, nchan, per, spread, quad, hi):
    """int32 [ntrials, nchan] whose plan is `per` trials a workgroup with a widest spread of exactly `spread`: trial t
    delays every position by 500 (t // per), and the trials with t % per == per - 1 position 4 quad + hi by `spread`
    more, the rest of that quad staying behind.  Any aligned 2 per trials spread 500 and are refused; `per` spread
    `spread`, inside one quad.  (Where `spread` is more than `per` trials are served with, the plan is one trial.)"""
    assert per in (8, 4, 2, 1) and per <= cap(ntrials) and ntrials >= per and 0 <= 4 * quad + hi < nchan and 0 <= hi < 4
    assert per > 1 or spread > 247 or ntrials == 1           # one trial a workgroup: two must not fit together
    t, d = _bases(ntrials, nchan, per)
    d[t % per == per - 1, 4 * quad + hi] += spread
    assert d.max() <= MAX_DELAY
    return d


def drop_table(ntrials, nchan, per, spread, quad, hi):
    """border_table with the later half of every group, t % per >= per / 2, one row behind the earlier half at every
    position, the delayed position still at `spread` behind the group's least delay: `per` trials spread `spread`, the
    later per / 2 of them spread - 1.  At spread 248 the plan is per / 2 trials a workgroup at 247."""
    assert per in (8, 4, 2) and spread >= 2
    t, d = _bases(ntrials, nchan, per)
    d[t % per >= per // 2] += 1
    d[t % per == per - 1, 4 * quad + hi] += spread - 1
    return d


# kind: "border" (border_table) or "drop" (drop_table); per, spread, place, ntrials: the table's arguments; plan_per,
# plan_spread: the trials a workgroup and the widest spread of the plan the table must get
Case = namedtuple("Case", "kind per spread place ntrials plan_per plan_spread")


def table(case, nchan=NCHAN):
    make = border_table if case.kind == "border" else drop_table
    return make(case.ntrials, nchan, case.per, case.spread, *_place(case.place, nchan))


def _place(place, nchan):
    return (0, 3) if place == "first" else (nchan // 4 - 1, 0)


def delayed_position(case, nchan=NCHAN):
    quad, hi = _place(case.place, nchan)
    return 4 * quad + hi


def case_id(case):
    return "%s-per%d-spread%d-%s-%dtrials" % (case.kind, case.per, case.spread, case.place, case.ntrials)


def _cases():
    out = []
    for per in (8, 4, 2):
        for place in PLACES:
            # nine trials (a last group of one trial), and one whole group and nothing else
            ntrials = 9 if place == "first" else per
            for spread in (0, 1, 23, 24, 247):
                out.append(Case("border", per, spread, place, ntrials, per, spread))
            # past the border: the delayed trial alone spreads 248, and one trial a workgroup takes it in chunks of 16 ...
            out.append(Case("border", per, 248, place, ntrials, 1, 248))
            # ... or only the group does, and half the group is served at 247
            out.append(Case("drop", per, 248, place, ntrials, per // 2, 247))
    spreads = sorted({s for _, last, beyond in BORDERS[:-1] for s in (last, beyond)} | {s for ss in STAGING.values() for s in ss})
    for place in PLACES:
        for spread in spreads:
            out.append(Case("border", 1, spread, place, 1 if spread <= 247 else 9, 1, spread))
    return out


CASES = _cases()


def _the_case(per, spread, place):
    return next(c for c in CASES if (c.kind, c.per, c.spread, c.place) == ("border", per, spread, place))


# one table per form: 8 trials in either LDS, 2 trials, chunks of 16, chunks of 4 in the whole 64 KiB, lone
SIX_FORMS = (_the_case(8, 23, "first"), _the_case(8, 247, "last"), _the_case(2, 24, "first"), _the_case(1, 302, "last"),
             _the_case(1, 3776, "first"), _the_case(1, 3777, "last"))


def masks(case, nchan=NCHAN):
    """((name, uint8 [nchan]), ..): dedisp_ref.random_mask under the first seed that keeps the delayed position and the
    one that stays behind beside it; position (q + 1) % 4 of every quad q left out; the quads q % 3 == 1 left out.  All
    keep positions 0, 3, nchan - 4 and nchan - 1, so the table keeps its spread"""
    p = delayed_position(case, nchan)
    beside = p - 3 if p % 4 else p + 3
    seed = next(s for s in range(p, 100 * nchan, nchan) if dedisp_ref.random_mask(nchan, s)[beside])
    i = np.arange(nchan)
    return (("random", dedisp_ref.random_mask(nchan, seed)), ("one of every quad", (i % 4 != (i // 4 + 1) % 4).astype(np.uint8)),
            ("whole quads", (i // 4 % 3 != 1).astype(np.uint8)))

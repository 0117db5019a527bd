"""CPU suite of the forms of a dedispersion plan (tests/dedisp_form_cases.py, csrc/dedisp.h, csrc/dedisp_shim.hip,
DESIGN.md 4.19): the restated rule gives the borders that include/rtlws_dedisp.h words (23, 247 and 3776 rows) and the
seven between and behind them, the tile fills its LDS to the last word at 3776, rtlws_dedisp_geometry gives every table
of the list the plan the rule says, a masked outlier is no spread, and the list that
tests/test_dedisp_gpu.py::test_every_border_of_the_plan launches stands on both sides of every border with the delayed
position in the row's first and last quad.  No GPU is used."""
import os
import re

import numpy as np

import dedisp_form_cases as forms
import dedisp_ref
from dedisp_form_cases import BIG_LDS, BORDERS, CASES, NCHAN, NOUT, SMALL_LDS, TILE
from test_abi_cpu import INCLUDE

CSRC = os.path.join(os.path.dirname(INCLUDE), "rtl-ws_amd", "csrc")


def test_the_rule_gives_the_borders():
    """Walking every spread 0 .. 65535, one trial a workgroup changes its form at the nine places of BORDERS and
    nowhere else; groups of 8, 4 and 2 are served to 247 and change their LDS behind 23; the header's three figures are
    those of the walk, and the constants restated here are dedisp.h's."""
    changes, before = [], None
    for spread in range(forms.MAX_DELAY + 1):
        now = forms.form(spread, 1)[:2]
        if now != before:
            changes.append((now, spread))
            before = now
    assert [f for f, _ in changes] == [f for f, _, _ in BORDERS]
    firsts = [first for _, first in changes] + [None]
    assert firsts[0] == 0 and [(first - 1 if first else forms.MAX_DELAY, first) for first in firsts[1:]] == [(last, beyond) for _, last, beyond in BORDERS]
    assert [last for _, last, _ in BORDERS] == [23, 247, 302, 750, 860, 1756, 1984, 3776, 65535]
    for per in (8, 4, 2):
        served = [forms.form(spread, per) for spread in range(300)]
        assert [f[:2] for f in served[:248]] == [(32, SMALL_LDS)] * 24 + [(32, BIG_LDS)] * 224 and not any(served[248:])
        assert all(forms.form(spread, per) == forms.form(spread, 1) for spread in range(248))
    assert forms.form(3777, 1) == forms.form(65535, 1) == ("lone", SMALL_LDS, 257)
    header = " ".join(open(os.path.join(INCLUDE, "rtlws_dedisp.h")).read().replace(" *", " ").split())
    for words in ("8, 4, 2, 1", "whose widest such spread stays within 247 rows", "within 23 rows a workgroup takes 36 KiB of LDS, else 64 KiB",
                  "spreads up to 3776 rows", "and beyond that each position by itself"):
        assert words in header, words
    txt = open(os.path.join(CSRC, "dedisp.h")).read()
    assert "TILE_OUT = %d;" % TILE in txt and "SMALL_WORDS = 9 * 1024, BIG_WORDS = 16 * 1024;" in txt and "MAX_CHUNK = 32;" in txt
    assert (forms.SMALL_WORDS, forms.BIG_WORDS) == (9 * 1024, 16 * 1024)
    assert "const int unit = quads > 1 ? 8 / quads : 1;" in txt and "if (quads > 1 && s % 2 == 0) ++s;" in txt
    for height, quads, want in ((256, 8, 257), (257, 8, 257), (258, 8, 259), (556, 4, 558), (1256, 2, 1260), (3756, 1, 3756)):
        assert forms.fit_stride(height, quads) == want           # tests/test_dedisp_cpu.py holds tools/lds_sim.py to the same


def test_the_tile_fits_at_every_border():
    """On both sides of every border a column holds its TILE + spread rows and the chunk's columns with the zeros behind
    them fit the form's LDS and not the smaller one; at 3776 the tile is the whole 64 KiB to the last word.  The lone
    form's columns are TILE rows."""
    for (chunk, lds), last, beyond in BORDERS[:-1]:
        for spread in (last, beyond):
            c, l, stride = forms.form(spread, 1)
            if c == "lone":                                      # behind the last border: below
                continue
            assert stride >= TILE + spread and c * stride + TILE <= l // 4, spread
            assert l == SMALL_LDS or c * stride + TILE > forms.SMALL_WORDS, spread
        assert forms.form(last, 1)[:2] == (chunk, lds) != forms.form(beyond, 1)[:2]
        # one row more does not fit this form's LDS with this chunk
        assert chunk * forms.fit_stride(TILE + beyond, chunk // 4) + TILE > lds // 4
    assert forms.form(3776, 1) == (4, BIG_LDS, 4032) and 4 * 4032 + TILE == forms.BIG_WORDS
    c, l, stride = forms.form(3777, 1)
    assert c == "lone" and stride >= TILE and 32 * stride + TILE <= l // 4
    # the staging loop covers 4 * 256 / quads rows a pass: the spreads of STAGING end a column 0 and 1 rows into a pass
    for quads, spreads in forms.STAGING.items():
        for spread in spreads:
            assert forms.form(spread, 1)[0] == 4 * quads and (TILE + spread) % (4 * 256 // quads) == spread % 2, spread


def _plan(built, delays, mask=None, nout=NOUT):
    rc, blocks, threads, lds, tile, per, most = built.dedisp_geometry(delays, mask, nout)
    assert rc == 0 and threads == 256 and tile == TILE and blocks == -(-nout // TILE) * -(-delays.shape[0] // per)
    return per, lds, most


def test_geometry_of_every_case(built):
    """rtlws_dedisp_geometry of every table of the list: the trials a workgroup and the LDS the rule says, the table's
    largest delay, the workgroups of nout and one output.  One trial a workgroup changes its LDS at every border, so
    the list holds every chunk width without the library saying which it took."""
    for case in CASES:
        delays = forms.table(case)
        assert delays.shape == (case.ntrials, NCHAN) and delays.dtype == np.int32
        want = forms.form(case.plan_spread, case.plan_per)
        assert _plan(built, delays) == (case.plan_per, want[1], int(delays.max())), forms.case_id(case)
        assert _plan(built, delays, None, 1)[:2] == (case.plan_per, want[1])
        # the table is what it says: per trials spread `spread` inside the delayed quad and nowhere else, 2 per do not fit
        p = forms.delayed_position(case)
        quad = slice(p & ~3, (p & ~3) + 4)
        for t0 in range(0, case.ntrials, case.per):
            group = delays[t0:t0 + case.per]
            whole = t0 + case.per <= case.ntrials
            assert int(group[:, quad].max() - group[:, quad].min()) == (case.spread if whole else 0), forms.case_id(case)
            rest = np.delete(group, np.arange(NCHAN)[quad], axis=1)
            assert int(rest.max() - rest.min()) == (0 if case.kind == "border" or not whole else 1)
        if case.ntrials >= 2 * case.per:
            assert int(delays[case.per, 0] - delays[0, 0]) == forms.STEP > 247


def test_a_masked_outlier_is_no_spread(built):
    """The mask takes the delayed position out of the spread: every border table then gets the plan of the table
    without the delay, and max_delay forgets it."""
    for case in CASES:
        if case.kind != "border":
            continue
        delays = forms.table(case)
        mask = np.ones(NCHAN, np.uint8)
        mask[forms.delayed_position(case)] = 0
        flat = delays.copy()
        flat[:, forms.delayed_position(case)] = flat[:, 1]
        want = (case.per, SMALL_LDS, forms.STEP * ((case.ntrials - 1) // case.per))
        assert _plan(built, delays, mask) == _plan(built, flat) == want, forms.case_id(case)


def test_the_list_stands_on_every_border():
    ids = [forms.case_id(c) for c in CASES]
    assert len(set(ids)) == len(ids) == 94
    assert all(re.fullmatch(r"(border|drop)-per[1248]-spread\d+-(first|last)-\d+trials", i) for i in ids)
    seen = {}
    for case in CASES:
        chunk, lds, _ = forms.form(case.plan_spread, case.plan_per)
        seen.setdefault((case.plan_per, chunk, lds), set()).add((case.plan_spread, case.place))
    # one trial a workgroup: every form at the last spread it serves and at the first one of the form behind it, the
    # first spread it serves and the last one of the form before it, with both placements
    first = 0
    for (chunk, lds), last, beyond in BORDERS:
        mine = seen[(1, chunk, lds)]
        for place in forms.PLACES:
            assert (first, place) in mine or first == 0, (chunk, lds)
            assert (last, place) in mine or beyond is None, (chunk, lds)
        first = beyond
    assert {s for s, _ in seen[(1, 32, SMALL_LDS)]} == {23} and {s for s, _ in seen[(1, "lone", SMALL_LDS)]} == {3777}
    for spreads in forms.STAGING.values():
        for spread in spreads:
            assert all((spread, place) in seen[(1, forms.form(spread, 1)[0], forms.form(spread, 1)[1])] for place in forms.PLACES)
    # groups: both LDS sizes on both sides of 23 | 24 and the last spread served, and what 248 becomes
    for per in (8, 4, 2):
        for place in forms.PLACES:
            assert {(s, place) for s in (0, 1, 23)} <= seen[(per, 32, SMALL_LDS)] and {(s, place) for s in (24, 247)} <= seen[(per, 32, BIG_LDS)]
            mine = [c for c in CASES if c.per == per and c.spread == 248 and c.place == place]
            assert sorted((c.kind, c.plan_per, c.plan_spread) for c in mine) == [("border", 1, 248), ("drop", per // 2, 247)]
    assert {k[0] for k in seen} == {8, 4, 2, 1}
    assert {k[1:] for k in seen if k[0] == 1} == {f for f, _, _ in BORDERS}
    # whole groups only, and a last group of fewer trials
    assert {c.ntrials for c in CASES if c.per > 1} == {9, 8, 4, 2} and {c.ntrials for c in CASES if c.per == 1} == {1, 9}
    # the six forms the signed, special and masked runs take, and their masks keep the form
    assert [forms.form(c.plan_spread, c.plan_per)[:2] + (c.plan_per,) for c in forms.SIX_FORMS] == [
        (32, SMALL_LDS, 8), (32, BIG_LDS, 8), (32, BIG_LDS, 2), (16, SMALL_LDS, 1), (4, BIG_LDS, 1), ("lone", SMALL_LDS, 1)]
    assert all(c in CASES for c in forms.SIX_FORMS)


def test_the_masks_keep_the_form(built):
    """The masks of tests/test_dedisp_gpu.py::test_masked_positions_are_never_added leave something out of every chunk and
    keep the delayed position and one beside it, so that the six tables keep their plans"""
    for case in forms.SIX_FORMS:
        delays = forms.table(case)
        for name, mask in forms.masks(case):
            assert mask.dtype == np.uint8 and mask.shape == (NCHAN,) and 0 < mask.sum() < NCHAN, name
            assert _plan(built, delays, mask)[:2] == _plan(built, delays)[:2], (forms.case_id(case), name)
            assert dedisp_ref.rows_needed(delays, mask, NOUT) == dedisp_ref.rows_needed(delays, None, NOUT)
        by = dict(forms.masks(case))
        assert all(by["one of every quad"][q:q + 4].sum() == 3 for q in range(0, NCHAN, 4))
        assert sorted({int(by["whole quads"][q:q + 4].sum()) for q in range(0, NCHAN, 4)}) == [0, 4]
